"""Per-kernel resource table of one translation unit, from the assembly hipcc writes for it (no GPU needed).

    hipcc <build.FLAGS> --cuda-device-only -S neurite_amd/csrc/fused.hip -o fused.s
    python tools/kernel_digest.py fused.s > fused_kernels.txt
    python tools/kernel_digest.py --diff parent_kernels.txt fused_kernels.txt
    python tools/kernel_digest.py --tree CHECKOUT > tree_kernels.txt     # every csrc/*.hip of that checkout, names as `stem:kernel`

One line per kernel (demangled, sorted): VGPRs, SGPRs, spilled VGPRs, scratch bytes, LDS bytes, the occupancy the compiler reports
(waves per SIMD), instruction count and a hash of the instruction stream with the local labels renumbered, so that an untouched
kernel keeps its hash when its neighbours in the file change.  --diff lists the kernels whose line differs between two tables.
"""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FIELDS = ('vgpr', 'sgpr', 'spill', 'scratch', 'lds', 'occ', 'n')
LINE = re.compile(r'(.*?)\s+v(\d+)\s+s(\d+)\s+spill(\d+)\s+scr(\d+)\s+lds(\d+)\s+occ(\d+)\s+n(\d+)\s+(\w+)$')


def digest(path):
    txt = open(path).read()
    meta = {}
    for m in re.finditer(r'- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)', txt, re.S):
        blk = m.group(0)

        def get(key):
            return re.search(r'\.%s:\s+(\S+)' % key, blk).group(1)
        meta[get('name')] = dict(vgpr=int(get('vgpr_count')), sgpr=int(get('sgpr_count')), spill=int(get('vgpr_spill_count')),
                                 scratch=int(get('private_segment_fixed_size')), lds=int(get('group_segment_fixed_size')))
    rows = []
    for name, m in meta.items():
        i = txt.find('\n%s:' % name)
        j = txt.find('.Lfunc_end', i)
        body = re.sub(r'\.L([A-Za-z_]+)\d+_', r'.L\1_', txt[i:j])
        lines = [ln.split(';')[0].rstrip() for ln in body.splitlines()
                 if not ln.strip().startswith((';', '.')) or ln.strip().startswith('.LBB')]
        occ = re.search(r'; Occupancy: (\d+)', txt[j:])
        m['occ'] = int(occ.group(1)) if occ else 0
        m['n'] = sum(1 for ln in lines if ln.startswith('\t'))
        m['hash'] = hashlib.sha1('\n'.join(lines).encode()).hexdigest()[:12]
        rows.append(name)
    # _Float16 is mangled DF16_, which an older c++filt leaves as it is; Dh (the same type before clang 15; like DF16_ a builtin, so no
    # substitution index moves) it prints as `half`
    dem = subprocess.run(['c++filt'], input='\n'.join(r.replace('DF16_', 'Dh') for r in rows), capture_output=True, text=True).stdout.splitlines()
    out = []
    for name, d in zip(rows, dem):
        d = re.sub(r'\bhalf\b', '_Float16', d) if 'DF16_' in name else d
        d = re.sub(r'\(anonymous namespace\)::', '', d).split('(')[0].replace('void ', '')
        m = meta[name]
        out.append('%-62s v%-3d s%-3d spill%-2d scr%-4d lds%-6d occ%-2d n%-5d %s' %
                   (d, m['vgpr'], m['sgpr'], m['spill'], m['scratch'], m['lds'], m['occ'], m['n'], m['hash']))
    return sorted(out)


def load(path):
    table = {}
    for ln in open(path):
        m = LINE.match(ln.rstrip())
        if m:
            table[m.group(1).strip()] = dict(zip(FIELDS, (int(v) for v in m.groups()[1:8])), hash=m.group(9))
    return table


def diff(pa, pb):
    a, b = load(pa), load(pb)
    for k in sorted(set(a) ^ set(b)):
        print('only in %s: %s' % (pa if k in a else pb, k))
    moved = [k for k in sorted(a) if k in b and a[k] != b[k]]
    for k in moved:
        print('%-62s %s' % (k, '  '.join('%s %d -> %d' % (f, a[k][f], b[k][f]) for f in FIELDS if a[k][f] != b[k][f]) or 'hash only'))
    print('%d kernels in both, %d differ' % (len(set(a) & set(b)), len(moved)))


def tree(root):
    """the table of every translation unit of the checkout at `root`, each kernel prefixed by its file stem"""
    spec = importlib.util.spec_from_file_location('nrt_tree_build', os.path.join(root, 'neurite_amd', 'build.py'))    # not the package
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    hipcc = os.environ.get('HIPCC', 'hipcc')

    def one(src, tmp):
        out = os.path.join(tmp, os.path.basename(src)[:-4] + '.s')
        subprocess.run([hipcc] + build.FLAGS + ['--cuda-device-only', '-S', src, '-o', out], check=True)
        return ['%s:%s' % (os.path.basename(src)[:-4], row) for row in digest(out)]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(16) as pool:
        return sorted(row for rows in pool.map(lambda s: one(s, tmp), build.sources()) for row in rows)


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--diff':
        diff(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 3 and sys.argv[1] == '--tree':
        print('\n'.join(tree(os.path.abspath(sys.argv[2]))))
    elif len(sys.argv) == 2:
        print('\n'.join(digest(sys.argv[1])))
    else:
        raise SystemExit(__doc__)
