"""
Timing of fused.warp_labels, utils.resize_labels and fused.fuse_labels (csrc/warp_argmax.hip) against the pipelines they replace.

    python tools/warp_labels_bench.py [--reps 10] [--out profiles/warp_labels/warp_labels_bench.jsonl] [--cases NAME,...]
    python tools/warp_labels_bench.py --dry     # CPU rehearsal: cases, byte counts, the inputs at a toy size; measures nothing

Cases (32 labels; blob labels and the smooth field of synth are the bench recipe):
    bench_4x160, bench_1x160   blob labels under the smooth field
    iid_4x160                  i.i.d. label ids under the smooth field (up to 8 labels per voxel, no wave takes the fast path)
    rough_4x160                blob labels under synth.rough_displacement (incoherent gathers)
    affine_4x160               blob labels under an affine matrix, the location formed in registers
    resize_80_to_160           resize_labels(ids, 2) of one 80^3 map
    fuse_4x160, fuse_16x160    fuse_labels of 4 / 16 atlases, each under its own smooth field
Alternatives, in the same process on the same inputs, alternated inside every repetition after a warm-up of all of them, device events:
    labels / labels_prob       warp_labels (nb_labels=32) without / with the winner's value
    labels_any                 warp_labels where every int32 value is a label (nb_labels=None)
    onehot / onehot_build      the pipeline it replaces, SpatialTransformer('linear') -> seg.pred_to_label on a float32 one-hot map built
                               beforehand / built on the device inside the timed region (affine: the layer on the matrix; resize: layers.Resize)
    nearest                    SpatialTransformer('nearest') on the ids as float32 [B, X, Y, Z, 1]: the cheap, biased alternative
    warp_dice_labels           the forward of the sibling kernel on the same maps (it does strictly more work per voxel)
    fuse / fuse_votes          fuse_labels without / with the votes; onehot / onehot_build: N one-hot warps accumulated by torch
                               (weights all 1) and one seg.pred_to_label
The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that fails
or runs out of time.  A child first checks that `labels` returns the ids of `onehot` (the share of differing voxels goes into the record:
0 is expected), then times and appends one JSON line: median / min / max ms of every alternative, the ratio of `labels` (or `fuse`) to
each, and the share of the 8 TB/s HBM peak that the algorithmic bytes (20 B per voxel: 12 B of field, 4 B of id in, 4 B of id out; 24 B
with prob; 8 B where the location is formed in registers; fusion 16 N + 4) over the median come to.  A time needs a GPU: without one the
tool fails.
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib, synth                                                                # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
L = 32
# name: (kind, batch or atlases, size)
CASES = {
    'bench_4x160': ('warp', 4, 160),
    'bench_1x160': ('warp', 1, 160),
    'iid_4x160': ('iid', 4, 160),
    'rough_4x160': ('rough', 4, 160),
    'affine_4x160': ('affine', 4, 160),
    'resize_80_to_160': ('resize', 1, 80),
    'fuse_4x160': ('fuse', 4, 160),
    'fuse_16x160': ('fuse', 16, 160),
}


def label_maps(kind, n, size, dev):
    """int32 label maps [n, S, S, S]"""
    if kind == 'iid':
        g = torch.Generator(device=dev).manual_seed(0)
        return torch.randint(0, L, (n, size, size, size), generator=g, device=dev, dtype=torch.int32)
    return torch.stack([synth.blob_labels(100 + 3 * b, size, L, device=dev) for b in range(n)]).to(torch.int32)


def fields(kind, n, size, dev):
    make = synth.rough_displacement if kind == 'rough' else synth.smooth_displacement
    return torch.stack([make(102 + 3 * b, size, device=dev) for b in range(n)])


def matrices(n, dev):
    """small rotations, scales and shifts around the identity"""
    rng = np.random.default_rng(5)
    m = np.eye(3, 4, dtype=np.float32)[None] + rng.normal(0, 0.02, (n, 3, 4)).astype(np.float32)
    m[:, :, 3] += rng.normal(0, 3.0, (n, 3)).astype(np.float32)
    return torch.from_numpy(m).to(dev)


def one_hot(lab):
    out = torch.zeros(tuple(lab.shape) + (L,), dtype=torch.float32, device=lab.device)
    out.scatter_(-1, lab.long().unsqueeze(-1), 1.0)
    return out


def eager(fn):
    with ne.deferred.scope(False):
        return fn()


def make_alternatives(kind, n, size, dev):
    """({name: callable}, name of the new op, name of the reference, bytes per voxel of the new op, output voxels)"""
    ids = label_maps(kind, n, size, dev)
    if kind == 'fuse':
        trfs = fields(kind, n, size, dev)

        def votes_by_torch(maps):
            V = None
            for a in range(n):
                w = eager(lambda: ne.layers.SpatialTransformer()([maps(a), trfs[a:a + 1]]))
                V = w if V is None else V.add_(w)
            return ne.seg.pred_to_label(V)[0][0]

        M = [one_hot(ids[a:a + 1]) for a in range(n)]
        fns = {'fuse': lambda: ne.fused.fuse_labels(ids, trfs, nb_labels=L),
               'fuse_votes': lambda: ne.fused.fuse_labels(ids, trfs, nb_labels=L, return_votes=True)[0],
               'fuse_any': lambda: ne.fused.fuse_labels(ids, trfs),
               'onehot': lambda: votes_by_torch(lambda a: M[a]),
               'onehot_build': lambda: votes_by_torch(lambda a: one_hot(ids[a:a + 1]))}
        return fns, 'fuse', 'onehot', {'fuse': 16 * n + 4, 'fuse_votes': 16 * n + 8, 'fuse_any': 16 * n + 4}, size ** 3
    if kind == 'resize':
        M = one_hot(ids)
        layer = ne.layers.Resize(2)
        fns = {'labels': lambda: ne.utils.resize_labels(ids[0], 2, nb_labels=L),
               'labels_any': lambda: ne.utils.resize_labels(ids[0], 2),
               'onehot': lambda: ne.seg.pred_to_label(layer(M))[0][0],
               'onehot_build': lambda: ne.seg.pred_to_label(layer(one_hot(ids)))[0][0]}
        return fns, 'labels', 'onehot', {'labels': 8, 'labels_any': 8}, (2 * size) ** 3
    M = one_hot(ids)
    st, st_nearest = ne.layers.SpatialTransformer(), ne.layers.SpatialTransformer('nearest')
    if kind == 'affine':
        mat = matrices(n, dev)
        fns = {'labels': lambda: ne.fused.warp_labels(ids, mat, nb_labels=L),
               'labels_prob': lambda: ne.fused.warp_labels(ids, mat, nb_labels=L, return_prob=True)[0],
               'labels_any': lambda: ne.fused.warp_labels(ids, mat),
               'onehot': lambda: ne.seg.pred_to_label(eager(lambda: st([M, mat])))[0],
               'onehot_build': lambda: ne.seg.pred_to_label(eager(lambda: st([one_hot(ids), mat])))[0]}
        return fns, 'labels', 'onehot', {'labels': 8, 'labels_prob': 12, 'labels_any': 8}, n * size ** 3
    trf = fields(kind, n, size, dev)
    fixed = torch.roll(ids, 7, dims=1).contiguous()
    as_float = ids.to(torch.float32).unsqueeze(-1)
    fns = {'labels': lambda: ne.fused.warp_labels(ids, trf, nb_labels=L),
           'labels_prob': lambda: ne.fused.warp_labels(ids, trf, nb_labels=L, return_prob=True)[0],
           'labels_any': lambda: ne.fused.warp_labels(ids, trf),
           'onehot': lambda: ne.seg.pred_to_label(eager(lambda: st([M, trf])))[0],
           'onehot_build': lambda: ne.seg.pred_to_label(eager(lambda: st([one_hot(ids), trf])))[0],
           'nearest': lambda: st_nearest([as_float, trf]),
           'warp_dice_labels': lambda: ne.fused.warp_dice_labels(ids, trf, fixed, L)}
    return fns, 'labels', 'onehot', {'labels': 20, 'labels_prob': 24, 'labels_any': 20}, n * size ** 3


def timed(fns, reps):
    """median / min / max ms of each of `fns` (name -> callable), alternated inside every repetition"""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1))
    return {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()}


def run_case(name, reps):
    kind, n, size = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('warp_labels_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    fns, new, ref, nbytes, nvox = make_alternatives(kind, n, size, dev)
    rec = {'case': name, 'inputs': kind, 'maps': n, 'size': size, 'labels': L, 'reps': reps, 'output_voxels': nvox,
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    got, want = fns[new](), fns[ref]()
    rec['share_of_voxels_differing_from_' + ref] = float((got.long() != want.long()).float().mean())
    del got, want
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = timed(fns, reps)
    rec['ms'] = t
    rec['over'] = {k: {b: t[k]['median'] / v['median'] for b, v in t.items() if b not in nbytes} for k in nbytes}
    rec['algorithmic_bytes_per_voxel'] = nbytes
    rec['hbm_peak_share'] = {k: nbytes[k] * nvox / (t[k]['median'] * 1e-3) / HBM_PEAK for k in nbytes}
    rec['faster_than_' + ref] = t[new]['median'] < t[ref]['median']
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts, and the inputs at a toy size on the CPU"""
    for c in names:
        kind, n, size = CASES[c]
        ids = label_maps(kind, 2, 12, 'cpu')
        M = one_hot(ids)
        assert ids.dtype == torch.int32 and ids.shape == (2, 12, 12, 12) and fields(kind, 2, 12, 'cpu').shape == (2, 12, 12, 12, 3)
        assert M.shape == (2, 12, 12, 12, L) and bool((M.sum(-1) == 1).all()) and bool((M.argmax(-1) == ids).all())
        assert matrices(2, 'cpu').shape == (2, 3, 4)
        nvox = n * size ** 3
        print('%-18s %-6s %2d x %d^3  ids %7.1f MB  one-hot f32 %8.1f MB' % (c, kind, n, size, nvox * 4 / 1e6, nvox * L * 4 / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_labels', 'warp_labels_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--case')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args.reps)))
        return
    names = [c for c in args.cases.split(',') if c]
    for c in names:
        if c not in CASES:
            raise SystemExit('unknown case %s (known: %s)' % (c, ', '.join(CASES)))
    if args.dry:
        dry(names)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('warp_labels_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('warp_labels_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-18s ' % c + '  '.join('%s %.3f' % (k, v['median']) for k, v in r['ms'].items()) + ' ms;  ' +
              '  '.join('%s %.3f of the HBM peak' % (k, v) for k, v in r['hbm_peak_share'].items()))


if __name__ == '__main__':
    main()
