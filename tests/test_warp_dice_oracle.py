"""
CPU tests of oracle/warp_dice_oracle.py and tests/warp_dice_cases.py (the restated dispatch, the table and the references behind
tests/test_gpu_warp_dice_arms.py) -- the part of "every arm has an id" that needs no GPU, at 256 compute units: every instance of
warp_dice_tile, warp_dice_tile_pad and warp_dice_wc in the committed kernel table (profiles/dispatch_arms/fused_kernels.txt) is named by
an id or is one of the 96 documented unreachable ones; every id is what `plan` derives for its call; the premises of the data hold on the
references alone; and the restated workspace size and kernel name agree with the library's own host code, which runs without a device
(nrt_num_cus falls back to 256 there).
"""

import os
import re
import sys

import numpy as np
import pytest

import warp_dice_cases as cs
from oracle import warp_dice_oracle as wdo
from oracle.warp_dice_oracle import ABSOLUTE, LINSPACE, SHIFT, Call, tune_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402

F = np.float32
FAMILIES = ('warp_dice_tile', 'warp_dice_tile_pad', 'warp_dice_wc')


def family_instances():
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS['warp_dice']))
    found = set()
    for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', 'fused_kernels.txt')):
        m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
        if m and fam.match(arm_coverage.norm(m.group(1))):
            found.add(arm_coverage.norm(m.group(1)))
    return found


def family(name):
    return name.split('<')[0]


def test_case_table_names_every_emitted_instance():
    inst = family_instances()
    count = {f: sum(family(k) == f for k in inst) for f in FAMILIES}
    assert count == dict(warp_dice_tile=168, warp_dice_tile_pad=144, warp_dice_wc=60) and len(inst) == 372
    unreachable = re.compile('^(?:%s)$' % '|'.join(arm_coverage.UNREACHABLE['warp_dice']))
    assert sorted(k for k in inst if unreachable.match(k)) == wdo.UNREACHABLE and len(wdo.UNREACHABLE) == 96
    # 42 + 36 of them are the bfloat16 STORE = true forms, the other 18 the rest of warp_dice_tile_pad<2, ...>
    assert sum(',true,' in k and k.endswith('unsignedshort>') for k in wdo.UNREACHABLE) == 78
    assert len(set(cs.IDS)) == len(cs.IDS)
    named = set()
    for c in cs.CASES:
        p = wdo.plan(c.call, cs.CUS)
        assert c.id.startswith('%s L%d B%d O%s %s' % (p['instance'], c.call.L, c.call.B, 'x'.join(map(str, c.call.O)), wdo.tags(p))), c.id
        for kind, fill, eps in cs.runs(c):                          # every launch of an id is the id's instance
            q = wdo.plan(cs.run_call(c.call, kind), cs.CUS)
            if family(p['instance']) == 'warp_dice_wc':
                assert fill == c.call.fill
            assert q['instance'] == p['instance'] and wdo.tags(q) == wdo.tags(p), (c.id, kind)
        named.add(p['instance'])
    assert named == inst - set(wdo.UNREACHABLE), sorted(inst - set(wdo.UNREACHABLE) - named)


def test_unreachable_forms():
    """`plan` keeps to what was read in the dispatcher: 16-bit storage with `warped` is refused, and no label count reaches the padded
    entry point at G = 2"""
    assert wdo.plan(Call(32, (9, 9, 9), (7, 7, 11), dtype='bf16', store=True))['status'] == wdo.ERR_UNSUPPORTED
    for L in range(4, 257, 4):
        p = wdo.plan(Call(L, (9, 9, 9), (7, 7, 11)))
        assert p['G'] == wdo.fused_group(L) and (p['instance'].startswith('warp_dice_tile_pad<') == (p['Gr'] != p['G']))
        assert not p['instance'].startswith('warp_dice_tile_pad<2,')


def has(prefix, *words):
    return any(cid.startswith(prefix) and all(w in cid for w in words) for cid in cs.IDS)


def test_table_reaches_the_mechanisms():
    """the geometry the ids are there for, by the words of their tags"""
    for G in cs.GS:
        for ST in ('float', 'unsignedshort'):
            for mode in (0, 1, 2):
                assert has('warp_dice_tile<%d,%d,false,1,%s>' % (G, mode, ST)) and has('warp_dice_tile<%d,%d,false,3,%s>' % (G, mode, ST))
        # one pass (odd), two, and more than FUSED_SYNC; z_outer; an XCD slab with idle tiles; a partial tile on every side the tile has
        assert has('warp_dice_tile<%d,' % G, ' passes1 ', 'z_outer') and has('warp_dice_tile<%d,' % G, ' passes2 ')
        assert any(cid.startswith('warp_dice_tile<%d,' % G) and int(re.search(r' passes(\d+) ', cid).group(1)) > wdo.FUSED_SYNC for cid in cs.IDS if ' tile' in cid)
        assert has('warp_dice_tile<%d,' % G, 'partial-xyz') and any(cid.startswith('warp_dice_tile<%d,' % G) and re.search(r' idle[1-9]', cid) for cid in cs.IDS)
        # x-march: 1, 3 and a ragged 5 pieces, padding columns
        for w in (' seg1x7 ', ' seg3x3 ragged1 ', ' seg5x3 ragged1 '):
            assert has('warp_dice_tile<%d,' % G, 'xmarch', w), (G, w)
        assert any(cid.startswith('warp_dice_tile<%d,' % G) and re.search(r'ncol\d+\+[1-9]', cid) for cid in cs.IDS), G
    for G, L in cs.PAD_L.items():
        for mode in (0, 1, 2):
            for store in ('false', 'true'):
                assert has('warp_dice_tile_pad<%d,%d,%s,1,float> L%d ' % (G, mode, store, L)) and has('warp_dice_tile_pad<%d,%d,%s,3,float> L%d ' % (G, mode, store, L))
    for L in (24, 28, 252):
        assert has('warp_dice_tile_pad<', ' L%d ' % L, ' tile') and has('warp_dice_tile_pad<', ' L%d ' % L, 'xmarch')
    assert has('warp_dice_tile<8,1,false,1,float>', 'tile4x8x5 passes5', 'tiles2x2x3', 'plane_major') and has('warp_dice_tile<4,', 'plane_major asked for and ignored')
    assert not any('plane_major' in wdo.tags(wdo.plan(c.call)) for c in cs.CASES if c.call.L != 32)
    for G in (64, 16):
        assert has('warp_dice_tile<%d,1,false,1,float>' % G, 'grid2048 x2', 'cap')
    for w in (' B1 ', ' B3 ', 'loc_batch_stride 0'):
        assert has('warp_dice_tile<4,1,true,1,float>', w) and has('warp_dice_tile<4,1,false,3,float>', w)
    for inst in ('warp_dice_tile<8,1,true,3,float>', 'warp_dice_wc<1,true,', 'warp_dice_tile<1,1,true,3,float>', 'warp_dice_tile<16,', 'warp_dice_tile_pad<4,'):
        assert has(inst, '(widened)', ' seg1x7 ') and has(inst.replace('true', 'false'), '(widened)', ' seg3x3 ragged1 '), inst
    assert has('warp_dice_tile<', 'clamp', ' seg7x1 ') and has('warp_dice_tile<8,', 'patch8x8') and has('warp_dice_tile_pad<8,', 'patch8x8')
    # mixed lengths
    for inst in ('warp_dice_tile<8,1,false,3,float>', 'warp_dice_tile<8,1,false,3,unsignedshort>', 'warp_dice_tile_pad<8,1,false,3,float>',
                 'warp_dice_tile_pad<8,1,false,3,unsignedshort>', 'warp_dice_wc<'):
        assert has(inst, 'mixed', ' full0 ', ' seg8x2 ragged-1 ') and has(inst, 'mixed', ' cpx66 full64 ', 'padrows0/8')
    assert has('warp_dice_tile<8,1,false,3,float>', ' short3 ') and has('warp_dice_wc<', ' short3 ', 'persist')
    assert has('warp_dice_wc<', 'default word', ' full0 ') and has('warp_dice_wc<', 'default word', 'padrows0/56', 'persist')
    assert has('warp_dice_tile<8,1,false,3,unsignedshort>', 'default word', 'padrows0/56') and has('warp_dice_tile_pad<8,1,false,3,float> L24', 'default word')
    # the wave-cache kernel: persistent and not through both set-ups, a short list
    for mode in (0, 1, 2):
        for w in (('xmarch', 'persist'), ('mixed', 'persist'), ('xmarch',), ('mixed',)):
            assert any(cid.startswith('warp_dice_wc<%d,' % mode) and all(x in cid for x in w) and ('persist' in cid) == ('persist' in w) for cid in cs.IDS), (mode, w)
    assert has('warp_dice_wc<1,', 'last list 4 items short', 'persist')
    # tune bit 30 keeps the register kernel where the wave-cache kernel applies, bit 29 changes nothing
    c = Call(32, (9, 9, 9), (7, 7, 19), tune=cs.xm_word('x1')[0])
    assert wdo.plan(c)['instance'].startswith('warp_dice_wc<') and wdo.plan(Call(32, c.S, c.O, tune=c.tune | cs.WC)) == wdo.plan(c)
    assert wdo.plan(Call(32, c.S, c.O, tune=c.tune | cs.NO_WC))['instance'] == 'warp_dice_tile<8,1,false,3,float>'
    assert sum(bool(c.call.tune > 0 and c.call.tune & cs.WC) for c in cs.CASES) >= 12


def test_plan_by_hand():
    """figures derived by hand from fused_geom, xmarch_setup and xmarch_setup_mixed"""
    p = wdo.plan(Call(256, (9, 9, 9), (13, 29, 22), tune=tune_word(0, 0, 2)))
    assert p['tiles'] == 8 * 48 * 6 and p['grid'] == 2048 and p['per_block'] == 2 and p['nblocks'] == 2048
    p = wdo.plan(Call(32, (9, 9, 9), (5, 14, 30), B=33, tune=cs.xm_word('mixed')[0]))
    assert (p['het_cpx'], p['het_full'], p['nseg'], p['items_x'], p['prows']) == (66, 64, 5, 74, 16 + 2 * 4) and p['persist']
    assert sorted(set(p['split'])) == [0, 2] and p['split'][4] == 2 and p['split'][0] == 0
    assert not wdo.plan(Call(32, (9, 9, 9), (5, 14, 30), B=33, tune=cs.xm_word('mixed')[0]), cus=304)['persist']      # 8 x 74 <= 608
    p = wdo.plan(Call(32, (9, 10, 11), (16, 32, 64), B=9))
    assert (p['het_cpx'], p['het_full'], p['nseg'], p['seglen']) == (72, 64, 8, 2) and p['padrows'][0] == 56 and set(p['padrows'][1:]) == {0}
    p = wdo.plan(Call(32, (9, 10, 11), (16, 32, 64), B=8))
    assert (p['het_full'], p['nseg'], p['items_x'], p['persist']) == (0, 1, 64, False)
    assert wdo.workspace_bytes(3, 32, 2) == 6 * 96 * 4 + 6 * 16 + 16 + 2 * 96 * 8 + 2 * 16 + 256


def test_refused_calls_plan():
    for name, c, want in cs.REFUSED:
        assert wdo.plan(c).get('status', wdo.OK) == want, name
    assert [w for _, c, w in cs.REFUSED].count(wdo.OK) == 1


def test_library_host_code_agrees():
    """nrt_warp_dice_workspace_bytes and nrt_warp_dice_kernel_name are host code: they run without a device, where nrt_num_cus falls back
    to 256 -- the count of this table.  With a device of another count the rows whose plan depends on the count are skipped here (the
    GPU file asserts every row with the device's count)."""
    from neurite_amd import _lib
    lib = _lib.lib()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else cs.CUS
    checked = 0
    for c in cs.CASES:
        k = c.call
        if k.entry != 'dice':
            continue
        p = wdo.plan(k, cs.CUS)
        if cus != cs.CUS and wdo.plan(k, cus) != p:               # (mixed lengths and `persist` depend on the count)
            continue
        assert lib.nrt_warp_dice_workspace_bytes(_lib.ints(k.O), k.L, k.B, k.tune) == p['ws'], c.id
        if k.dtype == 'f32':
            for kind in ('exact', 'grid'):
                S = cs.run_call(k, kind).S
                name = lib.nrt_warp_dice_kernel_name(_lib.ints(k.O), _lib.ints(S), k.L, k.B, k.mode, int(k.fill), int(k.store), int(k.minmax), k.tune)
                assert arm_coverage.norm(name.decode()) == p['instance'], c.id
        checked += 1
    assert checked >= 200 or cus != cs.CUS
    assert lib.nrt_warp_dice_kernel_name(_lib.ints((7, 7, 7)), _lib.ints((9, 9, 9)), 5, 1, 1, 0, 0, 1, 0) == b''


def _premises(c):
    """the premises of one case on its references alone: (outside share, least unequal-weight share) of the exact run"""
    k = c.call
    shares = []
    for kind, fill, eps in cs.runs(c):
        rc = cs.run_call(k, kind)
        inp = cs.inputs(k, kind, fill)
        what = '%s %s fill %d' % (c.id, kind, fill)
        if k.mode != LINSPACE:
            out = cs.outside_share(rc.S, inp.absloc)
            assert 0.15 <= out <= 0.75, '%s: %.2f of the voxels sample outside the volume' % (what, out)
            shares.append(('outside ' + ('exact' if kind == 'exact' else 'random'), out))
        else:
            assert cs.outside_share(rc.S, inp.absloc) == 0.0                      # LINSPACE never leaves the volume: the documented exemption
            if kind in ('grid', 'coarse'):                                                 # a step that is not dyadic and does not repeat within O - 1 voxels
                for s, o in zip(rc.S, rc.O):
                    assert np.gcd(s - 1, o - 1) == 1 and (o - 1) & (o - 2), (what, s, o)
            else:
                assert all(o == 2 * s - 1 for s, o in zip(rc.S, rc.O)), what
        if k.entry != 'dice':
            continue
        r = inp.ref
        nz = np.ones(k.L, bool)
        if inp.zero_label is not None:
            nz[inp.zero_label] = False
            assert (r['sums'][:, :, inp.zero_label] == 0).all()
        assert (r['sums'][:, :, nz] != 0).all(), what + ': a label with a zero sum'
        if kind == 'exact':
            wdo.assert_exact(r)
            assert (r['sums'].astype(F).astype(np.float64) == r['sums']).all()
            assert wdo.extrema_unique(inp.fix, inp.warped), what + ': an extremum in more than one place'
            assert fill or k.L == 4 or inp.zero_label is not None
            u = cs.unequal_weight_share(rc.S, inp.absloc)
            assert (u >= 0.25).all(), '%s: blend weights differ on %s of the voxels' % (what, u)
            shares.append(('unequal weights', float(u.min())))
    return shares


def _pieces(c, p):
    if p['schedule'] == 'xmarch' or p['het_full'] == 0:
        return [(i * p['seglen'], min(p['seglen'], c.O[0] - i * p['seglen'])) for i in range(p['nseg'])]
    return [(0, c.O[0])]                                              # (whole columns and a few split ones: counted as whole)


def test_wave_cache_regimes():
    """every wave-cache id with per-voxel locations has passes without an orphan (rows served from the cache), with 1 .. 16 (overflow rows)
    and with more than 16 (the cache forgotten, 64 references fetched as they are), counted from the locations of its first batch entry;
    LINSPACE meets the last two on its coarse grid only"""
    seen, lo = {}, [1.0, 1.0, 1.0]
    for c in cs.CASES:
        if family(cs.inst_of(c.id)) != 'warp_dice_wc' or c.call.entry != 'dice':
            continue
        tot = np.zeros(3)
        for kind, fill, eps in cs.runs(c):
            rc = cs.run_call(c.call, kind)
            p = wdo.plan(rc, cs.CUS)
            key = (rc.S, rc.O, rc.mode, kind, fill, p['schedule'], p['nseg'])
            if key not in seen:
                no = wdo.wc_orphans(rc.S, rc.O, cs.inputs(c.call, kind, fill).absloc[0], _pieces(rc, p))
                seen[key] = np.array([(no == 0).sum(), ((no > 0) & (no <= 16)).sum(), (no > 16).sum()])
            if rc.mode == LINSPACE and kind != 'coarse':
                assert seen[key][1:].sum() == 0
            tot += seen[key]
        if c.call.mode != LINSPACE or 'coarse' in c.kinds:
            assert (tot / tot.sum() >= 0.01).all(), (c.id, tot)
            lo = [min(a, b) for a, b in zip(lo, tot / tot.sum())]
    assert any('coarse' in c.kinds for c in cs.CASES)
    print('REGIMES least share of passes per id: no orphan %.2f, 1 .. 16 %.2f, more %.2f' % tuple(lo))


@pytest.mark.parametrize('fam', FAMILIES)
def test_premises_hold_on_every_reference(fam):
    seen = {}
    for c in cs.CASES:
        if family(cs.inst_of(c.id)) != fam:
            continue
        for k, v in _premises(c):
            lo, hi = seen.get(k, (v, v))
            seen[k] = (min(lo, v), max(hi, v))
    print('PREMISES %-20s %s' % (fam, '  '.join('%s %.2f-%.2f' % (k, lo, hi) for k, (lo, hi) in sorted(seen.items()))))


def test_reference_against_the_unfused_oracle():
    """warp_ref is the C oracle's interpn and soft_ref its Dice sums: against oracle.np_oracle on one small case per mode"""
    from oracle import np_oracle as npo
    for mode in (ABSOLUTE, SHIFT, LINSPACE):
        c = Call(12, (6, 7, 8), (7, 7, 11), B=2, mode=mode, fill=True)
        inp = cs.inputs(c, 'grid' if mode == LINSPACE else 'incoherent', True)
        rc = cs.run_call(c, 'grid')
        for b in range(2):
            want = npo.interpn(inp.mov[b], inp.absloc[b], 'linear', cs.FILL_RANDOM)
            assert np.array_equal(want.view(np.uint32), inp.warped[b].view(np.uint32)), (mode, rc)
        t, p = inp.fix.astype(np.float64).reshape(2, -1, 12), inp.warped.astype(np.float64).reshape(2, -1, 12)
        np.testing.assert_allclose(inp.ref['sums'], np.stack([(t * p).sum(1), (t * t).sum(1), (p * p).sum(1)], 1), rtol=1e-14)
