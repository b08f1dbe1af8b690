"""
CPU tests of oracle/warp_fwd_oracle.py (the restated dispatch and the reference behind tests/test_gpu_warp_forward_arms.py) -- the part of
"every arm has an id" that needs no GPU: every instance of the nine warp-forward families in the three committed kernel tables
(profiles/dispatch_arms/interpn_kernels.txt, interpn_lean_kernels.txt, interpn_any_kernels.txt) is the written instance of a case of the
GPU file or one of the 18 documented unreachable ones; every case's written instance is what `plan` derives for each of its launches; and
the premises of the GPU file hold on the reference of every launch.
"""

import dataclasses
import os
import re
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle import warp_fwd_oracle as wfo
from oracle.warp_fwd_oracle import ABSOLUTE, LINEAR, LINSPACE, NEAREST, SHIFT, Call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402
import test_gpu_warp_forward_arms as arms                                                 # noqa: E402  (the case table; nothing is launched)

F = np.float32
TABLES = ('interpn_kernels.txt', 'interpn_lean_kernels.txt', 'interpn_any_kernels.txt')
FAMILY_OF = re.compile(r'^(\w+?)(?:<|$)')


def family_instances():
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS['warp_fwd']))
    found = set()
    for t in TABLES:
        for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', t)):
            m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
            if m and fam.match(arm_coverage.norm(m.group(1))):
                found.add(arm_coverage.norm(m.group(1)))
    return found


def test_case_table_names_every_emitted_instance():
    inst = family_instances()
    count = {}
    for k in inst:
        count[FAMILY_OF.match(k).group(1)] = count.get(FAMILY_OF.match(k).group(1), 0) + 1
    assert count == dict(interpn_generic=27, interpn_rows=42, interpn_tile=21, interpn_zrun_c32=12, interpn_lean_tile=24, interpn_lean=27,
                         interpn_any_nd=48, interpn_any=8, interpn_any_nearest_i32=1) and len(inst) == 210
    unreachable = re.compile('^(?:%s)$' % '|'.join(arm_coverage.UNREACHABLE['warp_fwd']))
    assert sorted(k for k in inst if unreachable.match(k)) == wfo.UNREACHABLE and len(wfo.UNREACHABLE) == 18
    assert len(set(arms.IDS)) == len(arms.IDS) == len(arms.CASES)
    named = set()
    for cid, cs in zip(arms.IDS, arms.CASES):
        p = wfo.plan(cs.call)
        assert cid.startswith(wfo.plan_id(p)), cid
        if p.status:
            assert p.status == cs.want and not p.names, cid
            continue
        assert p.names == (cs.want,) and cs.want in inst, (cid, p)
        named.add(cs.want)
        for c, kind, fill in arms.subcalls(cs):                   # the extras of an id launch the id's instance
            assert wfo.plan(c).names == p.names, (cid, c)
    assert named == inst - set(wfo.UNREACHABLE), sorted(inst - set(wfo.UNREACHABLE) - named)


def test_unreachable_row_forms():
    """`plan` keeps to what was read in nrt_lean_launch (its first statement sends every call with per-voxel locations to interpn_lean_tile):
    it names no row form in ABSOLUTE or SHIFT mode.  This guards the restatement against an edit; the proof that the 18 instances are
    unreachable is the reading of the dispatcher (profiles/dispatch_arms/README.md), not this test."""
    for mode in (ABSOLUTE, SHIFT):
        for C in (1, 2, 3, 4):
            for O in ((13, 11, 8), (13, 11, 6), (13, 11, 7), (3, 3, 4), (5, 6, 1), (3, 130, 8)):
                for kw in ({}, dict(loc_pad=1), dict(shared_loc=True), dict(B=1)):
                    for entry in ('f32', 'add', 'i32'):
                        c = Call(entry, (9, 8, 7), O, C, mode, NEAREST if entry == 'i32' else LINEAR, 'i32' if entry == 'i32' else 'f32', **kw)
                        name = wfo.plan(c).names[0]
                        assert name.startswith('interpn_lean_tile<') or (entry == 'add' and name.startswith('interpn_generic<')), (c, name)


def test_plan_geometry():
    """the geometry the ids are there for, derived by hand from the launchers"""
    def has(prefix, *words):
        return any(cid.startswith(prefix) and all(w in cid for w in words) for cid in arms.IDS)
    assert has('interpn_generic<3,1,0,float> passes2')
    assert has('interpn_rows<1,1,0> vpb256 blocks2 last39')
    for G, tile in ((1, '4x4x64'), (2, '4x4x32'), (4, '4x4x16'), (64, '4x4x16')):
        for mode in (0, 1, 2):
            assert has('interpn_tile<%d,%d> tile%s' % (G, mode, tile), 'partial-xyz'), (G, mode)
    for G in (1, 2, 4, 8, 16, 32, 64):
        assert has('interpn_tile<%d,1>' % G, ' passes1 ', 'z_outer'), G
    assert has('interpn_tile<8,1> tile4x8x5 passes5', 'plane_major') and has('interpn_tile<8,1> tile4x8x17 passes17', 'plane_major')
    assert has('interpn_tile<2,1>', 'auto 4096 voxels') and has('interpn_rows<2,1,0>', 'auto 4095 voxels')
    for patch in (0, 1, 2, 3):
        for w in ('LZ27 zchunks1', 'LZ5 zchunks6 ', 'zc_outer1'):
            assert has('interpn_zrun_c32<1,%d,%d> patch%d' % (wfo.ZRUN_PATCH[patch] + (patch,)), w), (patch, w)
    assert has('interpn_zrun_c32<1,2,4>', 'lreg1 pad4', 'B1') and has('interpn_zrun_c32<1,2,4>', 'lreg1 pad4', 'B3') and has('interpn_zrun_c32<1,4,2>', 'lreg2 pad12')
    assert has('interpn_zrun_c32<1,4,4>', 'lds64K(attr)') and has('interpn_zrun_c32<1,2,2>', 'lds40K')
    for tpb in (1, 2, 4):
        assert has('interpn_lean_tile<1,1,0>', 'tpb%d ' % tpb), tpb
    assert {re.search(r'ltz(\d) lty(\d)', cid).groups() for cid in arms.IDS if cid.startswith('interpn_lean_tile<1,1,0>')} == {('5', '2'), ('4', '3'), ('2', '3'), ('0', '3'), ('3', '1'), ('3', '0'), ('3', '3')}
    for C, V in ((1, 4), (1, 1), (2, 4), (2, 2), (2, 1), (3, 4), (3, 1), (4, 4), (4, 1)):
        assert has('interpn_lean<%d,%d,2>' % (C, V), 'lpr1 '), (C, V)
        assert V == 2 or has('interpn_lean<%d,%d,2>' % (C, V), 'cpp2'), (C, V)
    for T in wfo.TNAME.values():
        for why in ('C%4', 'ptr%32', 'stride%4'):
            assert has('interpn_any_nd<%s,false,3,1> CG1(%s)' % (T, why)), (T, why)
    # outside the families
    assert wfo.plan(Call('f32', (16, 128, 128), (16, 128, 128), 32)).names[0].startswith('not warp_fwd')
    assert wfo.plan(Call('f32_ex', (9, 8, 7), (7, 6, 7), 3, variant=7)).status == wfo.INVALID_ARG


def premises(cs):
    """the premises of one case, on the references alone; returns the measured shares"""
    out = []
    for c, kind, fill in arms.subcalls(cs):
        inp = wfo.inputs(c, kind, fill)
        what = '%s %s fill %d' % (arms.IDS[arms.CASES.index(cs)], kind, fill)
        if c.mode != LINSPACE:
            masked = float(np.mean([wfo.masked_share(c, a) for a in inp.absloc]))
            assert 0.15 <= masked <= 0.75, '%s: masked share %.2f' % (what, masked)
            out.append(('masked', masked))
        if kind == 'lattice':
            half = float(np.mean([wfo.half_share(a) for a in inp.absloc]))
            assert half >= 0.20, '%s: half-integer share %.2f' % (what, half)
        if not fill and kind != 'lattice' and c.dtype != 'i32' and c is cs.call:
            other = dataclasses.replace(c, method=LINEAR if c.method == NEAREST else NEAREST)
            differ = float(np.mean([(wfo.reference(other, inp.vol[0 if c.shared_vol else b], inp.absloc[b], fill,
                                                   None if inp.addend is None else inp.addend[b]) != inp.refs[b]).mean() for b in range(c.B)]))
            assert differ >= 0.5, '%s: linear and nearest differ on %.2f' % (what, differ)
            out.append(('differ', differ))
            if c.dtype in ('f16', 'bf16', 'f64') and c.method == LINEAR:
                inexact = float(np.mean([wfo.inexact_share(c, inp.vol[b], inp.absloc[b]) for b in range(c.B)]))
                # a smooth field in 1-D cannot have that share with Gaussian data: a clamped location (>= 15 %) and one put on an integer
                # (31 % of the others) return a volume value unchanged, which leaves 0.58 at most, and the 8-bit locations of bfloat16 make
                # more products exact.  The share reached there (0.497 at bfloat16) is reported; the incoherent field of the same id holds 0.5
                smooth_1d = kind == 'smooth' and c.D == 1
                assert smooth_1d or inexact >= 0.5, '%s: %.2f of the outputs need the final rounding' % (what, inexact)
                out.append((('inexact(1-D smooth)' if smooth_1d else 'inexact') + ' ' + c.dtype, inexact))
    return out


FAMILIES = ('interpn_generic', 'interpn_rows', 'interpn_tile', 'interpn_zrun_c32', 'interpn_lean_tile', 'interpn_lean', 'interpn_any_nd', 'interpn_any',
            'interpn_any_nearest_i32')


@pytest.mark.parametrize('family', FAMILIES)
def test_premises_hold_on_every_reference(family):
    seen = {}
    for cs in arms.CASES:
        if cs.want.startswith('NRT_') or FAMILY_OF.match(cs.want).group(1) != family:
            continue
        for k, v in premises(cs):
            lo, hi = seen.get(k, (v, v))
            seen[k] = (min(lo, v), max(hi, v))
    print('PREMISES %-24s %s' % (family, '  '.join('%s %.2f-%.2f' % (k, lo, hi) for k, (lo, hi) in sorted(seen.items()))))


def test_fields_and_reference():
    """the two new field kinds, and the reference against np_oracle.interpn where both apply"""
    rng = np.random.default_rng(0)
    vol, loc = wfo.make_field(rng, (9, 8, 7), (7, 6, 7), 3, 'lattice', SHIFT)
    assert set(np.unique(loc)) <= set(wfo.LATTICE.tolist()) | set((wfo.LATTICE + 1).tolist()) | set((wfo.LATTICE - 1).tolist()) | set((wfo.LATTICE + 2).tolist())
    vol, loc = wfo.make_field(rng, (9, 8, 7), (7, 6, 7), 3, 'incoherent', ABSOLUTE)
    assert loc.min() >= -1 and (loc.reshape(-1, 3).max(0) <= (9, 8, 7)).all() and loc.reshape(-1, 3).max(0)[0] > 8
    for mode in (ABSOLUTE, SHIFT, LINSPACE):
        for method in (LINEAR, NEAREST):
            c = Call('f32', (9, 8, 7), (7, 6, 7), 3, mode, method)
            inp = wfo.inputs(c, 'grid' if mode == LINSPACE else 'incoherent', True)
            for b in range(c.B):
                want = npo.interpn(inp.vol[b], inp.absloc[b], 'nearest' if method else 'linear', wfo.FILL_F)
                assert arms.bits_equal(inp.refs[b], want)
    # the storage round trip of bfloat16
    x = npo.round_bf16(rng.standard_normal(100).astype(F))
    assert arms.bits_equal((arms.storage(x, 'bf16').astype(np.uint32) << 16).view(F), x)
