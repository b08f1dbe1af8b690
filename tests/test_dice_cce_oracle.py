"""
CPU tests of oracle/dice_cce_oracle.py and tests/dice_cce_cases.py (the restated dispatch, the references and the case table behind
tests/test_gpu_dice_cce_arms.py) -- the part of "every arm has an id" that needs no GPU: every instance of the Dice and cross-entropy
families in the committed kernel tables (profiles/dispatch_arms/dice_kernels.txt, cce_kernels.txt) is named by an id, or is a
second-stage kernel that the ids of an entry point launch behind their first stage; every id is what the plans derive for each of
its shapes; the premises of the exact runs hold on the reference of every case; and the restated nrt_block_range tiles [0, n)
exactly once for every (n, grid, unit) of the table.
"""

import os
import re
import sys

import numpy as np
import pytest

from oracle import dice_cce_oracle as dco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402
import dice_cce_cases as cs                                                               # noqa: E402

F, D = np.float32, np.float64

# the kernels behind the first stage: which cases launch them (dice_reduce.h: dice_finalize_soft; dice.hip: the tails of
# dice_hard_prob_impl and nrt_dice_hard_label_i32, the three entry points of the second stage)
SECOND_STAGE = {
    'reduce_rows<float,double>': 'every soft id', 'dice_soft_finalize': 'every soft id',
    'reduce_rows<unsignedint,longlong>': 'every dice_hard_vec id and the label ids with a workspace',
    'dice_counts_reduce': 'every dice_hard_vec id and the label ids with a workspace',
    'minmax_rows': 'the dice_hard_vec<G,true,ST> ids', 'dice_from_counts': 'every hard id',
    'dice_from_sums': 'test_dice_from_sums', 'dice_mean_pair': 'test_dice_mean',
}


def table_instances(table, family):
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS[family]))
    found = set()
    for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', table)):
        m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
        if m and fam.match(arm_coverage.norm(m.group(1))):
            found.add(arm_coverage.norm(m.group(1)))
    return found


def named(cases):
    return {c.id.split(' ')[0] for c in cases}


def test_ids_name_every_emitted_instance():
    dice, cce = table_instances('dice_kernels.txt', 'dice'), table_instances('cce_kernels.txt', 'cce')
    assert len(dice) == 107 and len(cce) == 60
    ids = [c.id for c in cs.SOFT + cs.HARD + cs.LABEL + cs.CCE]
    assert len(set(ids)) == len(ids)
    by_id = named(cs.SOFT) | named(cs.HARD) | named(cs.LABEL)
    assert by_id | set(SECOND_STAGE) == dice and not by_id & set(SECOND_STAGE)
    assert named(cs.CCE) == cce
    assert sum(k.startswith('wcce_vec') for k in cce) == 56
    assert not arm_coverage.UNREACHABLE['dice'] and not arm_coverage.UNREACHABLE['cce']


def test_every_id_is_what_the_plan_derives():
    for c in cs.SOFT + cs.HARD:
        for V, B in c.shapes:
            p = cs.case_plan(c, V, B)
            assert p['instance'] == c.id.split(' ')[0], (c.id, V, B, p)
            if 'cap' in c.id:
                assert p['nblk'] == 2048 and p['empty'] > 0.15 * 2048, (c.id, p)
            elif '_vec' in c.id:
                assert p['nblk'] < 2048 and p['Gr'] <= p['G'] < 2 * p['Gr'] or p['G'] == 1
            if 'VP' in c.id:
                assert 'VP%d' % p['VP'] in c.id
    for c in cs.LABEL:
        for V, B in c.shapes:
            assert dco.plan_hard_label(c.L, V, B, c.workspace)['instance'] == c.id.split(' ')[0]
    for c in cs.CCE:
        for n in c.sizes:
            p = dco.plan_cce(c.C, n, c.dtype, c.logits, c.per_voxel, c.off)
            assert p['instance'] == c.id.split(' ')[0], (c.id, n, p)
            if 'cap' in c.id:
                assert p['nblk'] == 2048 and p['empty'] > 0.15 * 2048
            if 'VP' in c.id:
                assert 'VP%d' % p['VP'] in c.id


def test_shapes_reach_the_mechanisms_they_are_chosen_for():
    """the grids of the vector ids: 1, 2, 63, 64, 65 and 513 blocks (1, 1, 1, 1, 2 and 9 row groups); every G with all lanes real and,
    from G = 4 on, with padded lanes; 3 L = 12, 396 and 768 columns; the ladders' edges; the label kernels' thresholds"""
    for L in cs.VEC_L:
        p = [dco.plan_soft(L, V, B, 0) for V, B in cs.vec_shapes(L)]
        assert [q['nblk'] for q in p[::2]] == [1, 1, 2, 63, 64, 65, 513] and [q['ngrp'] for q in p[::2]] == [1, 1, 1, 1, 1, 2, 9]
    groups = {(dco.vec_group(L), L // 4) for L in cs.VEC_L}
    assert {g for g, gr in groups if g == gr} == {1, 2, 4, 8, 16, 32, 64} and {g for g, gr in groups if gr < g} == {4, 8, 16, 32, 64}
    assert {3 * 4, 3 * 132, 3 * 256} <= {3 * L for L in cs.VEC_L}
    # generic soft kernel: L = 100 -> two voxel rows and 56 idle threads; 257 -> gz 2, the last chunk one label; 600 -> gz 3; 4096 -> gz 16
    assert dco.plan_soft(100, 10, 1, 0, 'f32', 4)['R'] == 2 and dco.plan_soft(257, 10, 1, 0)['gz'] == 2 and dco.plan_soft(600, 10, 1, 0)['gz'] == 3
    assert dco.plan_soft(4096, 5, 1, 0)['gz'] == 16 and 195e6 < dco.dice_workspace_bytes(4096, 1) < 205e6
    for L in (1, 3, 5, 100, 255, 257, 600):                     # the last shape takes a second grid-stride pass
        V, B = cs.generic_soft_shapes(L)[-1]
        p = dco.plan_soft(L, V, B, 0, 'f32', 4 if L == 100 else 0)
        assert p['nblk'] == 2048 // p['gz'] and V > p['nblk'] * p['R']
    # hard ladder: the widest row of every rung, and one label more takes the next rung (1117 + 1: the direct kernel)
    rungs = dco.hard_prob_rungs()
    assert rungs == {256: 47, 128: 93, 64: 183, 32: 351, 16: 646, 8: 1117}
    for VP, L in rungs.items():
        assert dco.hard_prob_vp(L) == VP and dco.hard_prob_vp(L + 1) == (VP // 2 if VP > 8 else 0)
        assert (VP * L + 3 * L) * 4 <= 48 * 1024 < (VP * (L + 1) + 3 * (L + 1)) * 4
    assert dco.plan_hard_prob(1118, 5, 1, False)['instance'] == 'dice_hard_prob_direct<float>'
    assert any(dco.plan_hard_prob(c.L, V, B, False, c.dtype)['passes'] == 2 for c in cs.HARD if 'VP8' in c.id for V, B in c.shapes)
    # cross-entropy ladder
    assert [dco.cce_vp(C) for C in (1, 2, 3, 24, 25, 49, 97, 193, 385, 768, 769)] == [256, 256, 256, 256, 128, 64, 32, 16, 8, 8, 0]
    assert dco.plan_cce(385, 2048 * 8 + 9, 'f32', False, True)['iters'] == 2
    for C in cs.VEC_L:
        assert [dco.plan_cce(C, n)['nblk'] for n in cs.cce_vec_sizes(C)] == [1, 1, 2, 7, 8, 9, 17]
    # label maps
    assert dco.plan_hard_label(40, 65536, 1)['instance'] == 'dice_hard_label_private' != dco.plan_hard_label(41, 65536, 1)['instance']
    assert dco.plan_hard_label(40, 65535, 1)['instance'] == 'dice_hard_label<true>'
    assert dco.plan_hard_label(5461, 100, 1, False)['use_lds'] and not dco.plan_hard_label(5462, 100, 1, False)['use_lds']
    assert dco.plan_hard_label(41, 512 * 2048 + 2049, 1)['nblk'] == 512 < dco.num_blocks(512 * 2048 + 2049, 2048)
    p = dco.plan_hard_label(8, 700324, 3)                       # the four-in-flight loop runs, then the one-quad loop, then the tail
    assert p['nblk'] == 170 and 3 * 170 * 256 < 700324 // 4 < 4 * 170 * 256 + 170 * 256


def test_block_range_tiles_the_voxels_once():
    seen = set()
    for c in cs.SOFT + cs.HARD:
        for V, B in c.shapes:
            p = cs.case_plan(c, V, B)
            if p.get('NG'):
                seen.add((V, p['nblk'], p['NG']))
    for c in cs.CCE:
        for n in c.sizes:
            p = dco.plan_cce(c.C, n, c.dtype, c.logits, c.per_voxel, c.off)
            if p.get('NG'):
                seen.add((n, p['nblk'], p['NG']))
    assert len(seen) > 80
    for n, grid, unit in sorted(seen):
        empty = dco.range_cover(n, grid, unit)
        per, beg, end = dco.block_range(n, grid, unit)
        assert int((end - beg).sum()) == n and empty == grid - dco.cdiv(n, per)
    for n in (0, 1, 5, 1000, 12345):                            # and a sweep of small grids
        for grid in (1, 2, 3, 7, 64):
            for unit in (1, 4, 256):
                dco.range_cover(n, grid, unit)


@pytest.mark.parametrize('c', cs.SOFT, ids=[c.id for c in cs.SOFT])
def test_soft_premises(c):
    """exact run: the storage type holds the draw, every term is an integer (a multiple of 2^-4 with normalize) and every sum of absolute
    terms is below 2^24 units; with normalize every label sum is 0, 1, 2 or 4 and a share of the rows is all zero; the one-block shape
    has a label whose denominator is 0"""
    for V, B in c.shapes:
        traw, praw, r = cs.build(c, V, B, 'exact')
        dco.assert_exact_soft(r, c.normalize)
        if c.normalize == 1:
            rng = cs.rng_for(c.id, V, B, 'exact')
            tt, pp = dco.draw_soft(rng, B, V, c.L, 'exact', 1, cs.zero_label(c, V))
            for m in (tt, pp):
                s = m.sum(-1)
                assert np.isin(s, (0, 1, 2, 4)).all() and (m >= 0).all()
                assert s.size < 500 or ((s == 0).mean() > 0.1 and (s == 4).mean() > 0.1)
        z = cs.zero_label(c, V)
        if z is not None:
            assert (r['sums'][:, 1:, z] == 0).all()
            assert (dco.dice_f32(r['sums'], 0.0)[:, z] == 0).all() and (dco.dice_f32(r['sums'], 0.5)[:, z] == 1).all()
    assert c.normalize == 2 or c.L == 1 or len(c.shapes) == 1 or any(cs.zero_label(c, V) is not None for V, B in c.shapes)


@pytest.mark.parametrize('c', cs.HARD, ids=[c.id for c in cs.HARD])
def test_hard_premises(c):
    """pooled over the rows of all shapes of a case (a shape of one voxel has no share of its own): at least 30 % of the rows have a
    tied maximum -- but for L = 1, where nothing can tie -- and, on the vector kernels with more than one lane per voxel (G >= 2), at
    least a third of those ties lie between labels of different lanes (the generic kernels scan a row in one thread: no lanes).
    The winner is spread over [0, L): on the vector kernels every label of both maps wins in some voxel, so every lane up to Gr - 1
    decides an arg-max, counts and fills its LDS slots; on the row scans (up to 2000 labels) every eighth of the label range holds
    winners and one lies in the last sixteenth.  Each map's extrema are spikes in one voxel and label, kept out of every arg-max"""
    rows = tied = cross = 0
    wins = np.zeros((2, c.L), np.int64)
    for V, B in c.shapes:
        _, _, r = cs.build(c, V, B, 'exact')
        rows, tied, cross, wins = rows + r['rows'], tied + r['tied'], cross + r['cross'], wins + r['wins']
        assert (r['counts'][:, 1:].sum(-1) == V).all()
        if c.L > 1:
            lo0, lo1, top, smin, smax = zip(*dco.HARD_VALUES)
            assert r['minmax'].tolist() == [smin[0], smax[0], smin[1], smax[1]]
    assert c.L == 1 or tied >= 0.3 * rows, (c.id, tied, rows)
    if '_vec<' in c.id:
        G = dco.vec_group(c.L)
        assert G == 1 or cross >= tied / 3, (c.id, cross, tied)
        assert (wins > 0).all(), (c.id, np.argwhere(wins == 0).tolist())
    elif c.L >= 16:
        eighths = np.add.reduceat(wins, np.arange(0, c.L, -(-c.L // 8)), axis=1)
        assert (eighths > 0).all() and (wins[:, c.L - c.L // 16:].sum(1) > 0).all(), (c.id, eighths)


def test_references_on_a_case_worked_by_hand():
    t = np.array([[[1, 0, 2], [0, 3, 3]]], F)
    p = np.array([[[1, 1, 0], [2, 2, 1]]], F)
    r = dco.soft_ref(t, p, 2, 0)
    assert r['sums'].tolist() == [[[1, 6, 3], [1, 9, 13], [5, 5, 1]]]
    assert dco.dice_f32(r['sums'], 0.0).tolist() == [[F(2) / F(6), F(12) / F(14), F(6) / F(14)]]
    rn = dco.soft_ref(t, p, 2, 1)
    assert np.allclose(rn['sums'][0, 0], [1 / 3 * 1 / 2 + 0, 0.5 * 0.4, 0.5 * 0.2])
    assert dco.soft_ref(t, p, 2, 2)['sums'][0].tolist() == [[4, 2, 8]] * 3
    h = dco.hard_ref(t, p, 2)                                    # arg-max: t -> 2, 1 (tie: the lowest); p -> 0 (tie), 0 (tie)
    assert h['counts'].tolist() == [[[0, 0, 0], [0, 1, 1], [2, 0, 0]]] and (h['tied'], h['rows']) == (3, 4)
    lab = dco.label_ref(np.array([[0, 1, 5, -1, 2]]), np.array([[0, 2, 5, -1, 2]]), 3)
    assert lab.tolist() == [[[1, 0, 1], [1, 1, 1], [1, 0, 2]]]
    # tiling: 2500 voxels of a 1021-voxel period
    rng = np.random.default_rng(1)
    base = rng.integers(0, 4, (2, 1021, 5)).astype(D)
    full = dco.Tiled(base, 2500).full()
    assert full.shape == (2, 2500, 5) and np.array_equal(dco.tiled_sum(base, 2500), full.sum(1))
    # cross-entropy against a plain loop
    tt, pp, w = rng.random((4, 3)), rng.random((4, 3)), np.array([0.5, 1.0, 1.5], F)
    pp[0, 1] = 0
    r = dco.cce_ref(tt, pp, w, 0.2, False)
    for v in range(4):
        q = np.clip(pp[v] / pp[v].sum(), float(F(1e-7)), float(F(1) - F(1e-7)))
        T = tt[v] * w * float(F(1) - F(0.2)) + float(F(0.2) / F(3))
        assert abs(r['l'][v] + (T * np.log(q)).sum()) < 1e-12 and r['bound'][v] > 0
    r = dco.cce_ref(tt, pp * 5, None, 0.0, True)
    for v in range(4):
        x = pp[v] * 5
        assert abs(r['l'][v] + (tt[v] * (x - np.log(np.exp(x).sum()))).sum()) < 1e-12
    bits, wide = dco.store(np.array([1.0, 1.00390625, 1.01171875, 0.1], F), 'bf16')         # ties to even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert wide[:3].tolist() == [1.0, 1.0, 1.015625] and bits[0] == 0x3F80 and abs(wide[3] - 0.1) < 2 ** -11
