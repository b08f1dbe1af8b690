"""
Every dispatch arm of the Dice and cross-entropy reductions (csrc/dice.hip, csrc/dice_reduce.h, csrc/cce.hip), each under an id that
names the kernel instance its call takes.  The instance is derived by oracle/dice_cce_oracle.py, a restatement of the host dispatch,
and every test asserts that the instance in its id is the one the plan gives for each of its shapes; a kernel trace of this file and
tools/arm_coverage.py --families dice / cce confirm it on the device (profiles/dispatch_arms/README.md).  The table of cases, their
inputs and their float64 references are in tests/dice_cce_cases.py; tests/test_dice_cce_oracle.py checks the table and the premises
below without a device.

The C ABI is called directly on guarded buffers (tests/arm_buffers.py): typed maps at an exact byte offset, a workspace of exactly
nrt_dice_workspace_bytes / nrt_wcce_workspace_bytes, outputs pre-filled with a byte pattern so that a result that was never written
is seen, guards checked after every call; a refused call must leave every output untouched.

Dice family, two runs per id on the same shapes:

  exact    soft sums of small integers (y_true 1 .. 3, y_pred 0 .. 2, so that the four extrema differ; -3 .. 3 for the squared
           difference; rows whose label sum is 0, 1, 2 or 4 for `normalize`, so every quotient is dyadic): every sum of absolute
           terms is below 2^24 units (asserted on the reference), so float32 adds them exactly in any order and `sums` must equal
           the reference BIT FOR BIT.  Hard counts are integers on any data: rows of two low values and a maximum whose label runs
           through [0, L), so that every label and lane wins somewhere, tied in over 30 % of the voxels at a second, higher label, a
           third of the ties and more between labels of different lanes; ties go to the lowest label.  Each map's two extrema sit
           in one voxel and label of the whole map.  `dice` must
           equal the float32 op sequence of the second stage on those sums, with laplace_smoothing 0 and 0.5 and a label whose
           denominator is 0.  The extrema are compared as values.
  random   uniform [0, 1) maps rounded to the storage type: |got - ref| <= (n + k) 2^-24 A element-wise (derived in the oracle's
           docstring); `dice` still bit for bit the op sequence on the sums the device returned.  Each id prints its worst
           err / bound in a BOUND line (profiles/dispatch_arms/dice_cce_bounds.txt is the record of one run).

Cross-entropy: the per-voxel output element-wise and loss_sum against the float64 reference within the bounds derived in the
oracle's docstring, and loss_sum against the float64 sum of the device's own per-voxel values within the accumulation term and the log2 G
shuffle additions that form a per-voxel value (a dropped voxel shows whatever the accuracy of the logarithm).

Shapes are the smallest at which each mechanism can go wrong; the maps repeat with a prime period of 1021 voxels, so that the
reference of the few multi-million-voxel cases (the 2048-block cap) costs one period.
"""

import math

import numpy as np
import pytest
import torch

import dice_cce_cases as cs
from arm_buffers import Bytes, Raw
from neurite_amd import _lib
from oracle import dice_cce_oracle as dco

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
OK = _lib.NRT_OK


def status(dev, name, *args):
    """the entry point on torch's current stream of `dev`, its status returned, not raised"""
    with torch.cuda.device(dev):
        return getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev))


def guards_ok(ws):
    """nothing outside the workspace was written (compared on the device: the workspaces run to 200 MB)"""
    g = ws.GUARD
    return bool((ws.whole[:g] == ws.MARK).all().item() and (ws.whole[g + ws.n:] == ws.MARK).all().item())


def upload(dev, raw, V, off=0):
    full = cs.tile(raw, V)
    return Raw(dev, full.nbytes, off, full)


def dice_ws(dev, V, L, B, short=0):
    nws = _lib.lib().nrt_dice_workspace_bytes(V, L, B)
    assert nws == dco.dice_workspace_bytes(L, B)
    return Bytes(dev, nws - short), nws - short


def inst_of(arm):
    return arm.split(' ')[0]


# ------------------------------------------------------------------------------------------------------------------------------
# Dice from probability maps
# ------------------------------------------------------------------------------------------------------------------------------

def launch_dice(dev, c, tb, pb, V, B, eps, expect=OK, short=0, normalize=None, batch=None, dtype=None, minmax=None):
    """one call of the case's entry point on fresh outputs: (sums or counts [B, 3, L], dice [B, L], minmax [4] or None); a refused
    call (expect != NRT_OK) must leave them untouched"""
    L = c.L
    ws, nws = dice_ws(dev, V, L, B, short)
    wide = Raw(dev, B * 3 * L * (4 if c.kind == 'soft' else 8))
    dice = Raw(dev, B * L * 4)
    want_mm = c.minmax if minmax is None else minmax
    mm = Raw(dev, 16) if want_mm else None
    dt = dco.DT[c.dtype] if dtype is None else dtype
    nb = B if batch is None else batch
    nz = c.normalize if normalize is None else normalize
    mp = mm.p if mm else None
    if c.entry == 'nrt_dice_soft':
        args = (tb.p, pb.p, dt, V, L, nb, nz, eps, wide.p, dice.p, mp, ws.p, nws)
    elif c.entry == 'nrt_dice_soft_f32':
        args = (tb.p, pb.p, V, L, nb, nz, eps, wide.p, dice.p, mp, ws.p, nws)
    elif c.entry == 'nrt_sqdiff_sums_f32':
        args = (tb.p, pb.p, V, L, nb, wide.p, dice.p, ws.p, nws)
    elif c.entry == 'nrt_dice_hard_prob':
        args = (tb.p, pb.p, dt, V, L, nb, eps, wide.p, dice.p, mp, ws.p, nws)
    elif c.entry == 'nrt_dice_hard_prob_minmax_f32':
        args = (tb.p, pb.p, V, L, nb, eps, wide.p, dice.p, mp, ws.p, nws)
    else:
        assert c.entry == 'nrt_dice_hard_prob_f32' and not want_mm
        args = (tb.p, pb.p, V, L, nb, eps, wide.p, dice.p, ws.p, nws)
    rc = status(dev, c.entry, *args)
    assert rc == expect, '%s: status %d, expected %d' % (c.id, rc, expect)
    assert guards_ok(ws), 'a write outside the workspace'
    if expect != OK:
        assert wide.untouched() and dice.untouched() and (mm is None or mm.untouched()), c.id + ': a refused call wrote an output'
        return None
    return (wide.get(F if c.kind == 'soft' else np.int64, (B, 3, L)), dice.get(F, (B, L)), mm.get(F) if mm else None)


def check_dice_case(dev, c):
    worst = 0.0
    for V, B in c.shapes:
        plan = cs.case_plan(c, V, B)
        assert plan['instance'] == inst_of(c.id), (c.id, V, B, plan)
        for kind in c.kinds:
            traw, praw, r = cs.build(c, V, B, kind)
            tb, pb = (Raw(dev, m.nbytes, c.off, m) for m in cs.whole_maps(c, traw, praw, r, V))
            what = '%s V%d B%d %s' % (c.id, V, B, kind)
            for eps in ((0.0, 0.5) if kind == 'exact' else (0.5,)):
                wide, dice, mm = launch_dice(dev, c, tb, pb, V, B, eps)
                if c.kind == 'hard':
                    dco.check_exact(wide, r['counts'], what + ' counts')
                elif kind == 'exact':
                    dco.assert_exact_soft(r, c.normalize)
                    dco.check_exact(wide, r['sums'], what + ' sums')
                else:
                    worst = max(worst, dco.check_bounded(wide, r['sums'], (r['n'] + r['k']) * dco.U * r['A'], what + ' sums'))
                deps = 0.0 if c.normalize == 2 else eps          # nrt_sqdiff_sums_f32 has no smoothing: its scratch output is the plain quotient
                dco.check_exact(dice, dco.dice_f32(wide, deps), what + ' dice, laplace_smoothing %g' % deps)
                if mm is not None and (kind == 'exact' or c.normalize == 0):
                    assert mm.tolist() == r['minmax'].astype(F).tolist(), (what, mm, r['minmax'])
    if 'random' in c.kinds:
        print('BOUND %-64s worst err / bound: sums %.3g' % (c.id, worst))


@pytest.mark.parametrize('c', cs.SOFT, ids=[c.id for c in cs.SOFT])
def test_soft(dev, c):
    """nrt_dice_soft / nrt_dice_soft_f32 / nrt_sqdiff_sums_f32: dice_soft_vec<G, NORMALIZE, ST> with all lanes real and with padded
    lanes, dice_soft_generic<NORMALIZE, ST>, then reduce_rows<float, double> and dice_soft_finalize at 3 L = 12 .. 768 columns and
    1 .. 2048 rows"""
    if 'cap' in c.id:
        assert cs.case_plan(c, *c.shapes[0])['nblk'] == 2048 and cs.case_plan(c, *c.shapes[0])['empty'] > 0
    check_dice_case(dev, c)


@pytest.mark.parametrize('c', cs.HARD, ids=[c.id for c in cs.HARD])
def test_hard_prob(dev, c):
    """nrt_dice_hard_prob / _f32: dice_hard_vec<G, MINMAX, ST>, every rung of dice_hard_prob_generic<ST>'s VP ladder,
    dice_hard_prob_direct<ST>; then reduce_rows<unsigned, long long>, dice_counts_reduce, minmax_rows, dice_from_counts"""
    if 'cap' in c.id:
        assert cs.case_plan(c, *c.shapes[0])['nblk'] == 2048 and cs.case_plan(c, *c.shapes[0])['empty'] > 0
    check_dice_case(dev, c)


@pytest.mark.parametrize('c', cs.LABEL, ids=[c.id for c in cs.LABEL])
def test_hard_label(dev, c):
    """nrt_dice_hard_label_i32, labels from -2 .. L + 2, bit for bit against np.bincount"""
    for V, B in c.shapes:
        assert dco.plan_hard_label(c.L, V, B, c.workspace)['instance'] == inst_of(c.id)
        t, p, ref = cs.build_labels(c, V, B)
        tb, pb = Raw(dev, t.nbytes, 0, t), Raw(dev, p.nbytes, 0, p)
        for eps in (0.0, 0.5):
            ws, nws = dice_ws(dev, V, c.L, B) if c.workspace else (None, 0)
            counts, dice = Raw(dev, B * 3 * c.L * 8), Raw(dev, B * c.L * 4)
            rc = status(dev, 'nrt_dice_hard_label_i32', tb.p, pb.p, V, c.L, B, eps, counts.p, dice.p, ws.p if ws else None, nws)
            assert rc == OK, '%s: status %d' % (c.id, rc)
            assert ws is None or guards_ok(ws)
            got = counts.get(np.int64, (B, 3, c.L))
            dco.check_exact(got, ref, '%s V%d B%d counts' % (c.id, V, B))
            dco.check_exact(dice.get(F, (B, c.L)), dco.dice_f32(got, eps), c.id + ' dice')


def test_hard_prob_generic_refuses_extrema(dev):
    """the generic hard kernels have no extrema: NRT_ERR_UNSUPPORTED, nothing written"""
    c = cs.Case('refused', 'hard', 5, 'f32', 0, True, 0, 'nrt_dice_hard_prob', ((40, 2),), ('exact',))
    assert cs.case_plan(c, 40, 2)['status'] == dco.ERR_UNSUPPORTED
    traw, praw, _ = cs.build(c, 40, 2, 'exact')
    launch_dice(dev, c, upload(dev, traw, 40), upload(dev, praw, 40), 40, 2, 0.0, expect=_lib.NRT_ERR_UNSUPPORTED)


@pytest.mark.parametrize('kind', ('soft', 'hard'))
def test_refused_calls(dev, kind):
    """a workspace one byte short: NRT_ERR_WORKSPACE; batch 65536 (and, soft, normalize = 3): NRT_ERR_INVALID_ARG; an unknown dtype:
    NRT_ERR_UNSUPPORTED -- every output untouched"""
    c = cs.Case('refused', kind, 8, 'f32', 0, True, 0, 'nrt_dice_soft' if kind == 'soft' else 'nrt_dice_hard_prob', ((40, 2),), ('exact',))
    traw, praw, _ = cs.build(c, 40, 2, 'exact')
    tb, pb = upload(dev, traw, 40), upload(dev, praw, 40)
    assert launch_dice(dev, c, tb, pb, 40, 2, 0.0) is not None
    launch_dice(dev, c, tb, pb, 40, 2, 0.0, expect=_lib.NRT_ERR_WORKSPACE, short=1)
    launch_dice(dev, c, tb, pb, 40, 2, 0.0, expect=_lib.NRT_ERR_INVALID_ARG, batch=65536)
    launch_dice(dev, c, tb, pb, 40, 2, 0.0, expect=_lib.NRT_ERR_UNSUPPORTED, dtype=7)
    if kind == 'soft':
        launch_dice(dev, c, tb, pb, 40, 2, 0.0, expect=_lib.NRT_ERR_INVALID_ARG, normalize=3)
        launch_dice(dev, c._replace(entry='nrt_dice_soft_f32'), tb, pb, 40, 2, 0.0, expect=_lib.NRT_ERR_INVALID_ARG, normalize=3)


def test_soft_refuses_4097_labels(dev):
    """dice_soft_generic's grid.z covers 4096 labels: one more is NRT_ERR_UNSUPPORTED (the workspace, 201 MB, is large enough)"""
    c = cs.Case('refused', 'soft', 4097, 'f32', 0, True, 0, 'nrt_dice_soft_f32', ((2, 1),), ('exact',))
    z = np.zeros((1, 2, 4097), F)
    launch_dice(dev, c, upload(dev, z, 2), upload(dev, z, 2), 2, 1, 0.0, expect=_lib.NRT_ERR_UNSUPPORTED)


# ------------------------------------------------------------------------------------------------------------------------------
# the second stage on its own
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L,B', cs.MEAN, ids=['dice_from_sums n%d' % (L * B) for L, B in cs.MEAN])
def test_dice_from_sums(dev, L, B):
    """nrt_dice_from_sums_f32 at n = L B = 1, 255, 256, 257, 1000: the float32 op sequence, bit for bit, zero denominators included"""
    rng = cs.rng_for('from_sums', L, B)
    sums = rng.random((B, 3, L)).astype(F)
    sums[:, :, ::3] = 0
    sb = Raw(dev, sums.nbytes, 0, sums)
    for eps in (0.0, 0.5):
        dice = Raw(dev, B * L * 4)
        assert status(dev, 'nrt_dice_from_sums_f32', sb.p, L, B, eps, dice.p) == OK
        dco.check_exact(dice.get(F, (B, L)), dco.dice_f32(sums, eps))


@pytest.mark.parametrize('L,B', cs.MEAN, ids=['dice_mean_pair n%d' % (L * B) for L, B in cs.MEAN])
def test_dice_mean(dev, L, B):
    """nrt_dice_mean_pair_f32 and nrt_dice_mean_f32 without weights, with shared [L] and per-batch [B, L] weights, on values whose
    float64 sum is exact: [sum, n] and [sum, n, float32(sum) / float32(n)] bit for bit"""
    dice, w_shared, w_batch = cs.build_mean(L, B)
    db = Raw(dev, dice.nbytes, 0, dice)
    for w, per_batch in ((None, 0), (w_shared, 0), (w_batch, 1)):
        wb = Raw(dev, w.nbytes, 0, w) if w is not None else None
        s, n = dco.mean_ref(dice, w)
        assert n == L * B and s * 1024 == round(s * 1024) and s * 1024 < 2 ** 53
        for entry, k in (('nrt_dice_mean_pair_f32', 2), ('nrt_dice_mean_f32', 3)):
            out = Raw(dev, 4 * k)
            assert status(dev, entry, db.p, wb.p if wb else None, L, B, per_batch, out.p) == OK
            want = [F(s), F(n)] + ([F(s) / F(n)] if k == 3 else [])
            dco.check_exact(out.get(F), np.array(want, F), '%s n%d' % (entry, n))


# ------------------------------------------------------------------------------------------------------------------------------
# weighted categorical cross-entropy
# ------------------------------------------------------------------------------------------------------------------------------

def launch_cce(dev, c, tb, pb, wb, n, smooth, pv, ws=None, divide_by=None, loss=None):
    """nrt_wcce (or nrt_wcce_mean) on fresh outputs: (loss buffer, per-voxel buffer or None); the results are read by the caller"""
    lib = _lib.lib()
    assert lib.nrt_wcce_workspace_bytes(n, c.C) == dco.WCCE_WORKSPACE_BYTES
    ws = ws or Bytes(dev, dco.WCCE_WORKSPACE_BYTES)
    loss = loss or Raw(dev, 4)
    per = Raw(dev, 4 * n) if pv else None
    head = (tb.p, pb.p, dco.DT[c.dtype], wb.p if wb else None, n, c.C, int(c.logits), smooth)
    tail = (loss.p, per.p if per else None, ws.p, dco.WCCE_WORKSPACE_BYTES)
    rc = status(dev, 'nrt_wcce', *head, *tail) if divide_by is None else status(dev, 'nrt_wcce_mean', *head, float(divide_by), *tail)
    assert rc == OK, '%s: status %d' % (c.id, rc)
    return loss, per, ws


def check_cce(c, plan, ref, n, loss, per, what):
    """the three checks of the module docstring: (worst per-voxel ratio, worst sum ratio)"""
    l, bound, A = (cs.tiled_prefix(ref[k], n) for k in ('l', 'bound', 'A'))
    acc = (plan['iters'] + 10) * dco.U
    wv = 0.0
    if per is not None:
        wv = dco.check_bounded(per, l, bound, what + ' per_voxel')
        own = acc + math.log2(plan['G']) * dco.U
        dco.check_bounded([loss], [per.astype(D).sum()], [own * np.abs(per.astype(D)).sum()], what + ' loss_sum against its own per-voxel values')
    ws = dco.check_bounded([loss], [l.sum()], [bound.sum() + acc * A.sum()], what + ' loss_sum')
    return wv, ws


@pytest.mark.parametrize('c', cs.CCE, ids=[c.id for c in cs.CCE])
def test_wcce(dev, c):
    """nrt_wcce: all 56 wcce_vec<G, T, LOGITS, PERVOX> and the VP ladder of wcce_generic<T, LOGITS>, each with and without label weights
    and label smoothing, at sizes that put the ticket of wcce_finish on grids of 1, 2, 7, 8, 9 and 17 blocks"""
    traw, praw, w, refs = cs.build_cce(c)
    nmax = max(c.sizes)
    tb, pb = Raw(dev, nmax * c.C * dco.BYTES[c.dtype], c.off, cs.tile(traw, nmax)), Raw(dev, nmax * c.C * dco.BYTES[c.dtype], c.off, cs.tile(praw, nmax))
    wb = Raw(dev, w.nbytes, 0, w)
    worst_v = worst_s = 0.0
    for n in c.sizes:
        for pv in ((c.per_voxel,) if 'wcce_vec' in c.id else (False, True)):
            plan = dco.plan_cce(c.C, n, c.dtype, c.logits, pv, c.off)
            assert plan['instance'] == inst_of(c.id), (c.id, n, plan)
            if 'cap' in c.id:
                assert plan['nblk'] == 2048 and plan['empty'] > 0
            for hw, smooth in cs.COMBOS:
                loss, per, ws = launch_cce(dev, c, tb, pb, wb if hw else None, n, smooth, pv)
                ws.check()
                wv, wsum = check_cce(c, plan, refs[hw, smooth], n, loss.get(F)[0], per.get(F) if per else None,
                                     '%s n%d weights %d smoothing %g' % (c.id, n, hw, smooth))
                worst_v, worst_s = max(worst_v, wv), max(worst_s, wsum)
    print('BOUND %-64s worst err / bound: per_voxel %.3g loss_sum %.3g' % (c.id, worst_v, worst_s))


def test_wcce_ticket_back_to_back(dev):
    """id wcce_vec<1,float,false,false> C4 ticket: grids of 2048, 1, 9, 8, 7 and 2048 blocks launched back to back on one stream and one
    workspace, loss_sum pre-filled with NaN: every result is right, so every launch found the counters of wcce_finish clean; and
    nrt_wcce_mean with divide_by = n is float32(sum) / float32(n) of the nrt_wcce result, bit for bit"""
    C, u = cs.TICKET_C, cs.vec_unit(cs.TICKET_C)
    c = cs.CceCase('wcce_vec<1,float,false,false> C4 ticket', C, 'f32', False, False, 0, tuple(g * u for g in cs.TICKET_GRIDS))
    traw, praw, w, refs = cs.build_cce(c)
    nmax = max(c.sizes)
    tb, pb, wb = Raw(dev, nmax * C * 4, 0, cs.tile(traw, nmax)), Raw(dev, nmax * C * 4, 0, cs.tile(praw, nmax)), Raw(dev, w.nbytes, 0, w)
    ws = Bytes(dev, dco.WCCE_WORKSPACE_BYTES)
    nan = np.full(1, np.nan, F)
    plans, losses, means = [], [], []
    for g, n in zip(cs.TICKET_GRIDS, c.sizes):
        plans.append(dco.plan_cce(C, n, 'f32'))
        assert plans[-1]['nblk'] == g and plans[-1]['instance'] == inst_of(c.id)
        losses.append(launch_cce(dev, c, tb, pb, wb, n, 0.2, False, ws=ws, loss=Raw(dev, 4, 0, nan))[0])
    for n in c.sizes:
        means.append(launch_cce(dev, c, tb, pb, wb, n, 0.2, False, ws=ws, divide_by=n, loss=Raw(dev, 4, 0, nan))[0])
    ws.check()
    for plan, n, loss, mean in zip(plans, c.sizes, losses, means):
        s = loss.get(F)[0]
        check_cce(c, plan, refs[True, 0.2], n, s, None, '%s grid %d' % (c.id, plan['nblk']))
        dco.check_exact(mean.get(F), np.array([s / F(n)], F), 'nrt_wcce_mean grid %d' % plan['nblk'])


def test_wcce_refused_calls(dev):
    """a workspace one byte short: NRT_ERR_WORKSPACE; float16 maps: NRT_ERR_UNSUPPORTED; divide_by = 0: NRT_ERR_INVALID_ARG"""
    z = np.full((8, 4), 0.25, F)
    tb, pb = Raw(dev, z.nbytes, 0, z), Raw(dev, z.nbytes, 0, z)
    nws = dco.WCCE_WORKSPACE_BYTES
    for dt, short, div, want in ((0, 1, 1.0, _lib.NRT_ERR_WORKSPACE), (2, 0, 1.0, _lib.NRT_ERR_UNSUPPORTED), (0, 0, 0.0, _lib.NRT_ERR_INVALID_ARG)):
        ws, loss, per = Bytes(dev, nws - short), Raw(dev, 4), Raw(dev, 32)
        assert status(dev, 'nrt_wcce_mean', tb.p, pb.p, dt, None, 8, 4, 0, 0.0, div, loss.p, per.p, ws.p, nws - short) == want
        ws.check()
        assert loss.untouched() and per.untouched()
