"""
The host dispatch of the Dice and cross-entropy reductions (csrc/dice.hip, csrc/dice_reduce.h, csrc/cce.hip), restated, and float64
references of what they compute, for tests/test_gpu_dice_cce_arms.py and tests/test_dice_cce_oracle.py.  numpy only.

Plans.  plan_soft / plan_hard_prob / plan_hard_label / plan_cce return the kernel instance a call takes (named as the kernel tables
of tools/kernel_digest.py name it, blanks removed), the grid (`nblk`, `gz`), the voxels per LDS pass `VP` of the staged generic
kernels, the number of row groups `ngrp` of the second stage and, for the kernels that walk nrt_block_range, the voxels a block
gets (`per`) and the number of blocks whose range is empty (`empty`).

References.  Written from neurite/tf/metrics.py, not from the kernels:
  soft Dice   :434-436 optional y / sum_l y with divide_no_nan; :476-477 sum t p, sum t^2, sum p^2 over the voxels
  hard Dice   :463-468 arg-max over the labels (the first of tied maxima, as tf.argmax and np.argmax), one-hot, then the same
              sums, which are counts; integer label maps go to one_hot directly, an id outside [0, L) is an all-zero row
  dice        :476-482 2 top / bottom, with laplace smoothing (top + eps) / (bottom + eps), else divide_no_nan
  mean        :499-510 K.mean(dice * weights)
  wcce        :640-650 y_true * label_weights, then tf.keras.losses.CategoricalCrossentropy: label smoothing
              t (1 - s) + s / C, p / sum_c p clipped to [1e-7, 1 - 1e-7] or log-soft-max of logits, - sum_c t log p

Maps are periodic in the voxel index with a prime period (`Tiled`), so that a reference over millions of voxels costs one period:
a sum over V voxels is (V // P) sums of a period plus a prefix.

Bounds (u = 2^-24, first order in u; the neglected terms are below n u times the bound, and the kernels' sums are trees that use a
small part of it).

  soft sums.  An element is a sum of n = V terms.  Each term carries k roundings before it is added, the float32 sum of n terms
  carries at most n - 1 in any order, the float64 second stage none that matters and its conversion to float32 one:
      |got - ref| <= (n + k) u A,   A = the sum of the absolute terms.
  k = 1 for t p, t t and p p of stored values (the product).  With `normalize` the label sum of L non-negative values carries at
  most L - 1 roundings and the quotient one, so each factor is off by at most L u relative, the two factors of a term by 2 L u, and
  the product adds one: k = 2 L + 1.  For the squared difference (nrt_sqdiff_sums_f32) d = t - p rounds once, relative to d, which
  is 2 u in d d, and the product adds one: k = 3.  (soft_k)

  weighted cross-entropy, per voxel (cce_ref).  T_c = w_c t_c, smoothed, carries at most 3 roundings (the weight, `keep`, `add`):
  3 u T_c.  The product with the log adds one and the sum over the C channels of a voxel at most C - 1.
    probabilities: s = sum_c p_c within (C - 1) u relative, q = p / s within C u, the clip is 1-Lipschitz, so log q moves by at most
      C u; logf itself is within one ulp (2 u |log q|, the accuracy the device library documents).  Together
          bound_v = u sum_c T_c (C + (C + 6) |log q_c|).
    logits: d_c = x_c - max within u |d_c|; exp(d_c) then within (2 + 2 |d_c|) u relative (cce.hip states 2^-23 + |d| 2^-24 for
      lse_exp, expf is within one ulp; the other |d_c| u is the argument); the sum se within (C - 1) u + E u with E the
      e-weighted mean of 2 + 2 |d_c|; lse = log se moves by that and the function adds 2^-22 = 4 u absolute (lse_log on [1, C],
      as cce.hip states) or one ulp (logf: 2 u lse); the last subtraction rounds once.  So
          dlq_c = u (|d_c| + C - 1 + E + 4 + 2 lse + |lq_c|),   bound_v = sum_c T_c dlq_c + (C + 4) u T_c |lq_c|.
  The reference clips with the kernel's float32 constants (float32(1e-7), float32(1) - float32(1e-7)) and smooths with its float32
  `keep` and `add`.
  loss_sum is held to the float64 sum of the reference values within sum_v bound_v + (iters + 10) u sum_v A_v: a lane adds `iters`
  terms, the wave six shuffles, the block three adds and the result is converted once (A_v = sum_c T_c |log q_c| = |l_v| for
  non-negative weights).  Against the float64 sum of the device's own per-voxel values the margin is (iters + 10 + log2 G) u
  sum_v |l_v| alone: the per-voxel value is the lane-group's shuffle sum of the lane terms, log2 G more additions.
"""

import numpy as np

F, D = np.float32, np.float64
U = 2.0 ** -24
BLOCK, MAX_BLOCKS, RED_ROWS = 256, 2048, 64
PERIOD = 1021
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
DT = {'f32': 0, 'bf16': 1, 'f16': 2}
BYTES = {'f32': 4, 'bf16': 2, 'f16': 2}
DICE_ST = {'f32': 'float', 'bf16': 'DiceBf16', 'f16': '_Float16'}
CCE_T = {'f32': 'float', 'bf16': 'unsignedshort'}


def _b(v):
    return 'true' if v else 'false'


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# storage types
# ------------------------------------------------------------------------------------------------------------------------------

def store(x, dtype):
    """x rounded to the storage type (round to nearest even): (the array to upload, its values as float64)"""
    x = np.ascontiguousarray(x, F)
    if dtype == 'f32':
        return x, x.astype(D)
    if dtype == 'f16':
        h = x.astype(np.float16)
        return h, h.astype(D)
    bits = x.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    return bits, (bits.astype(np.uint32) << 16).view(F).astype(D)


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------

def num_blocks(n, per_pass):
    """dice_num_blocks"""
    return max(1, min(MAX_BLOCKS, cdiv(n, per_pass)))


def block_range(n, grid, unit):
    """nrt_block_range for every block of the grid: (per, beg [grid], end [grid])"""
    per = cdiv(n, grid * unit) * unit
    beg = np.minimum(np.arange(grid, dtype=np.int64) * per, n)
    return per, beg, np.minimum(beg + per, n)


def range_cover(n, grid, unit):
    """asserts that the ranges tile [0, n) exactly once, in order; the number of blocks with an empty range"""
    per, beg, end = block_range(n, grid, unit)
    assert beg[0] == 0 and end[-1] == n and (beg[1:] == end[:-1]).all() and (end >= beg).all(), (n, grid, unit)
    assert per % unit == 0
    return int((end == beg).sum())


def vec_labels(L):
    return L % 4 == 0 and 4 <= L <= 256


def vec_group(L):
    g = 1
    while g < L // 4:
        g <<= 1
    return g


def _vec_plan(name, L, V):
    G = vec_group(L)
    NG = BLOCK // G
    nblk = num_blocks(V, NG * 4)
    per, _, _ = block_range(V, nblk, NG)
    return dict(instance=name % G, nblk=nblk, gz=1, VP=None, ngrp=cdiv(nblk, RED_ROWS), G=G, Gr=L // 4, NG=NG, per=per,
                empty=range_cover(V, nblk, NG))


def plan_soft(L, V, B, normalize, dtype='f32', off=0):
    """dice_soft_impl.  normalize: 0, 1, or 2 = nrt_sqdiff_sums_f32; off: the byte offset of both maps from a 16-byte boundary"""
    assert 1 <= L <= 4096 and 1 <= B <= 65535
    norm = _b(normalize == 1)
    if vec_labels(L) and off % (4 * BYTES[dtype]) == 0:
        return _vec_plan('dice_soft_vec<%%d,%s,%s>' % (norm, DICE_ST[dtype]), L, V)
    Lc = min(L, BLOCK)
    gz = cdiv(L, BLOCK)
    nblk = min(num_blocks(V, BLOCK // Lc), MAX_BLOCKS // gz)
    return dict(instance='dice_soft_generic<%s,%s>' % (norm, DICE_ST[dtype]), nblk=nblk, gz=gz, VP=None, ngrp=cdiv(nblk, RED_ROWS),
                R=BLOCK // Lc, per=None, empty=None)


def hard_prob_vp(L):
    """the VP ladder of dice_hard_prob_impl: voxels per LDS pass, 0 = rows too wide for 48 KB (dice_hard_prob_direct)"""
    VP = BLOCK
    while VP > 8 and (VP * L + 3 * L) * 4 > 48 * 1024:
        VP >>= 1
    return VP if (VP * L + 3 * L) * 4 <= 48 * 1024 else 0


def hard_prob_rungs():
    """{VP: the largest label count that still takes it}: (VP + 3) L 4 <= 49152, so L <= 12288 // (VP + 3)"""
    return {VP: 12288 // (VP + 3) for VP in (256, 128, 64, 32, 16, 8)}


def plan_hard_prob(L, V, B, minmax, dtype='f32', off=0):
    """dice_hard_prob_impl; status = NRT_ERR_UNSUPPORTED where the generic kernels are asked for extrema"""
    if vec_labels(L) and off % (4 * BYTES[dtype]) == 0:
        return _vec_plan('dice_hard_vec<%%d,%s,%s>' % (_b(minmax), DICE_ST[dtype]), L, V)
    if minmax:
        return dict(instance=None, status=ERR_UNSUPPORTED)
    VP = hard_prob_vp(L)
    if VP:
        return dict(instance='dice_hard_prob_generic<%s>' % DICE_ST[dtype], nblk=max(1, min(1024, cdiv(V, VP))), gz=1, VP=VP, ngrp=None,
                    per=None, empty=None, passes=cdiv(V, VP * max(1, min(1024, cdiv(V, VP)))))
    return dict(instance='dice_hard_prob_direct<%s>' % DICE_ST[dtype], nblk=num_blocks(V, BLOCK), gz=1, VP=0, ngrp=None, per=None, empty=None)


def plan_hard_label(L, V, B, workspace=True):
    """nrt_dice_hard_label_i32"""
    use_lds = 3 * L * 4 <= 64 * 1024
    nblk = num_blocks(V, BLOCK * 8)
    if use_lds and workspace:
        nblk = min(nblk, 512)
        if 3 * L * BLOCK * 4 <= 120 * 1024 and V >= 65536:
            nblk = min(nblk, max(1, 512 // B))
            inst = 'dice_hard_label_private'
        else:
            inst = 'dice_hard_label<true>'
        return dict(instance=inst, nblk=nblk, gz=1, VP=None, ngrp=cdiv(nblk, RED_ROWS), use_lds=True, per=None, empty=None)
    return dict(instance='dice_hard_label<false>', nblk=nblk, gz=1, VP=None, ngrp=None, use_lds=use_lds, per=None, empty=None)


def cce_vp(C):
    """the VP ladder of launch_any (cce.hip): both tensors' rows of VP voxels in 48 KB, 0 beyond 768 channels"""
    VP = BLOCK
    while VP > 8 and 2 * VP * C * 4 > 48 * 1024:
        VP >>= 1
    return VP if 2 * VP * C * 4 <= 48 * 1024 else 0


def plan_cce(C, n, dtype='f32', logits=False, per_voxel=False, off=0):
    """wcce_impl / launch_any.  iters: the terms a lane adds before the wave reduction"""
    if vec_labels(C) and off % 16 == 0:
        G = vec_group(C)
        NG = BLOCK // G
        nblk = max(1, min(MAX_BLOCKS, cdiv(n, NG * 4)))
        per, _, _ = block_range(n, nblk, NG)
        return dict(instance='wcce_vec<%d,%s,%s,%s>' % (G, CCE_T[dtype], _b(logits), _b(per_voxel)), nblk=nblk, gz=1, VP=None, ngrp=None,
                    G=G, Gr=C // 4, NG=NG, per=per, empty=range_cover(n, nblk, NG), iters=per // NG)
    VP = cce_vp(C)
    per = VP or BLOCK
    nblk = max(1, min(MAX_BLOCKS, cdiv(n, per)))
    return dict(instance='wcce_generic<%s,%s>' % (CCE_T[dtype], _b(logits)), nblk=nblk, gz=1, VP=VP, ngrp=None, G=1, per=None, empty=None,
                iters=cdiv(n, nblk * per))


def dice_workspace_bytes(L, B):
    """dice_ws_bytes"""
    per, grp = B * MAX_BLOCKS, B * cdiv(MAX_BLOCKS, 64)
    return per * 3 * L * 4 + per * 16 + per * 3 * L * 4 + grp * 3 * L * 8 + grp * 16 + 256


WCCE_WORKSPACE_BYTES = MAX_BLOCKS * 4 + 256


# ------------------------------------------------------------------------------------------------------------------------------
# periodic maps
# ------------------------------------------------------------------------------------------------------------------------------

class Tiled:
    """a map [B, V, ...] that repeats its first P = min(V, PERIOD) voxels"""

    def __init__(self, base, V):
        self.base, self.V, self.P = base, V, base.shape[1]
        assert self.P == min(V, PERIOD)

    def full(self):
        reps = cdiv(self.V, self.P)
        return np.ascontiguousarray(np.concatenate([self.base] * reps, axis=1)[:, :self.V])


def tiled_sum(terms, V):
    """sum over V voxels of per-voxel float64 / int64 terms [B, P, ...] repeated with period P"""
    P = terms.shape[1]
    q, r = divmod(V, P)
    return q * terms.sum(axis=1) + terms[:, :r].sum(axis=1)


def period(V):
    return min(V, PERIOD)


# ------------------------------------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------------------------------------

def draw_soft(rng, B, V, L, kind, normalize, zero_label=None, small=False):
    """one period of both maps as float32.  kind 'exact': y_true from 1 .. 3 and y_pred from 0 .. 2 (1 .. 2 and 0 .. 1 if `small`), so
    the two minima and the two maxima differ; -3 .. 3 for the squared difference; rows of label sum 0, 1, 2 or 4 for `normalize`.
    kind 'random': uniform [0, 1).  zero_label: that label is 0 in both maps, so its denominator is 0"""
    P = period(V)
    if kind == 'random':
        t, p = rng.random((B, P, L)), rng.random((B, P, L))
    elif normalize == 2:
        t, p = rng.integers(-3, 4, (B, P, L)), rng.integers(-3, 4, (B, P, L))
    elif normalize == 1:
        Ld = L if zero_label is None else L - 1                 # the zero label stays out of the rows, so their sums stay 0, 1, 2 or 4
        t, p = (_dyadic_rows(rng, B * P, Ld).reshape(B, P, Ld) for _ in range(2))
        if zero_label is not None:
            t, p = (np.insert(m, zero_label, 0, axis=-1) for m in (t, p))
    else:
        hi = 2 if small else 3
        t, p = rng.integers(1, hi + 1, (B, P, L)), rng.integers(0, hi, (B, P, L))
    t, p = t.astype(F), p.astype(F)
    if zero_label is not None:
        t[..., zero_label] = 0
        p[..., zero_label] = 0
    return t, p


def _dyadic_rows(rng, N, L):
    """rows of non-negative integers whose sum is 0, 1, 2 or 4 (a fifth of them 0)"""
    s = rng.choice(np.array([0, 1, 2, 4]), size=N, p=[0.2, 0.3, 0.3, 0.2])
    rows = np.zeros((N, L), np.int64)
    for j in range(4):
        np.add.at(rows, (np.arange(N), rng.integers(0, L, N)), (j < s).astype(np.int64))
    return rows


HARD_VALUES = ((0.25, 0.5, 0.75, 0.0, 0.875), (0.125, 0.25, 0.5, 0.0625, 0.625))       # per map: two low values, the maximum, the two spikes


def _spread(rng, n, L):
    """n labels that run through [0, L) in a shuffled order: every label n / L times where n >= L, else one from each of n equal strata"""
    seq = np.arange(n) % L if n >= L else ((np.arange(n) + rng.random(n)) * L / max(n, 1)).astype(np.int64)
    return rng.permutation(seq)


def draw_hard(rng, B, V, L):
    """one period of both maps, multiples of 2^-4 (exact in all three storage types), and the spikes of the whole map.
    A row holds the map's two low values and its maximum at a label w that runs through [0, L) in a shuffled order, so that every label, lane
    and quad wins somewhere (a draw with the maximum on a share of ALL labels lets only the lowest few win: ties go to the lowest); in
    60 % of the rows the maximum is tied at a second label drawn uniformly from (w, L), which keeps w the winner; y_pred's winner is
    y_true's in every other row.  y_true: {.25, .5} below .75; y_pred: {.125, .25} below .5, so the extrema of the two maps differ.
    Spikes (map, b, v, l, value): the global minimum and maximum of each map sit in ONE voxel and label of the whole map (0 and .875;
    .0625 and .625) -- the maximum on the winner of its voxel, the minimum on a label that is not, so no arg-max moves -- and the
    extrema reductions have to carry them from one lane, wave and block."""
    P = period(V)
    maps, winners = [], []
    for k, (lo0, lo1, top, _, _) in enumerate(HARD_VALUES):
        m = np.where(rng.random((B, P, L)) < 0.5, lo0, lo1)
        w = np.stack([_spread(rng, P, L) for _ in range(B)])
        if k == 1:
            w[:, ::2] = winners[0][:, ::2]
            w[:, 1::2] = np.stack([_spread(rng, P // 2, L) for _ in range(B)])
        w2 = w + 1 + (rng.random((B, P)) * (L - 1 - w)).astype(np.int64)             # uniform in (w, L), = L where w is the last label
        w2 = np.where((rng.random((B, P)) < 0.6) & (w2 < L), w2, w)
        bi, vi = np.meshgrid(np.arange(B), np.arange(P), indexing='ij')
        m[bi, vi, w] = top
        m[bi, vi, w2] = top
        maps.append(m.astype(F))
        winners.append(w)
    spikes = []
    for k, (_, _, _, smin, smax) in enumerate(HARD_VALUES):
        b, v = int(rng.integers(0, B)), int(rng.integers(0, V))
        spikes.append((k, b, v, int(winners[k][b, v % P]), smax))
        if L > 1:
            b, v = int(rng.integers(0, B)), int(rng.integers(0, V))
            spikes.append((k, b, v, int((winners[k][b, v % P] + 1 + rng.integers(0, L - 1)) % L), smin))
    if V == P:                                                    # the period is the whole map: the spikes go in here
        for k, b, v, l, val in spikes:
            maps[k][b, v, l] = val
        spikes = []
    return maps[0], maps[1], spikes


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------

def soft_k(L, normalize):
    return 2 * L + 1 if normalize == 1 else 3 if normalize == 2 else 1


def soft_ref(t, p, V, normalize):
    """t, p: one period [B, P, L] as float64 (the stored values).  sums [B, 3, L] float64, A likewise (sums of absolute terms),
    n = V, k, minmax [4] over the maps as they enter the sums, and `terms`, the per-voxel terms of one period [B, P, 3, L]"""
    t, p = t.astype(D), p.astype(D)
    if normalize == 2:
        t = t - p
        p = t
    elif normalize == 1:
        st, sp = t.sum(-1, keepdims=True), p.sum(-1, keepdims=True)
        t = np.divide(t, st, out=np.zeros_like(t), where=st != 0)
        p = np.divide(p, sp, out=np.zeros_like(p), where=sp != 0)
    terms = np.stack([t * p, t * t, p * p], axis=2)
    L = t.shape[-1]
    return dict(sums=tiled_sum(terms, V), A=tiled_sum(np.abs(terms), V), n=V, k=soft_k(L, normalize), terms=terms,
                minmax=np.array([t.min(), t.max(), p.min(), p.max()]))


def assert_exact_soft(r, normalize):
    """the premise of the exact run: every per-voxel term is a multiple of 2^-4 (an integer without normalize) and every sum of
    absolute terms, in those units, is below 2^24 -- float32 then adds them exactly in any order"""
    scale = 16.0 if normalize == 1 else 1.0
    assert (r['terms'] * scale == np.round(r['terms'] * scale)).all()
    assert (r['A'] * scale < 2 ** 24).all(), r['A'].max() * scale


def dice_f32(sums, eps):
    """the float32 op sequence of dice_soft_finalize / dice_from_counts / dice_from_sums on sums [B, 3, L] (float32, or counts)"""
    s = np.asarray(sums).astype(F)
    top = F(2) * s[:, 0]
    bottom = s[:, 1] + s[:, 2]
    if eps > 0:
        return ((top + F(eps)) / (bottom + F(eps))).astype(F)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bottom == 0, F(0), top / bottom).astype(F)


def hard_ref(t, p, V, spikes=()):
    """one period [B, P, L] (and the spikes of the whole map, which move no arg-max) -> counts [B, 3, L] int64 (both arg-max l,
    y_true's, y_pred's); over the rows of one period of both maps: `rows`, the number whose maximum is tied (`tied`) and of those the
    number whose tied maxima lie in different label quads, the lanes of a lane group (`cross`); `wins` [2, L]: in how many rows of
    the period a label wins; minmax over the whole map"""
    B, P, L = t.shape
    at, ap = t.argmax(-1), p.argmax(-1)
    oh_t, oh_p = np.eye(L, dtype=np.int64)[at], np.eye(L, dtype=np.int64)[ap]
    counts = np.stack([tiled_sum(oh_t * oh_p, V), tiled_sum(oh_t, V), tiled_sum(oh_p, V)], axis=1)
    tied = cross = 0
    for m in (t, p):
        ismax = m == m.max(-1, keepdims=True)
        tie = ismax.sum(-1) > 1
        quads = np.add.reduceat(ismax, np.arange(0, L, 4), axis=-1) > 0
        tied += int(tie.sum())
        cross += int((tie & (quads.sum(-1) > 1)).sum())
    mm = [t.min(), t.max(), p.min(), p.max()]
    for k, b, v, l, val in spikes:
        m = (t, p)[k]
        win = (at, ap)[k][b, v % P]
        assert V > P and ((val > m.max() and win == l) or (val < m.min() and win != l))           # the arg-max of that voxel stays
        mm[2 * k], mm[2 * k + 1] = min(mm[2 * k], val), max(mm[2 * k + 1], val)
    return dict(counts=counts, rows=2 * B * P, tied=tied, cross=cross, wins=np.stack([oh_t.sum((0, 1)), oh_p.sum((0, 1))]), minmax=np.array(mm, D))


def label_ref(t, p, L):
    """integer label maps [B, V] -> counts [B, 3, L] by np.bincount; ids outside [0, L) count nowhere (tf.one_hot)"""
    out = np.zeros((t.shape[0], 3, L), np.int64)
    for b in range(t.shape[0]):
        okt, okp = (t[b] >= 0) & (t[b] < L), (p[b] >= 0) & (p[b] < L)
        out[b, 0] = np.bincount(t[b][okt & okp & (t[b] == p[b])], minlength=L)
        out[b, 1] = np.bincount(t[b][okt], minlength=L)
        out[b, 2] = np.bincount(p[b][okp], minlength=L)
    return out


def mean_ref(dice, weights):
    """K.mean(dice * weights): (float64 sum of the float32 products, n); weights None, [L] or [B, L]"""
    v = dice.astype(F) if weights is None else (dice.astype(F) * np.broadcast_to(weights.astype(F), dice.shape)).astype(F)
    return v.astype(D).sum(), v.size


KERAS_EPS = F(1e-7)
KERAS_TOP = F(1) - KERAS_EPS


def cce_ref(t, p, w, smooth, logits):
    """t, p [n, C] float64 (the stored values), w [C] float32 or None -> the per-voxel loss l [n] in float64, its bound and A (module
    docstring)"""
    n, C = t.shape
    T = t * (1.0 if w is None else w.astype(D))
    if smooth != 0:
        keep, add = F(1) - F(smooth), F(smooth) / F(C)
        T = T * D(keep) + D(add)
    assert (T >= 0).all()                                   # non-negative maps and weights: every term has the sign of -log
    if logits:
        d = p - p.max(-1, keepdims=True)
        e = np.exp(d)
        se = e.sum(-1, keepdims=True)
        lse = np.log(se)
        lq = d - lse
        E = (e * (2 + 2 * np.abs(d))).sum(-1, keepdims=True) / se
        dlq = U * (np.abs(d) + C - 1 + E + 4 + 2 * lse + np.abs(lq))
        bound = (T * dlq + (C + 4) * U * T * np.abs(lq)).sum(-1)
    else:
        q = np.clip(p / p.sum(-1, keepdims=True), D(KERAS_EPS), D(KERAS_TOP))
        lq = np.log(q)
        bound = U * (T * (C + (C + 6) * np.abs(lq))).sum(-1)
    return dict(l=-(T * lq).sum(-1), bound=bound, A=(T * np.abs(lq)).sum(-1))


def check_bounded(got, ref, bound, what=''):
    """|got - ref| <= bound element-wise, exactly 0 where the bound is 0; the worst err / bound"""
    got, ref, bound = np.asarray(got, D), np.asarray(ref, D), np.asarray(bound, D)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), what + ': not finite'
    bad = err > bound
    assert not bad.any(), '%s: %d of %d over the bound, worst err / bound %.3g' % (what, bad.sum(), bad.size, (err[bad] / np.maximum(bound[bad], 1e-300)).max())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def check_exact(got, ref, what=''):
    """bit for bit against the float64 / integer reference converted to the type of `got`"""
    got = np.asarray(got)
    want = np.asarray(ref).astype(got.dtype)
    assert np.array_equal(want.astype(D), np.asarray(ref, D)), what + ': the reference is not representable'
    if got.dtype == F:
        same = got.view(np.uint32) == want.view(np.uint32)
    else:
        same = got == want
    assert same.all(), '%s: %d of %d elements differ, first at %s: got %r want %r' % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0].tolist(), got[tuple(np.argwhere(~same)[0])], want[tuple(np.argwhere(~same)[0])])
