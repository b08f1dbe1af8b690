"""
TEST INFRASTRUCTURE ONLY -- float64 reference of the warp backward (neurite_amd/csrc/backward.hip: nrt_interpn_bwd_f32 and
nrt_interpn_nearest_bwd_f32) WITH an element-wise error bound for a float32 implementation (CPU, torch float64).

A direct restatement of corner_1d, out_of_bounds and load_loc of neurite_amd/csrc/interpn_core.h for D = 1, 2, 3, starting from
the float32 location the kernel forms (`locations`).  Besides the gradients it returns what a bound on a float32 scatter needs:

    grad_vol, grad_loc   the gradients
    A_vol, A_loc         the same sums with every term replaced by its absolute value
    Ap_vol, Ap_loc       the same absolute sums with every 1-D weight w0, w1 increased by u = 2^-24
    T_vol [rows]         the number of live (voxel, corner) pairs that land on each volume row

and `bound_vol` / `bound_loc` turn them into

    |got - ref| <= (T + 16) u A' + (A' - A) + T 2^-126            T = T_vol[row] for grad_vol, 2^D C for grad_loc

(T + 16) u is the first-order bound (T - 1 + k) u of a sum of T float32 terms added in ANY order (float atomics, the LDS merge and
the lane shuffles all reorder the sum) whose terms carry k <= 14 roundings each: two per weight product, one for w0 = l1 - cl, the
4-term dot product, the mask and weight factors.  A' - A is there because w1 = 1 - w0 is rounded absolutely, not relatively: a w0
within 2^-25 of 1 leaves w1 = 0, and the upper-corner row may receive nothing else.  T 2^-126 allows hardware float atomics that
flush subnormals.  Where every term of an element is exactly zero (A' = 0) the bound is 0 and the result must be exactly 0.
None of the constants is tuned on the kernels; tests/test_oracle.py checks the bound against a float32 emulation of the same
formulas (`emulate_f32`, corners and pairs in shuffled order) and that `check` rejects small mutations.

The sums run through torch.index_add_ on float64 tensors (np.add.at takes several times as long at the 8.65 M output elements of
the largest GPU case).  Only tests/ may import this module.
"""

import itertools

import numpy as np
import torch

F = np.float32
F64 = torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
ABSOLUTE, SHIFT, LINSPACE = 0, 1, 2


def locations(mode, S, O, loc=None):
    """the float32 location load_loc forms for every output voxel: [*O, D] float32.
    ABSOLUTE: as given.  SHIFT: float32(q) + shift, one rounding.  LINSPACE: tf.linspace(0, S - 1, O) as fill_args / load_loc
    compute it: delta = fl(fl(S - 1) / fl(O - 1)), first = 0, last = S - 1 exactly, middle = fl(delta * i)."""
    D = len(S)
    O = tuple(int(o) for o in O)
    if mode == ABSOLUTE:
        return np.ascontiguousarray(loc, F).reshape(O + (D,))
    if mode == SHIFT:
        grid = np.stack(np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij'), -1)
        return (grid + np.asarray(loc, F).reshape(O + (D,))).astype(F)
    lin = []
    for d in range(D):
        delta = F(F(S[d] - 1) / F(O[d] - 1)) if O[d] > 1 else F(0)
        x = (delta * np.arange(O[d], dtype=F)).astype(F)
        x[-1] = F(S[d] - 1)
        x[0] = F(0)                                   # (qd == 0 is tested first: O = 1 gives 0)
        lin.append(x)
    return np.stack(np.meshgrid(*lin, indexing='ij'), -1).astype(F)


def make_field(rng, S, O, C, kind, mode):
    """test inputs: vol [*S, C], grad_out [*O, C] standard normal, and the location tensor of `mode` (None for LINSPACE) around
    the grid that maps the output onto the source.  'smooth': noise of amplitude 1.5, every 7th location put on an integer, every
    11th on the far border, every 13th on 0 (one component each: the kinks of clip and floor); 'rough': amplitude 12, most
    locations clipped.  In SHIFT mode the shift is location - voxel, so the kinks survive the kernel's float32 addition."""
    D = len(S)
    vol = rng.standard_normal(tuple(S) + (C,)).astype(F)
    gout = rng.standard_normal(tuple(O) + (C,)).astype(F)
    if mode == LINSPACE:
        return vol, None, gout
    grid = np.stack(np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij'), -1)
    scale = np.array([(S[d] - 1) / max(O[d] - 1, 1) for d in range(D)], F)
    pos = (grid * scale + rng.standard_normal(tuple(O) + (D,)) * (1.5 if kind == 'smooth' else 12.0)).astype(F)
    if kind == 'smooth':
        flat = pos.reshape(-1, D)
        n = flat.shape[0]
        for k in range(0, n, 7):
            flat[k, k % D] = F(rng.integers(0, S[k % D]))
        for k in range(3, n, 11):
            flat[k, k % D] = F(S[k % D] - 1)
        for k in range(5, n, 13):
            flat[k, k % D] = 0.0
    return vol, (pos if mode == ABSOLUTE else (pos - grid).astype(F)), gout


def _corners(p, S, xp):
    """corner_1d per dimension on the float32 locations p [n, D] widened to float64 (every op below is then exact up to the
    float64 rounding of 1 - w0).  xp = torch or numpy.  Returns i0, i1 (integer), w0, w1, m per dimension."""
    D = p.shape[1]
    i0, i1, w0, w1, m = [], [], [], [], []
    for d in range(D):
        mx = float(S[d] - 1)
        pd = p[:, d]
        cl = xp.clip(pd, 0.0, mx)
        l0 = xp.clip(xp.floor(pd), 0.0, mx)
        l1 = xp.clip(l0 + 1.0, 0.0, mx)
        a = l1 - cl
        i0.append(l0), i1.append(l1), w0.append(a), w1.append(1.0 - a)
        m.append(((pd >= 0.0) & (pd <= mx)))
    return i0, i1, w0, w1, m


def _oob(p, S):
    o = None
    for d in range(p.shape[1]):
        t = (p[:, d] < 0.0) | (p[:, d] > float(S[d] - 1))
        o = t if o is None else (o | t)
    return o


def warp_bwd(vol, loc32, grad_out, fill=False):
    """vol [*S, C], loc32 [*O, D] float32 (see `locations`), grad_out [*O, C]; fill: a fill value is set (the out-of-bounds voxels
    pass no gradient).  Returns a dict of float64 numpy arrays: grad_vol, A_vol, Ap_vol [*S, C]; T_vol [*S]; grad_loc, A_loc,
    Ap_loc [*O, D]; and `oob_share`, the share of masked voxels."""
    assert loc32.dtype == np.float32
    D = loc32.shape[-1]
    S, C = tuple(vol.shape[:D]), vol.shape[-1]
    O = tuple(loc32.shape[:-1])
    rows = int(np.prod(S))
    v = torch.from_numpy(np.ascontiguousarray(vol, np.float64)).reshape(rows, C)
    g = torch.from_numpy(np.ascontiguousarray(grad_out, np.float64)).reshape(-1, C)
    p = torch.from_numpy(np.ascontiguousarray(loc32)).reshape(-1, D).double()
    n = p.shape[0]
    i0, i1, w0, w1, m = _corners(p, S, torch)
    live = ~_oob(p, S) if fill else torch.ones(n, dtype=torch.bool)
    keep = live.double()
    g = g * keep[:, None]
    ga = g.abs()
    mf = [x.double() * keep for x in m]
    w = [w0, w1]
    wp = [[x + U for x in w0], [x + U for x in w1]]
    ii = [[x.long() for x in i0], [x.long() for x in i1]]
    # grad_vol | A_vol side by side: one index_add_ per corner for both
    acc = torch.zeros(rows, 2 * C, dtype=F64)
    accp = torch.zeros(rows, C, dtype=F64)
    tv = torch.zeros(rows, dtype=F64)
    gl = torch.zeros(n, D, dtype=F64)
    al = torch.zeros(n, D, dtype=F64)
    alp = torch.zeros(n, D, dtype=F64)
    for c in itertools.product((0, 1), repeat=D):
        idx = torch.zeros(n, dtype=torch.long)
        wt = torch.ones(n, dtype=F64)
        wtp = torch.ones(n, dtype=F64)
        for d in range(D):
            idx = idx * S[d] + ii[c[d]][d]
            wt = wt * w[c[d]][d]
            wtp = wtp * wp[c[d]][d]
        acc.index_add_(0, idx, torch.cat([g * wt[:, None], ga * wt.abs()[:, None]], 1))
        accp.index_add_(0, idx, ga * wtp[:, None])
        tv.index_add_(0, idx, keep)
        vr = v[idx]
        dot = (g * vr).sum(1)
        dota = (ga * vr.abs()).sum(1)
        for d in range(D):
            ex = torch.ones(n, dtype=F64)
            exp_ = torch.ones(n, dtype=F64)
            for e in range(D):
                if e != d:
                    ex = ex * w[c[e]][e]
                    exp_ = exp_ * wp[c[e]][e]
            sgn = 1.0 if c[d] else -1.0
            gl[:, d] += sgn * mf[d] * ex * dot
            al[:, d] += mf[d] * ex.abs() * dota
            alp[:, d] += mf[d] * exp_ * dota
    return dict(grad_vol=acc[:, :C].reshape(S + (C,)).numpy(), A_vol=acc[:, C:].reshape(S + (C,)).numpy(),
                Ap_vol=accp.reshape(S + (C,)).numpy(), T_vol=tv.reshape(S).numpy(),
                grad_loc=gl.reshape(O + (D,)).numpy(), A_loc=al.reshape(O + (D,)).numpy(), Ap_loc=alp.reshape(O + (D,)).numpy(),
                oob_share=1.0 - float(keep.mean()), D=D, C=C)


def _bound(T, A, Ap):
    b = (T + 16.0) * U * Ap + (Ap - A) + T * TINY
    return np.where(Ap > 0.0, b, 0.0)          # every term exactly zero: so is any float32 sum of them


def bound_vol(r):
    return _bound(r['T_vol'][..., None], r['A_vol'], r['Ap_vol'])


def bound_loc(r):
    return _bound(float(2 ** r['D'] * r['C']), r['A_loc'], r['Ap_loc'])


def nearest_bwd(S, C, loc32, grad_out, fill=False):
    """nearest interpolation: grad_vol is the scatter of grad_out into row clip(round_half_even(p)).  Returns grad_vol, A_vol
    (sum of |g|) [*S, C] and T_vol [*S] (voxels per row)."""
    D = loc32.shape[-1]
    S = tuple(S)
    rows = int(np.prod(S))
    p = torch.from_numpy(np.ascontiguousarray(loc32)).reshape(-1, D).double()
    g = torch.from_numpy(np.ascontiguousarray(grad_out, np.float64)).reshape(-1, C)
    keep = (~_oob(p, S)).double() if fill else torch.ones(p.shape[0], dtype=F64)
    g = g * keep[:, None]
    idx = torch.zeros(p.shape[0], dtype=torch.long)
    for d in range(D):
        idx = idx * S[d] + torch.clip(torch.round(p[:, d]), 0.0, float(S[d] - 1)).long()       # torch.round: half to even
    acc = torch.zeros(rows, 2 * C, dtype=F64).index_add_(0, idx, torch.cat([g, g.abs()], 1))
    tv = torch.zeros(rows, dtype=F64).index_add_(0, idx, keep)
    return dict(grad_vol=acc[:, :C].reshape(S + (C,)).numpy(), A_vol=acc[:, C:].reshape(S + (C,)).numpy(), T_vol=tv.reshape(S).numpy())


def bound_nearest(r):
    """a sum of T exact float32 terms in any order: (T - 1) u A to first order; (T + 1) u A covers the higher orders"""
    return (r['T_vol'][..., None] + 1.0) * U * r['A_vol'] + r['T_vol'][..., None] * TINY * (r['A_vol'] > 0)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements with a bound > 0 (inf if an element with bound 0 is not exactly 0)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    pos = bound > 0.0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if not np.all(got[~pos] == 0.0):
        return float('inf')
    return worst if np.isfinite(got).all() else float('inf')


def check(got, ref, bound, what=''):
    """assert |got - ref| <= bound element-wise (exactly 0 where the bound is 0); prints and returns the worst err / bound"""
    worst = ratio(got, ref, bound)
    print('%s: worst err / bound = %.3g' % (what, worst))
    assert worst <= 1.0, '%s: worst err / bound = %.3g' % (what, worst)
    return worst


def emulate_f32(vol, loc32, grad_out, fill, rng):
    """the same formulas in float32 numpy, one rounding per operation as the kernels' scalar forms have, with the (voxel, corner)
    pairs of grad_vol added in a shuffled order and the corner x channel terms of grad_loc likewise: what a float32 scatter may
    legitimately return.  Small shapes only (np.add.at)."""
    D = loc32.shape[-1]
    S, C = tuple(vol.shape[:D]), vol.shape[-1]
    O = tuple(loc32.shape[:-1])
    rows = int(np.prod(S))
    v = np.ascontiguousarray(vol, F).reshape(rows, C)
    g = np.ascontiguousarray(grad_out, F).reshape(-1, C)
    p = loc32.reshape(-1, D)
    n = p.shape[0]
    i0, i1, w0, w1, m = [], [], [], [], []
    for d in range(D):
        mx = F(S[d] - 1)
        cl = np.clip(p[:, d], F(0), mx)
        l0 = np.clip(np.floor(p[:, d]), F(0), mx)
        l1 = np.clip(l0 + F(1), F(0), mx)
        a = (l1 - cl).astype(F)
        i0.append(l0.astype(np.int64)), i1.append(l1.astype(np.int64)), w0.append(a), w1.append((F(1) - a).astype(F))
        m.append(((p[:, d] >= 0) & (p[:, d] <= mx)).astype(F))
    live = ~_oob(p, S) if fill else np.ones(n, bool)
    w, ii = [w0, w1], [i0, i1]
    pair_idx, pair_val, loc_terms = [], [], [[] for _ in range(D)]
    for c in itertools.product((0, 1), repeat=D):
        idx = np.zeros(n, np.int64)
        wt = np.ones(n, F)
        for d in range(D):
            idx = idx * S[d] + ii[c[d]][d]
            wt = (wt * w[c[d]][d]).astype(F)
        pair_idx.append(idx[live])
        pair_val.append((wt[:, None] * g).astype(F)[live])
        vr = v[idx]
        for d in range(D):
            ex = (m[d] if c[d] else -m[d]).astype(F)
            for e in range(D):
                if e != d:
                    ex = (ex * w[c[e]][e]).astype(F)
            loc_terms[d].append((((g * vr).astype(F)) * ex[:, None]).astype(F))
    pair_idx, pair_val = np.concatenate(pair_idx), np.concatenate(pair_val)
    order = rng.permutation(pair_idx.shape[0])
    gv = np.zeros((rows, C), F)
    np.add.at(gv, pair_idx[order], pair_val[order])                      # unbuffered: one float32 rounding per add, in this order
    gl = np.zeros((n, D), F)
    for d in range(D):
        t = np.concatenate(loc_terms[d], 1)
        t = t[:, rng.permutation(t.shape[1])]
        gl[:, d] = np.cumsum(t, axis=1, dtype=F)[:, -1]                   # sequential float32 sum
    gl[~live] = 0
    return gv.reshape(S + (C,)), gl.reshape(O + (D,))
