"""
Plain NumPy restatements of the backward contracts of the separable filter, min-max normalisation and the axis gather
(csrc/filter.hip, csrc/synth.hip), shared by tests/test_filter_bwd_cpu.py (checked there against torch float64 autograd) and
tests/test_gpu_filter_bwd.py (the kernels checked against them).  None of them calls the library.

  conv_dx_ref32 / conv_dx_ref64   dx[o, p, i] = sum_t k[t] g[o, (p + pad - t dil) / stride, i] over the t whose quotient is an integer
                in [0, out_len): from +0, terms in DESCENDING t, one rounding per multiply and per add, absent terms skipped.  The
                float64 version also returns S = sum_t |k[t]| |g|.
  conv_dk_ref64   dk[t] = sum_{o, a, i} g[o, a, i] x[o, a stride + t dil - pad, i] and S[t] = sum |g| |x|, float64.
  minmax_bwd_ref64   with m, M the extrema of a group, r = M - m: 0 when r == 0, else
                dx_i = g_i / r + [x_i == m] (Sgy - Sg) / (r n_min) - [x_i == M] Sgy / (r n_max); ties by float equality.
  gather_bwd_ref32   dx[o, a, i] = sum of g[o, j, i] over the run of outputs j that read slice a, ascending j from +0, float32.
"""

import numpy as np

F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32


def tap_range(t, A, Aout, stride, dil, pad):
    """the outputs a in [lo, hi) whose tap t reads inside the axis, and off with input index = a * stride + off"""
    off = t * dil - pad
    lo = max(0, -(off // stride))
    hi = min(Aout, (A - 1 - off) // stride + 1) if A - 1 - off >= 0 else 0
    return lo, hi, off


def _conv_dx(g, k, outer, A, inner, Aout, stride, dil, pad, dtype):
    g = np.asarray(g, dtype).reshape(outer, Aout, inner)
    k = np.asarray(k, dtype).ravel()
    dx = np.zeros((outer, A, inner), dtype)
    mag = np.zeros((outer, A, inner), np.float64) if dtype is np.float64 else None
    for t in range(k.size - 1, -1, -1):                         # descending: an element receives at most one term per tap
        lo, hi, off = tap_range(t, A, Aout, stride, dil, pad)
        if hi <= lo:
            continue
        sl = slice(lo * stride + off, (hi - 1) * stride + off + 1, stride)
        dx[:, sl] = dx[:, sl] + (k[t] * g[:, lo:hi])
        if mag is not None:
            mag[:, sl] += np.abs(k[t]) * np.abs(g[:, lo:hi])
    assert dx.dtype == dtype
    return dx, mag


def conv_dx_ref32(g, k, outer, A, inner, Aout, stride, dil, pad):
    with np.errstate(invalid='ignore', over='ignore'):
        return _conv_dx(g, k, outer, A, inner, Aout, stride, dil, pad, np.float32)[0]


def conv_dx_ref64(g, k, outer, A, inner, Aout, stride, dil, pad):
    """(the sum in float64, S = sum_t |k[t]| |g|)"""
    return _conv_dx(g, k, outer, A, inner, Aout, stride, dil, pad, np.float64)


def conv_dk_ref64(x, g, W, outer, A, inner, Aout, stride, dil, pad):
    """(dk [W] in float64, S[t] = sum |g| |x|)"""
    x = np.asarray(x, np.float64).reshape(outer, A, inner)
    g = np.asarray(g, np.float64).reshape(outer, Aout, inner)
    dk, S = np.zeros(W), np.zeros(W)
    for t in range(W):
        lo, hi, off = tap_range(t, A, Aout, stride, dil, pad)
        if hi <= lo:
            continue
        xs = x[:, lo * stride + off:(hi - 1) * stride + off + 1:stride]
        dk[t] = (g[:, lo:hi] * xs).sum()
        S[t] = (np.abs(g[:, lo:hi]) * np.abs(xs)).sum()
    return dk, S


def minmax_bwd_ref64(x, g, outer, R, inner):
    """dx in float64, and what a bound on the tie terms needs: a dict of r, n_min, n_max, sum |g|, sum |g y| per group [outer, 1, inner]"""
    x = np.asarray(x, np.float64).reshape(outer, R, inner)
    g = np.asarray(g, np.float64).reshape(outer, R, inner)
    m, M = x.min(1, keepdims=True), x.max(1, keepdims=True)
    r = M - m
    flat = r == 0
    rs = np.where(flat, 1.0, r)
    y = (x - m) / rs
    Sg, Sgy = g.sum(1, keepdims=True), (g * y).sum(1, keepdims=True)
    is_min, is_max = x == m, x == M                             # float equality: -0 == +0
    nmin, nmax = is_min.sum(1, keepdims=True), is_max.sum(1, keepdims=True)
    dx = g / rs + is_min * (Sgy - Sg) / (rs * nmin) - is_max * Sgy / (rs * nmax)
    dx = np.where(flat, 0.0, dx)
    info = dict(r=rs, flat=flat, nmin=nmin, nmax=nmax, is_min=is_min, is_max=is_max, abs_g=np.abs(g).sum(1, keepdims=True),
                abs_gy=np.abs(g * y).sum(1, keepdims=True))
    return dx, info


def run_starts(index, A):
    """run_start [A + 1] of a non-decreasing index list: the outputs that read slice a are [run_start[a], run_start[a + 1])"""
    index = np.asarray(index)
    assert (np.diff(index) >= 0).all()
    return np.searchsorted(index, np.arange(A + 1), side='left').astype(np.int32)


def gather_bwd_ref32(g, index, outer, A, inner):
    index = np.asarray(index)
    g = np.asarray(g, F).reshape(outer, index.size, inner)
    dx = np.zeros((outer, A, inner), F)
    for j in range(index.size):                                 # ascending j: the order within every run
        dx[:, index[j]] = dx[:, index[j]] + g[:, j]
    assert dx.dtype == F
    return dx


def ulp32(v):
    """the spacing of float32 at |v| (v float64): 2^(floor(log2 |v|) - 23), 2^-149 in the subnormal range and at 0"""
    v = np.abs(np.asarray(v, np.float64))
    e = np.frexp(v)[1]
    e = np.where(v == 0, -200, e)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def gamma(n):
    return n * U / (1 - n * U)


def same_geometry(n, stride, ke):
    """TF SAME: (outputs, padding in front)"""
    o = -(-n // stride)
    return o, max((o - 1) * stride + ke - n, 0) // 2


def geometry(n, W, stride, dil, padding):
    """(out_len, pad_before), or None where VALID leaves no output"""
    ke = (W - 1) * dil + 1
    if padding == 'SAME':
        return same_geometry(n, stride, ke)
    o = (n - ke) // stride + 1
    return (o, 0) if o >= 1 else None
