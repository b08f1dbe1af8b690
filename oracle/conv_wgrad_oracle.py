"""
TEST INFRASTRUCTURE ONLY -- float64 reference of the convolution weight gradient (neurite_amd/csrc/conv_bwd.hip:
nrt_conv3d_wgrad_f32 / nrt_conv3d_wgrad2_f32, nrt_hyperconv3d_wgrad_f32, nrt_conv3d_wgrad_s2d_f32, nrt_upsample_sum_f32) WITH an
element-wise error bound for a float32 implementation (CPU, numpy float64).

A plain restatement of the formulas of include/neurite_amd.h, one tap at a time over the whole zero-padded volume; nothing of the
kernels' 4 x 4 x 8 voxel tiles, channel chunks or tap-to-wave assignment is in it.  With pad = floor((k - 1) dil / 2) per axis:

    dW[tx,ty,tz,ci,co] = sum_{b,v} xin[b, v + t dil - pad, ci] dpre[b, v, co]        (zero outside the volume)
    dB[co]             = sum_{b,v} dpre[b, v, co]
    xin                = concat(x, repeat(x_lo, up)) when a second source is given
    per-entry form     : no sum over b, dW [B, ...], dB [B, cout]
    folded form        : dWf[P][t][ci][g] = sum_{b,q} x_lo[b, q + p + t - 1, ci] dY'[b, q, P group + g],
                         P = (px 2 + py) 2 + pz, t = (tx 2 + ty) 2 + tz, dY' = space_to_depth2(dpre)
    upsample_sum       : grad_lo[b, v, c] = sum over the up^3 block of grad_up[b, v up + i, offset + c]

Every function returns, besides the sums, the same sums with every term replaced by its absolute value (`A_...`) and the number
of terms `n` of one output element (B X Y Z, X Y Z per entry, ux uy uz), and

    bound = (n + 1) 2^-24 A

is the first-order bound of a sum of n float32 products added in ANY order: a term passes through at most n - 1 additions and
one product rounding, n roundings of relative size 2^-24 in all, and the + 1 covers the higher orders as long as n 2^-24 << 1.
The four waves' tap split, the LDS merge of the 1x1x1 form and the float atomics across blocks all reorder the sum; none of
them adds a rounding that is not one of the n - 1 additions.  Nothing in it is tuned on the kernels (tests/test_gpu_dispatch_arms.py
uses the same bound for channel_sums).  Where A = 0 every term is exactly zero and the result must be exactly 0.

With inputs drawn from the integers -3 .. 3 every product is an integer of magnitude <= 9 and every partial sum one of magnitude
<= 9 n; below 2^24 (`exact_condition`) float32 holds all of them exactly, in any order, float atomics included, so a float32
result must equal this reference BIT FOR BIT (`check_exact`): the check that sees one dropped, doubled or misplaced term.

Only tests/ may import this module.
"""

import numpy as np

F = np.float32
F64 = np.float64
U = 2.0 ** -24


def pad_before(k, dilation):
    return ((k - 1) * dilation) // 2


def layer_input(x, x_lo=None, up=None):
    """the tensor the layer saw, float64: x [B, X, Y, Z, c0], or concat(x, nearest up-sampling of x_lo [B, X/ux, Y/uy, Z/uz, c1])"""
    x = np.asarray(x, F64)
    if x_lo is None:
        return x
    lo = np.asarray(x_lo, F64)
    for d, u in enumerate(up):
        lo = np.repeat(lo, u, axis=1 + d)
    assert lo.shape[:4] == x.shape[:4], (lo.shape, x.shape)
    return np.concatenate([x, lo], -1)


def _tap_products(xp, g, offs, per_entry):
    """sum over the voxels of xp[b, v + offs] (x) g[b, v]: [ci, co], or [B, ci, co] per entry"""
    B, X, Y, Z, co = g.shape
    s = xp[:, offs[0]:offs[0] + X, offs[1]:offs[1] + Y, offs[2]:offs[2] + Z, :]
    ci = s.shape[-1]
    if per_entry:
        return np.matmul(s.reshape(B, -1, ci).transpose(0, 2, 1), g.reshape(B, -1, co))
    return s.reshape(-1, ci).T @ g.reshape(-1, co)


def conv_wgrad(x, grad_pre, ksize, dilation=1, x_lo=None, up=None, per_entry=False):
    """x [B, X, Y, Z, c0] (+ x_lo, up), grad_pre [B, X, Y, Z, cout] -> dict of float64 arrays: dW, A_W [kx, ky, kz, cin, cout],
    dB, A_B [cout] (a leading B axis on all four with per_entry) and n"""
    xin = layer_input(x, x_lo, up)
    g = np.asarray(grad_pre, F64)
    B, X, Y, Z, cin = xin.shape
    cout = g.shape[-1]
    assert g.shape[:4] == xin.shape[:4]
    pads = [(0, 0)] + [(pad_before(k, dilation), (k - 1) * dilation - pad_before(k, dilation)) for k in ksize] + [(0, 0)]
    xp = np.pad(xin, pads)
    xa, ga = np.abs(xp), np.abs(g)
    lead = (B,) if per_entry else ()
    dW = np.zeros(lead + tuple(ksize) + (cin, cout), F64)
    AW = np.zeros_like(dW)
    for tx in range(ksize[0]):
        for ty in range(ksize[1]):
            for tz in range(ksize[2]):
                offs = (tx * dilation, ty * dilation, tz * dilation)
                dW[..., tx, ty, tz, :, :] = _tap_products(xp, g, offs, per_entry)
                AW[..., tx, ty, tz, :, :] = _tap_products(xa, ga, offs, per_entry)
    axes = (1, 2, 3) if per_entry else (0, 1, 2, 3)
    return dict(dW=dW, A_W=AW, dB=g.sum(axes), A_B=ga.sum(axes), n=(1 if per_entry else B) * X * Y * Z)


def space_to_depth2(g):
    """y[b][q][P C + c] = g[b][2 q + p][c], P = (px 2 + py) 2 + pz (nrt_space_to_depth2_f32 as the header states it)"""
    g = np.asarray(g)
    B, X, Y, Z, C = g.shape
    assert X % 2 == 0 and Y % 2 == 0 and Z % 2 == 0
    y = np.zeros((B, X // 2, Y // 2, Z // 2, 8 * C), g.dtype)
    for px in range(2):
        for py in range(2):
            for pz in range(2):
                P = (px * 2 + py) * 2 + pz
                y[..., P * C:(P + 1) * C] = g[:, px::2, py::2, pz::2, :]
    return y


def fold_wgrad(x_lo, grad_s2d, group):
    """x_lo [B, X, Y, Z, cin], grad_s2d [B, X, Y, Z, 8 group] -> dW, A_W [8, 8, cin, group] and n = B X Y Z"""
    lo = np.asarray(x_lo, F64)
    g = np.asarray(grad_s2d, F64)
    B, X, Y, Z, cin = lo.shape
    assert g.shape == (B, X, Y, Z, 8 * group)
    xp = np.pad(lo, [(0, 0), (1, 1), (1, 1), (1, 1), (0, 0)])
    xa, ga = np.abs(xp), np.abs(g)
    dW = np.zeros((8, 8, cin, group), F64)
    AW = np.zeros_like(dW)
    for P in range(8):
        p = ((P >> 2) & 1, (P >> 1) & 1, P & 1)
        sl = slice(P * group, (P + 1) * group)
        for t in range(8):
            offs = tuple(p[d] + ((t >> (2 - d)) & 1) for d in range(3))          # q + p + t - 1 in the tensor padded by 1
            dW[P, t] = _tap_products(xp, g[..., sl], offs, False)
            AW[P, t] = _tap_products(xa, ga[..., sl], offs, False)
    return dict(dW=dW, A_W=AW, n=B * X * Y * Z)


def upsample_sum(grad_up, channel_offset, channels, up):
    """grad_up [B, X ux, Y uy, Z uz, grad_channels] -> grad_lo, A [B, X, Y, Z, channels] and n = ux uy uz"""
    g = np.asarray(grad_up, F64)[..., channel_offset:channel_offset + channels]
    B, X, Y, Z, C = g.shape
    assert X % up[0] == 0 and Y % up[1] == 0 and Z % up[2] == 0
    blocks = g.reshape(B, X // up[0], up[0], Y // up[1], up[1], Z // up[2], up[2], C)
    return dict(grad_lo=blocks.sum((2, 4, 6)), A=np.abs(blocks).sum((2, 4, 6)), n=up[0] * up[1] * up[2])


def bound(n, A):
    """|float32 sum of n float32 products in any order - exact sum| <= (n + 1) 2^-24 sum |terms|; 0 where every term is 0"""
    return (n + 1.0) * U * np.asarray(A, F64)


def exact_condition(n, amax=3):
    """inputs are integers of magnitude <= amax: every partial sum of n products stays below 2^24, where float32 is exact"""
    assert amax * amax * n < 2 ** 24, 'n = %d: integer sums may leave the exact range of float32' % n


def integers(rng, shape, amax=3):
    return rng.integers(-amax, amax + 1, size=shape).astype(F)


def ratio(got, ref, bnd):
    """worst |got - ref| / bound over the elements with a bound > 0 (inf if an element with bound 0 is not exactly 0, or if
    anything is not finite)"""
    got = np.asarray(got, F64)
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    if not np.isfinite(got).all():
        return float('inf')
    pos = bnd > 0.0
    if not np.all(got[~pos] == 0.0):
        return float('inf')
    return float((np.abs(got - ref)[pos] / bnd[pos]).max()) if pos.any() else 0.0


def check(got, ref, bnd, what=''):
    """assert |got - ref| <= bound element-wise (exactly 0 where the bound is 0); returns the worst err / bound"""
    worst = ratio(got, ref, bnd)
    assert worst <= 1.0, '%s: worst err / bound = %.3g' % (what, worst)
    return worst


def check_exact(got, ref, what=''):
    """every element of the float32 result equals the float64 reference bit for bit (integer inputs, see exact_condition)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max(initial=0.0) < 2 ** 24, 'the reference is not in the exact range'
    bad = np.argwhere(got.astype(F64) != ref)
    assert len(bad) == 0, '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, len(bad), ref.size, tuple(bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))


def emulate_f32(x, grad_pre, ksize, dilation, rng, x_lo=None, up=None):
    """the shared weight gradient in float32 numpy: every product rounded to float32, the terms of every output element added one
    by one in a shuffled order (one rounding per addition): what waves, an LDS merge and float atomics may legitimately return.
    Small shapes only (all n terms of every element are held at once)."""
    xin = layer_input(x, x_lo, up).astype(F)
    g = np.asarray(grad_pre, F)
    B, X, Y, Z, cin = xin.shape
    cout = g.shape[-1]
    pads = [(0, 0)] + [(pad_before(k, dilation), (k - 1) * dilation - pad_before(k, dilation)) for k in ksize] + [(0, 0)]
    xp = np.pad(xin, pads)
    dW = np.zeros(tuple(ksize) + (cin, cout), F)
    gf = g.reshape(-1, 1, cout)
    for tx in range(ksize[0]):
        for ty in range(ksize[1]):
            for tz in range(ksize[2]):
                s = xp[:, tx * dilation:tx * dilation + X, ty * dilation:ty * dilation + Y, tz * dilation:tz * dilation + Z, :]
                terms = (s.reshape(-1, cin, 1) * gf).astype(F)                   # [n, cin, cout]
                terms = terms[rng.permutation(terms.shape[0])]
                dW[tx, ty, tz] = np.cumsum(terms, axis=0, dtype=F)[-1]
    gb = g.reshape(-1, cout)
    dB = np.cumsum(gb[rng.permutation(gb.shape[0])], axis=0, dtype=F)[-1]
    return dW, dB
