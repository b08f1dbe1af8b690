"""
Every dispatch arm of the separable filter and the min-max kernels (csrc/filter.hip), through the C ABI, on guarded buffers whose
alignment is exact (tests/arm_buffers.py).  One pytest id names the kernel that the dispatcher's conditions send the case to: there
is no hook that reports the arm, so `arm_of` restates the three `if`s of nrt_conv1d_axis_f32 and every case asserts that its id is
what they pick.

References, all plain NumPy, none of them another arm of the library:
  conv1d_ref32   the contract of the file restated in float32: an output starts at +0 and receives its taps in ascending order, one
                 rounding per multiply and per add, out-of-range taps skipped.  The library is built with -ffp-contract=off, so
                 this is the bit-for-bit reference of EVERY conv arm, plain and fast.
  conv1d_ref64   the same sum in float64 and S = sum_t |k[t]| |x|.  Every finite case also asserts
                 |got - ref64| <= gamma_{W+1} S + ulp32(|ref64|) / 2, gamma_n = n u / (1 - n u), u = 2^-24: the standard bound of a
                 sequential sum of W rounded products plus the rounding of ref64 to float32 -- no measured margin.  It guards against
                 conv1d_ref32 and the kernel sharing a mistake; test_conv1d_ref32_against_oracle checks conv1d_ref32 against
                 oracle.np_oracle.conv1d_axis within that bound without a GPU.
  min-max        mn, mx by np.min / np.max over the reduced axis, y = where(mx - mn != 0, (x - mn) / (mx - mn), 0) in float32, bit for
                 bit (float division is correctly rounded in this build).  np.min / np.max leave the sign of a zero extreme to the
                 order of the elements; the kernels order -0 below +0, and `extrema` says so for the reference.
  bin centres    oracle.np_oracle.tf_linspace, bit for bit.

Bits are compared on the integer view; a NaN equals a NaN at the same position, payloads are not compared.

NaN in a min-max INPUT is out of scope: what the reference library does with it could not be recorded, so nothing here puts a NaN
into a min-max input (NaN appears only in results, e.g. Inf - Inf).  That case stays open.

Which test reaches which launch of csrc/filter.hip (ids in brackets are prefixes):
  nrt_conv1d_axis_f32
    conv1d_inner_lds            test_conv_inner_lds[*]; the other side of test_conv_boundary_pair[W256|257-inner1, out7|8-inner1, outer7|8]
    conv1d_axis_rows<true,8>    test_conv_rows[conv1d_axis_rows<true,8>-*], ...second_grid_stride_iteration[conv1d_axis_rows<true,8>-*]
    conv1d_axis_rows<false,8>   test_conv_rows[conv1d_axis_rows<false,8>-*], ...second_grid_stride_iteration[conv1d_axis_rows<false,8>-*]
    conv1d_axis_run4            test_conv_run4[*], ...second_grid_stride_iteration[conv1d_axis_run4-*]
    conv1d_axis<true>           test_conv_axis[conv1d_axis<true>-*], ...second_grid_stride_iteration[conv1d_axis<true>-*]
    conv1d_axis<false>          test_conv_axis[conv1d_axis<false>-*], ...second_grid_stride_iteration[conv1d_axis<false>-*]
    first `if` (inner_lds) declined because of: NRT_CONV1D_GENERIC  test_conv_run4[*-generic-*];
        stride / dilation  test_conv_axis[*-inner1-stride*]; W > 256  test_conv_run4[*-W257-*];
        out_len < 8  test_conv_axis[*-inner1-out7]; inner != 1  test_conv_rows[*];
        outer < 8  test_conv_run4[*-outer7]; y unaligned  test_conv_run4[*-y+1].  Its inner `nblk < 2^31` is never false here: that takes
        2^31 blocks of at least 512 outputs, terabytes of output
    second `if` (rows): vec and inner >= 64  [conv1d_axis_rows<true,8>-inner64]; not vec and inner >= 32
        [conv1d_axis_rows<false,8>-inner33, -inner32-x+1, -inner64-y+1]; declined: vec and inner < 64
        test_conv_axis[conv1d_axis<true>-inner32, -inner60]; not vec and
        inner < 32  test_conv_axis[conv1d_axis<false>-inner31*]; not fast  test_conv_axis[*-inner64-W257*, *-generic*, *-stride*]
    third `if`: run4 as above; declined by W > 1024  [conv1d_axis<false>-inner1-W1025-*], out_len < 8  [*-inner1-out7*], stride /
        dilation  [*-inner1-stride*]; then vec  [conv1d_axis<true>-*] or not  [conv1d_axis<false>-*]
    test_conv_boundary_pair runs both sides of inner 31|32, 60|64, W 256|257, 1024|1025, out_len 7|8, outer 7|8
  nrt_minmax_norm_f32
    inner == 1: minmax_reduce1, minmax_apply1   test_minmax_inner1_lengths, test_minmax_inner1_data_shapes; nb at its cap of 256
        test_minmax_inner1_block_caps[reduce1-block-cap]; `ab` at either cap  [apply1-cap-64], [apply1-cap-4096/outer]
    inner > 1: minmax_init, minmax_reduce, minmax_apply   test_minmax_columns, test_minmax_columns_data_shapes; bx at its cap of 2048 and
        the second iteration of minmax_init  test_minmax_columns_block_caps.  `bx < 1` cannot happen (reduce_len >= 1), and the
        `inner == 1` halves of minmax_reduce / minmax_apply are not reached from this dispatcher, which sends inner == 1 elsewhere
    refusals, no-ops, workspace   test_minmax_refusals_and_limits, test_minmax_workspace, test_extrema_refusals
  nrt_minmax_f32: minmax_reduce1, minmax_decode   test_minmax_f32
  nrt_bin_centers_f32: minmax_reduce1, minmax_centers   test_bin_centers
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
from arm_buffers import Buf, Bytes, call
from neurite_amd import _lib
from oracle import np_oracle as npo

gpu = pytest.mark.gpu
F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
GRID = 4096 * 256                   # work items of one grid-stride iteration: fblocks() caps the grid at 4096 blocks of 256


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------

def _conv1d(x, k, outer, A, inner, Aout, stride, dil, pad, dtype):
    """y[o, a, i] = sum_t k[t] x[o, a stride + t dil - pad, i] in `dtype`: from +0, taps ascending, one rounding per multiply and per
    add, out-of-range taps skipped (not multiplied).  The valid outputs of a tap are a run of consecutive a, so they are a slice."""
    x = np.asarray(x, dtype).reshape(outer, A, inner)
    k = np.asarray(k, dtype).ravel()
    acc = np.zeros((outer, Aout, inner), dtype)
    mag = np.zeros((outer, Aout, inner), np.float64) if dtype is np.float64 else None
    for t in range(k.size):
        off = t * dil - pad                                     # input index of output a: a * stride + off
        lo = max(0, -(off // stride))                           # first a with a * stride + off >= 0
        hi = min(Aout, (A - 1 - off) // stride + 1) if A - 1 - off >= 0 else 0          # one past the last a with ... <= A - 1
        if hi <= lo:
            continue
        xs = x[:, lo * stride + off:(hi - 1) * stride + off + 1:stride]
        acc[:, lo:hi] = acc[:, lo:hi] + (k[t] * xs)
        if mag is not None:
            mag[:, lo:hi] += np.abs(k[t]) * np.abs(xs)
    assert acc.dtype == dtype
    return acc, mag


def conv1d_ref32(x, k, outer, A, inner, Aout, stride, dil, pad):
    with np.errstate(invalid='ignore', over='ignore'):
        return _conv1d(x, k, outer, A, inner, Aout, stride, dil, pad, np.float32)[0]


def conv1d_ref64(x, k, outer, A, inner, Aout, stride, dil, pad):
    """(the sum in float64, S = sum_t |k[t]| |x|)"""
    return _conv1d(x, k, outer, A, inner, Aout, stride, dil, pad, np.float64)


def ulp32(v):
    """the spacing of float32 at |v| (v float64): 2^(floor(log2 |v|) - 23), 2^-149 in the subnormal range and at 0"""
    v = np.abs(np.asarray(v, np.float64))
    e = np.frexp(v)[1]                                          # |v| = m 2^e, 0.5 <= m < 1
    e = np.where(v == 0, -200, e)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def conv_bound(ref64, S, W):
    n = W + 1
    return n * U / (1 - n * U) * S + ulp32(ref64) / 2


def bits_differ(got, ref):
    got, ref = np.ascontiguousarray(got, F), np.ascontiguousarray(ref, F)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))


def assert_bits(got, ref, what):
    bad = bits_differ(got, ref)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d values differ from the reference, the first at %s: got %r, reference %r'
                             % (what, int(bad.sum()), bad.size, at, np.asarray(got)[at], np.asarray(ref)[at]))


def same_geometry(n, stride, ke):
    """TF SAME: (outputs, padding in front)"""
    o = -(-n // stride)
    return o, max((o - 1) * stride + ke - n, 0) // 2


def test_conv1d_ref32_against_oracle():
    """no GPU: the float32 restatement against the project's float64 oracle, within the bound that the kernels are held to"""
    rng = np.random.default_rng(5)
    outer, A, inner = 2, 29, 3
    x = rng.standard_normal((outer, A, inner)).astype(F)
    worst = 0.0
    for W in (1, 4, 5, 8, 9):
        k = rng.standard_normal(W).astype(F)
        for stride in (1, 2, 3):
            for dil in (1, 2, 3):
                ke = (W - 1) * dil + 1
                for padding in ('SAME', 'VALID'):
                    Aout, pad = same_geometry(A, stride, ke) if padding == 'SAME' else ((A - ke) // stride + 1, 0)
                    want = npo.conv1d_axis(x.astype(np.float64), k, 1, padding, stride, dil)
                    assert want.dtype == np.float64 and want.shape == (outer, Aout, inner)
                    got = conv1d_ref32(x, k, outer, A, inner, Aout, stride, dil, pad)
                    assert got.dtype == F
                    ref64, S = conv1d_ref64(x, k, outer, A, inner, Aout, stride, dil, pad)
                    np.testing.assert_allclose(ref64, want, rtol=1e-14, atol=1e-14)      # two float64 sums of at most 9 terms
                    bound = conv_bound(want, S, W)
                    err = np.abs(got.astype(np.float64) - want)
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (W, stride, dil, padding)
    print('conv1d_ref32 against the oracle: largest error / bound = %.3g' % worst)
    assert worst > 0                                            # float32 rounds: an error of exactly 0 everywhere means float64 ran


def test_ulp32():
    for v, e in ((1.0, -23), (1.5, -23), (2.0 - 2.0 ** -30, -23), (2.0, -22), (-7.0, -21), (2.0 ** -126, -149), (3e-39, -149), (0.0, -149)):
        assert ulp32(v) == 2.0 ** e, v
    assert ulp32(1.0) == np.spacing(F(1)) and ulp32(1e30) == np.spacing(F(1e30))


# ------------------------------------------------------------------------------------------------------------------------------
# nrt_conv1d_axis_f32: the dispatcher restated, the cases
# ------------------------------------------------------------------------------------------------------------------------------

INNER_LDS, RUN4, AXIS_S, AXIS_V = 'conv1d_inner_lds', 'conv1d_axis_run4', 'conv1d_axis<false>', 'conv1d_axis<true>'
ROWS_S, ROWS_V = 'conv1d_axis_rows<false,8>', 'conv1d_axis_rows<true,8>'


def arm_of(outer, inner, out_len, W, stride=1, dil=1, xo=0, yo=0, generic=False):
    """the kernel nrt_conv1d_axis_f32 launches: its three dispatch `if`s, with (pointer & 15) == 0 written as offset == 0"""
    vec = inner % 4 == 0 and xo == 0 and yo == 0
    fast = (not generic) and stride == 1 and dil == 1 and W <= 256 and out_len >= 8
    if fast and inner == 1 and outer >= 8 and yo == 0:
        return INNER_LDS
    if fast and ((vec and inner >= 64) or (not vec and inner >= 32)):
        return ROWS_V if vec else ROWS_S
    if inner == 1 and stride == 1 and dil == 1 and out_len >= 8 and W <= 1024:
        return RUN4
    return AXIS_V if vec else AXIS_S


def ci_geometry(out_len, W):
    """(log2 of the lanes per row, segments per row, floats of a staged row) of conv1d_inner_lds, as the host function of that name"""
    wp = -(-W // 8) * 8
    best = None
    for l2 in (2, 3, 4, 5):
        seg = 8 << l2
        segs = -(-out_len // seg)
        cost = segs * (seg + wp + 8)
        if best is None or cost < best[0]:
            best = (cost, l2, segs, seg + wp + 8)
    return best[1:]


def geometry(c):
    """(axis_len, out_len, pad_before) of a case: pad 'SAME' / 'VALID' by the TF rules from `A` or from the wanted `out_len`; an integer
    pad is passed as it is, with axis_len = out_len * stride unless both are given"""
    W, s, d = c['W'], c.get('stride', 1), c.get('dil', 1)
    ke = (W - 1) * d + 1
    pad = c.get('pad', 'SAME')
    if pad == 'SAME':
        A = c['A'] if 'A' in c else c['out_len'] * s
        o, before = same_geometry(A, s, ke)
    elif pad == 'VALID':
        A = c['A'] if 'A' in c else (c['out_len'] - 1) * s + ke
        o, before = (A - ke) // s + 1, 0
    else:
        A = c['A'] if 'A' in c else c['out_len'] * s
        o, before = c.get('out_len', -(-A // s)), int(pad)
    assert 'out_len' not in c or o == c['out_len'], c
    return A, o, before


SPECIALS = np.array([np.inf, -0.0, np.nan, -np.inf], F)


def conv_inputs(c, A, seed):
    """standard-normal inputs and mixed-sign random taps (Gaussian taps are positive and symmetric: they hide order and mirror
    errors).  data = 'edges': Inf, -0, NaN, -Inf at the two positions next to either border, in an order that changes with (o, i).
    taps = 'inf' / 'nan': that value at one tap."""
    rng = np.random.default_rng(seed)
    outer, inner, W = c['outer'], c['inner'], c['W']
    k = rng.standard_normal(W).astype(F)                        # first: cases that differ in the shape of x alone share their taps
    x = rng.standard_normal((outer, A, inner)).astype(F)
    if c.get('data') == 'edges':
        oi = np.arange(outer)[:, None] + np.arange(inner)[None, :]
        for j, a in enumerate(sorted({0, min(1, A - 1), max(A - 2, 0), A - 1})):
            x[:, a, :] = SPECIALS[(j + oi) % 4]
    if c.get('taps') in ('inf', 'nan'):
        k[(2 * W) // 3] = np.inf if c['taps'] == 'inf' else np.nan
    return x, k


def run_conv(dev, x, k, outer, A, inner, Aout, stride, dil, pad, xo=0, yo=0):
    """inputs are guarded buffers too, with the fill value outside: a read one element past a row mixes -12345 into a border output"""
    xb, kb, yb = Buf(dev, x.size, xo, x), Buf(dev, k.size, 0, k), Buf(dev, outer * Aout * inner, yo)
    call(dev, 'nrt_conv1d_axis_f32', xb.p, kb.p, yb.p, outer, A, inner, Aout, k.size, stride, dil, pad)
    return yb.get((outer, Aout, inner))


def check_conv(dev, c, monkeypatch, seed=0):
    """one case, once per x offset it lists: the id's arm is what the dispatcher picks, the result equals conv1d_ref32 bit for bit
    and, when everything is finite, lies within the float64 bound"""
    A, Aout, pad = geometry(c)
    outer, inner, W, s, d = c['outer'], c['inner'], c['W'], c.get('stride', 1), c.get('dil', 1)
    x, k = conv_inputs(c, A, seed)
    ref = conv1d_ref32(x, k, outer, A, inner, Aout, s, d, pad)
    finite = bool(np.isfinite(x).all() and np.isfinite(k).all())
    if c.get('generic'):
        monkeypatch.setenv('NRT_CONV1D_GENERIC', '1')
    else:
        monkeypatch.delenv('NRT_CONV1D_GENERIC', raising=False)
    got = None
    for xo in c.get('xo', (0,)):
        yo = c.get('yo', 0)
        what = '%s %s xo %d yo %d' % (c['arm'], c['tag'], xo, yo)
        assert arm_of(outer, inner, Aout, W, s, d, xo, yo, c.get('generic', False)) == c['arm'], what
        got = run_conv(dev, x, k, outer, A, inner, Aout, s, d, pad, xo, yo)
        assert_bits(got, ref, what)
        if finite:
            worst = 0.0
            for o in range(outer):                              # row by row: the float64 copies of the largest case stay small
                ref64, S = conv1d_ref64(x[o], k, 1, A, inner, Aout, s, d, pad)
                bound = conv_bound(ref64, S, W)
                err = np.abs(got[o].astype(np.float64) - ref64[0])
                assert (err <= bound[0]).all(), what
                worst = max(worst, float((err / bound[0]).max()))
            print('%s: largest error / bound = %.3g' % (what, worst))
    monkeypatch.delenv('NRT_CONV1D_GENERIC', raising=False)
    return got


def case(arm, tag, **kw):
    kw.update(arm=arm, tag=tag)
    return pytest.param(kw, id='%s-%s' % (arm, tag))


BOTH = (0, 1)       # conv1d_inner_lds reads x with 4-byte-aligned loads: the alignment of x must not matter, so run both

# conv1d_inner_lds: inner == 1, outer >= 8, out_len >= 8, W <= 256, stride 1, dilation 1, y 16-byte aligned
INNER_LDS_CASES = (
    # W = 5: out_len 32 / 64 / 128 / 256 pick 4 / 8 / 16 / 32 lanes per row; 96 / 192 / 384 / 512 the same with more than one segment
    [case(INNER_LDS, 'lanes%d-out%d' % (lanes, n), outer=11, inner=1, W=5, out_len=n, xo=BOTH)
     for lanes, n in ((4, 32), (8, 64), (16, 128), (32, 256), (4, 96), (8, 192), (16, 384), (32, 512))] +
    # the store: out_len % 4 != 0 is the scalar store; 36 is the vector store in the full lanes, the scalar one in the partial lane,
    # and lanes past the end return
    [case(INNER_LDS, 'store-out%d' % n, outer=9, inner=1, W=7, out_len=n, xo=BOTH) for n in (8, 9, 34, 35, 36, 37, 67)] +
    # rows: 8 of a block's 64; 70 = one full block and 6 rows; 9 rows of 8 per block (32 lanes per row) = a second block of one row
    [case(INNER_LDS, 'rows-outer8', outer=8, inner=1, W=5, out_len=32, xo=BOTH),
     case(INNER_LDS, 'rows-outer70', outer=70, inner=1, W=5, out_len=32, xo=BOTH),
     case(INNER_LDS, 'rows-outer9-out256', outer=9, inner=1, W=5, out_len=256, xo=BOTH)] +
    # widths across the tap-block limits, SAME / VALID / a pad_before that is neither
    [case(INNER_LDS, 'W%d-%s' % (W, 'pad%d' % (W - 1) if pad == 'full' else pad), outer=9, inner=1, W=W, out_len=40,
          pad=W - 1 if pad == 'full' else pad, xo=BOTH)
     for W in (1, 4, 8, 9, 255, 256) for pad in ('SAME', 'VALID', 'full')] +
    [case(INNER_LDS, 'axis9-W31', outer=8, inner=1, W=31, A=9, xo=BOTH),
     # the largest dynamic LDS request: 64 rows of 296 floats and the taps, 76 832 bytes
     case(INNER_LDS, 'lds-max-W256-out16-outer64', outer=64, inner=1, W=256, out_len=16, xo=BOTH),
     # a non-finite tap: the plain loop inside the fast kernel
     case(INNER_LDS, 'tap-inf', outer=9, inner=1, W=11, out_len=40, taps='inf', xo=BOTH),
     case(INNER_LDS, 'tap-nan', outer=9, inner=1, W=11, out_len=40, taps='nan', xo=BOTH),
     case(INNER_LDS, 'tap-inf-VALID-2seg', outer=9, inner=1, W=12, out_len=96, pad='VALID', taps='inf', xo=BOTH),
     # non-finite and -0 inputs next to both borders, finite taps
     case(INNER_LDS, 'edges-SAME', outer=9, inner=1, W=9, out_len=40, data='edges', xo=BOTH),
     case(INNER_LDS, 'edges-VALID', outer=9, inner=1, W=4, out_len=37, pad='VALID', data='edges', xo=BOTH),
     case(INNER_LDS, 'edges-tap-nan', outer=9, inner=1, W=9, out_len=40, data='edges', taps='nan', xo=BOTH)])

RUN4_CASES = (
    [case(RUN4, 'y+1', outer=8, inner=1, W=5, out_len=40, yo=1, xo=BOTH),
     case(RUN4, 'outer7', outer=7, inner=1, W=5, out_len=40, xo=BOTH)] +
    [case(RUN4, 'W%d-%s' % (W, pad), outer=8, inner=1, W=W, out_len=40, pad=pad) for W in (257, 1024) for pad in ('SAME', 'VALID')] +
    # the shapes of the fast kernel on the plain one
    [case(RUN4, 'generic-out%d' % n, outer=11, inner=1, W=5, out_len=n, generic=True) for n in (32, 36, 96)] +
    [case(RUN4, 'generic-W%d-%s' % (W, pad), outer=9, inner=1, W=W, out_len=40, pad=W - 1 if pad == 'full' else pad, generic=True)
     for W in (1, 8, 9, 256) for pad in ('SAME', 'full')] +
    [case(RUN4, 'generic-tap-inf', outer=9, inner=1, W=11, out_len=40, taps='inf', generic=True),
     case(RUN4, 'generic-edges', outer=9, inner=1, W=9, out_len=40, data='edges', generic=True)] +
    # every tail length of the run of 4
    [case(RUN4, 'tail-out%d' % n, outer=7, inner=1, W=6, out_len=n, xo=BOTH) for n in (8, 9, 10, 11, 12)] +
    [case(RUN4, 'tail-out%d-VALID-y+1' % n, outer=9, inner=1, W=6, out_len=n, pad='VALID', yo=1) for n in (9, 10, 11, 12)])

# stride / dilation: SAME padding of an axis of out_len * stride; check_strided asserts that the first window starts before the axis
# and the last one ends after it
STRIDED = [(2, 1), (3, 1), (1, 2), (1, 3), (2, 2), (3, 2), (2, 3), (3, 3)]
AXIS_CASES = (
    [case(AXIS_S, 'inner1-W1025-%s' % pad, outer=8, inner=1, W=1025, out_len=40, pad=pad) for pad in ('SAME', 'VALID')] +
    [case(AXIS_S, 'inner1-out7', outer=8, inner=1, W=5, out_len=7, xo=BOTH),
     case(AXIS_S, 'inner1-out7-VALID-y+1', outer=9, inner=1, W=4, out_len=7, pad='VALID', yo=1),
     case(AXIS_S, 'inner31-x+1', outer=2, inner=31, W=9, out_len=19, xo=(1,)),
     case(AXIS_S, 'inner31-y+1', outer=2, inner=31, W=9, out_len=19, yo=1),
     case(AXIS_S, 'inner31', outer=2, inner=31, W=8, out_len=19, pad='VALID'),
     case(AXIS_S, 'inner64-W257-x+1', outer=2, inner=64, W=257, out_len=19, xo=(1,)),
     case(AXIS_S, 'inner33-generic', outer=2, inner=33, W=9, out_len=19, generic=True),
     case(AXIS_S, 'inner1-generic-out7', outer=8, inner=1, W=5, out_len=7, generic=True),
     case(AXIS_S, 'inner5-edges', outer=3, inner=5, W=9, out_len=19, data='edges'),
     case(AXIS_S, 'inner5-tap-inf', outer=3, inner=5, W=9, out_len=19, taps='inf'),
     case(AXIS_V, 'inner32', outer=2, inner=32, W=9, out_len=19),
     case(AXIS_V, 'inner60', outer=2, inner=60, W=9, out_len=19),
     case(AXIS_V, 'inner60-VALID', outer=2, inner=60, W=8, out_len=19, pad='VALID'),
     case(AXIS_V, 'inner64-W257', outer=2, inner=64, W=257, out_len=19),
     case(AXIS_V, 'inner64-out7', outer=2, inner=64, W=5, out_len=7),
     case(AXIS_V, 'inner68-generic', outer=2, inner=68, W=9, out_len=19, generic=True),
     case(AXIS_V, 'inner8-edges', outer=3, inner=8, W=9, out_len=19, data='edges'),
     case(AXIS_V, 'inner8-tap-nan', outer=3, inner=8, W=9, out_len=19, taps='nan')] +
    [case(AXIS_S, 'inner1-stride%d-dil%d' % sd, outer=8, inner=1, W=5, out_len=13, stride=sd[0], dil=sd[1]) for sd in STRIDED] +
    [case(AXIS_S, 'inner33-stride%d-dil%d' % sd, outer=2, inner=33, W=5, out_len=13, stride=sd[0], dil=sd[1]) for sd in STRIDED] +
    [case(AXIS_V, 'inner64-stride%d-dil%d' % sd, outer=2, inner=64, W=5, out_len=13, stride=sd[0], dil=sd[1]) for sd in STRIDED])

# the rows kernels: scalar at inner >= 32 when inner % 4 != 0 or a pointer is off, vector at inner >= 64
ROWS_ARMS = ((ROWS_S, 33), (ROWS_V, 68))
ROWS_CASES = (
    [case(ROWS_S, 'inner32-x+1', outer=2, inner=32, W=9, out_len=19, xo=(1,)),
     case(ROWS_S, 'inner64-x+1', outer=2, inner=64, W=9, out_len=19, xo=(1,)),
     case(ROWS_S, 'inner64-y+1', outer=2, inner=64, W=9, out_len=19, yo=1),
     case(ROWS_S, 'inner257', outer=2, inner=257, W=9, out_len=19),           # more than one block's lanes in a row
     case(ROWS_V, 'inner64', outer=2, inner=64, W=9, out_len=19),
     case(ROWS_V, 'inner1028', outer=2, inner=1028, W=9, out_len=19)] +
    # out_len 8 / 16: whole chunks; 9 / 15: a partial last chunk
    [case(arm, 'inner%d-out%d-%s' % (inner, n, pad), outer=3, inner=inner, W=5, out_len=n, pad=pad)
     for arm, inner in ROWS_ARMS for n in (8, 9, 15, 16) for pad in ('SAME', 'VALID')] +
    [case(arm, 'inner%d-W%d-%s' % (inner, W, pad), outer=2, inner=inner, W=W, out_len=19, pad=pad)
     for arm, inner in ROWS_ARMS for W in (1, 8, 9, 256) for pad in ('SAME', 'VALID')] +
    [c for arm, inner in ROWS_ARMS for c in (
        case(arm, 'inner%d-axis9-W31' % inner, outer=2, inner=inner, W=31, A=9),
        case(arm, 'inner%d-pad8' % inner, outer=2, inner=inner, W=9, out_len=19, pad=8),
        case(arm, 'inner%d-tap-inf' % inner, outer=2, inner=inner, W=11, out_len=19, taps='inf'),
        case(arm, 'inner%d-tap-nan-VALID' % inner, outer=2, inner=inner, W=12, out_len=15, pad='VALID', taps='nan'),
        case(arm, 'inner%d-edges-SAME' % inner, outer=2, inner=inner, W=9, out_len=19, data='edges'),
        case(arm, 'inner%d-edges-VALID' % inner, outer=2, inner=inner, W=4, out_len=15, pad='VALID', data='edges'),
        case(arm, 'inner%d-edges-tap-inf' % inner, outer=2, inner=inner, W=9, out_len=19, data='edges', taps='inf'))])


@gpu
@pytest.mark.parametrize('c', INNER_LDS_CASES)
def test_conv_inner_lds(dev, monkeypatch, c):
    check_conv(dev, c, monkeypatch)


def test_inner_lds_cases_reach_every_geometry():
    """no GPU: the case list reaches 4, 8, 16 and 32 lanes per row, each with one segment and with several, and the largest LDS
    request of the kernel"""
    seen = set()
    for p in INNER_LDS_CASES:
        c = p.values[0]
        _, out_len, _ = geometry(c)
        l2, segs, span = ci_geometry(out_len, c['W'])
        seen.add((1 << l2, segs > 1))
        if c['tag'].startswith('lanes'):
            assert c['W'] == 5 and c['tag'].startswith('lanes%d-' % (1 << l2)), c['tag']
        if c['tag'].startswith('lds-max'):
            assert ((256 >> l2) * span + 256 + 8) * 4 == 76832
    assert seen >= {(lanes, many) for lanes in (4, 8, 16, 32) for many in (False, True)}, seen
    assert [ci_geometry(n, 5)[0] for n in (32, 64, 128, 256)] == [2, 3, 4, 5]
    # no geometry asks for more: 64 rows of 32 + 256 + 8 floats is the largest product of rows and span
    assert max(((256 >> l2) * ((8 << l2) + 264) + 264) * 4 for l2 in (2, 3, 4, 5)) == 76832


@gpu
@pytest.mark.parametrize('c', RUN4_CASES)
def test_conv_run4(dev, monkeypatch, c):
    check_conv(dev, c, monkeypatch)


@gpu
@pytest.mark.parametrize('c', AXIS_CASES)
def test_conv_axis(dev, monkeypatch, c):
    s, d = c.get('stride', 1), c.get('dil', 1)
    if s > 1 or d > 1:
        A, Aout, pad = geometry(c)
        assert pad > 0 and (Aout - 1) * s - pad + (c['W'] - 1) * d >= A, 'the windows must overhang the axis on both sides'
    check_conv(dev, c, monkeypatch)


@gpu
@pytest.mark.parametrize('c', ROWS_CASES)
def test_conv_rows(dev, monkeypatch, c):
    check_conv(dev, c, monkeypatch)


def _pair(tag, lo_arm, hi_arm, lo, hi):
    return pytest.param(dict(lo, arm=lo_arm, tag=tag + '-below'), dict(hi, arm=hi_arm, tag=tag + '-above'),
                        id='%s:%s|%s' % (tag, lo_arm, hi_arm))


def _two(key, a, b, **common):
    return dict(common, **{key: a}), dict(common, **{key: b})


# one case on each side of every limit of the dispatcher, with otherwise equal arguments
BOUNDARY_PAIRS = [
    _pair('inner31|32-x+1', AXIS_S, ROWS_S, *_two('inner', 31, 32, outer=2, W=9, out_len=19, xo=(1,))),
    _pair('inner60|64', AXIS_V, ROWS_V, *_two('inner', 60, 64, outer=2, W=9, out_len=19)),
    _pair('W256|257-inner1', INNER_LDS, RUN4, *_two('W', 256, 257, outer=8, inner=1, out_len=40)),
    _pair('W256|257-inner64', ROWS_V, AXIS_V, *_two('W', 256, 257, outer=2, inner=64, out_len=19)),
    _pair('W256|257-inner33', ROWS_S, AXIS_S, *_two('W', 256, 257, outer=2, inner=33, out_len=19)),
    _pair('W1024|1025', RUN4, AXIS_S, *_two('W', 1024, 1025, outer=8, inner=1, out_len=40)),
    _pair('out7|8-inner1', AXIS_S, INNER_LDS, *_two('out_len', 7, 8, outer=8, inner=1, W=5)),
    _pair('out7|8-inner1-y+1', AXIS_S, RUN4, *_two('out_len', 7, 8, outer=8, inner=1, W=5, yo=1)),
    _pair('out7|8-inner64', AXIS_V, ROWS_V, *_two('out_len', 7, 8, outer=2, inner=64, W=5)),
    _pair('out7|8-inner33', AXIS_S, ROWS_S, *_two('out_len', 7, 8, outer=2, inner=33, W=5)),
    _pair('outer7|8', RUN4, INNER_LDS, *_two('outer', 7, 8, inner=1, W=5, out_len=40)),
]


@gpu
@pytest.mark.parametrize('lo,hi', BOUNDARY_PAIRS)
def test_conv_boundary_pair(dev, monkeypatch, lo, hi):
    """both sides equal the float32 reference -- and so each other wherever they compute the same outputs"""
    assert lo['arm'] != hi['arm']
    got_lo, got_hi = check_conv(dev, lo, monkeypatch), check_conv(dev, hi, monkeypatch)
    if lo['outer'] != hi['outer']:                              # the same seed: the rows of the smaller are the first rows of the larger
        n = min(lo['outer'], hi['outer'])
        xl, kl = conv_inputs(lo, geometry(lo)[0], 0)
        xh, kh = conv_inputs(hi, geometry(hi)[0], 0)
        assert np.array_equal(xl[:n], xh[:n]) and np.array_equal(kl, kh)
        assert_bits(got_lo[:n], got_hi[:n], 'the two sides of ' + lo['tag'])


# the second grid-stride iteration of every looping kernel: just over 4096 * 256 work items, not a multiple of the grid, so the second
# iteration is partial and a wrong decomposition of the item index lands in another row.  W <= 3 keeps the reference near a second.
STRIDE_CASES = [
    # (case, work items per output element group)
    (case(AXIS_S, 'grid-stride', outer=30, inner=31, W=3, out_len=1129), lambda o, n, i: o * n * i),
    (case(AXIS_V, 'grid-stride', outer=7, inner=60, W=3, out_len=10011), lambda o, n, i: o * n * (i // 4)),
    (case(RUN4, 'grid-stride', outer=1029, inner=1, W=3, out_len=4079, yo=1), lambda o, n, i: o * ((n + 3) // 4)),
    (case(ROWS_S, 'grid-stride', outer=5, inner=33, W=3, out_len=50875), lambda o, n, i: o * ((n + 7) // 8) * i),
    (case(ROWS_V, 'grid-stride', outer=3, inner=68, W=2, out_len=164557), lambda o, n, i: o * ((n + 7) // 8) * (i // 4)),
]


@gpu
@pytest.mark.parametrize('c,items', [pytest.param(p.values[0], f, id=p.id) for p, f in STRIDE_CASES])
def test_conv_second_grid_stride_iteration(dev, monkeypatch, c, items):
    n = items(c['outer'], c['out_len'], c['inner'])
    assert GRID < n < GRID + GRID // 256 and n % GRID != 0, n    # a partial second iteration of a few blocks
    check_conv(dev, c, monkeypatch)


def status(dev, name, *args):
    """the status an entry point returns (call() raises on anything but NRT_OK)"""
    with torch.cuda.device(dev):
        return getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev))


@gpu
def test_conv_refusals_and_noops(dev):
    x, k, y = Buf(dev, 64, 0, np.ones(64, F)), Buf(dev, 3, 0, np.ones(3, F)), Buf(dev, 64)

    def st(xp=x.p, kp=k.p, yp=y.p, outer=2, A=8, inner=4, out_len=8, W=3, stride=1, dil=1, pad=1):
        return status(dev, 'nrt_conv1d_axis_f32', xp, kp, yp, outer, A, inner, out_len, W, stride, dil, pad)
    for bad in (dict(xp=None), dict(kp=None), dict(yp=None), dict(A=0), dict(W=0), dict(stride=0), dict(dil=0), dict(A=-1), dict(W=-3),
                dict(inner=0), dict(outer=-1), dict(out_len=-1)):
        assert st(**bad) == _lib.NRT_ERR_INVALID_ARG, bad
    for noop in (dict(outer=0), dict(out_len=0)):
        assert st(**noop) == _lib.NRT_OK, noop
    torch.cuda.synchronize(dev)
    assert (y.get() == F(-12345.0)).all()                       # nothing was written, guards included
    assert st() == _lib.NRT_OK                                  # and the same arguments without the refusal do write
    assert_bits(y.get(), conv1d_ref32(np.ones(64, F), np.ones(3, F), 2, 8, 4, 8, 1, 1, 1).ravel(), 'after the refusals')


# ------------------------------------------------------------------------------------------------------------------------------
# min-max: nrt_minmax_norm_f32, nrt_minmax_f32, nrt_bin_centers_f32
# ------------------------------------------------------------------------------------------------------------------------------

MM_NB = 256                         # blocks per entry of minmax_reduce1, at most


def ws_bytes(outer, inner):
    """nrt_minmax_workspace_bytes: a pair of int keys per block and entry (inner == 1), or per (outer, inner) column"""
    return max(outer, 0) * (MM_NB if inner == 1 else max(inner, 0)) * 2 * 4


def extrema(x, axis):
    """np.min / np.max with keepdims.  Where the extreme is a zero, NumPy returns whichever zero it met; the kernels order the floats
    by an integer key in which -0 < +0, so the minimum is -0 if a -0 is present and the maximum is +0 if a +0 is present."""
    mn, mx = x.min(axis, keepdims=True), x.max(axis, keepdims=True)
    neg0 = ((x == 0) & np.signbit(x)).any(axis, keepdims=True)
    pos0 = ((x == 0) & ~np.signbit(x)).any(axis, keepdims=True)
    mn = np.where(mn == 0, np.where(neg0, F(-0.0), F(0.0)), mn).astype(F)
    mx = np.where(mx == 0, np.where(pos0, F(0.0), F(-0.0)), mx).astype(F)
    return mn, mx


def minmax_ref(x):
    """x [outer, R, inner] float32 -> div_no_nan(x - min, max - min) over R, every op in float32"""
    assert x.dtype == F and not np.isnan(x).any(), 'NaN in a min-max input is out of scope'
    mn, mx = extrema(x, 1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        den = mx - mn
        y = np.where(den != 0, (x - mn) / den, F(0))
    assert y.dtype == F
    return y


def run_minmax(dev, x, xo=0, yo=0):
    outer, R, inner = x.shape
    xb, yb = Buf(dev, x.size, xo, x), Buf(dev, x.size, yo)
    nws = int(_lib.lib().nrt_minmax_workspace_bytes(outer, inner))
    assert nws == ws_bytes(outer, inner)
    ws = Bytes(dev, nws)                                        # exactly the stated size, guarded
    call(dev, 'nrt_minmax_norm_f32', xb.p, yb.p, outer, R, inner, ws.p, nws)
    ws.check()
    return yb.get(x.shape)


def check_minmax(dev, x, xo=0, yo=0, what=''):
    assert_bits(run_minmax(dev, x, xo, yo), minmax_ref(x), '%s shape %s xo %d yo %d' % (what, x.shape, xo, yo))


def columns(rng, outer, R, inner):
    """standard-normal values, every (outer, inner) column scaled and shifted into a range of its own: a column index error changes
    the extrema"""
    scale = (0.5 + rng.random((outer, 1, inner))).astype(F)
    shift = (20 * rng.standard_normal((outer, 1, inner))).astype(F)
    return (rng.standard_normal((outer, R, inner)).astype(F) * scale + shift).astype(F)


def place(x, hi_at, lo_at):
    """put a column's extremes at chosen positions of the reduced axis"""
    x = x.copy()
    mn, mx = x.min(1), x.max(1)
    x[:, hi_at, :] = mx + F(3)
    if lo_at != hi_at:
        x[:, lo_at, :] = mn - F(3)
    return x


def data_shapes(rng, outer, R, inner):
    """(name, data) of every kind of content a min-max path is run on"""
    base = columns(rng, outer, R, inner)
    body = (R // 2 // 4 * 4 + 1) % R                            # inside the 16-byte body of an aligned entry
    out = [('mixed', base),
           ('max-first-min-last', place(base, 0, R - 1)),
           ('min-first-max-last', place(base, R - 1, 0)),
           ('extremes-in-the-body', place(base, body, (body + 2) % R)),
           ('all-negative', place(-np.abs(base) - F(1), body, R - 1)),
           ('all-negative-min-first', place(-np.abs(base) - F(1), R - 1, 0)),
           ('zeros-of-both-signs', np.where(rng.random((outer, R, inner)) < 0.5, F(0.0), F(-0.0)).astype(F)),
           ('all-minus-zero', np.full((outer, R, inner), -0.0, F)),
           ('constant', np.full((outer, R, inner), 2.5, F)),
           ('constant-negative', np.full((outer, R, inner), -7.25, F)),
           ('subnormal', (rng.integers(1, 1 << 22, (outer, R, inner)) * np.where(rng.random((outer, R, inner)) < 0.5, -1, 1)
                          * 2.0 ** -149).astype(F))]
    for name, vals in (('+inf', (np.inf,)), ('-inf', (-np.inf,)), ('both-inf', (np.inf, -np.inf))):
        x = base.copy()
        for j, v in enumerate(vals):
            x[:, (body + 3 * j) % R, :] = v
        out.append((name, x))
    x = base.copy()
    x[:, R - 1, :] = np.inf                                     # in the scalar tail
    x[:, 0, :] = -np.inf
    out.append(('inf-at-the-ends', x))
    return out


@gpu
@pytest.mark.parametrize('R', [1, 3, 4, 5, 1001, 4095, 4097, 8191, 8193])
def test_minmax_inner1_lengths(dev, R):
    """minmax_reduce1 / minmax_apply1; outer = 3 with a reduce_len that is no multiple of 4: entries 1 and 2 are misaligned although
    the base is aligned, so the 16-byte body is chosen entry by entry.  Every alignment of x and y."""
    rng = np.random.default_rng(R)
    for outer in (1, 3):
        x = columns(rng, outer, R, 1)
        for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)):
            check_minmax(dev, x, xo, yo, 'inner 1')


@gpu
@pytest.mark.parametrize('outer,R,xo,yo', [(3, 1001, 0, 0), (2, 1004, 0, 0), (2, 1004, 1, 1)],
                         ids=['entries-misaligned', 'aligned', 'x+1,y+1'])
def test_minmax_inner1_data_shapes(dev, outer, R, xo, yo):
    for name, x in data_shapes(np.random.default_rng(R + xo), outer, R, 1):
        check_minmax(dev, x, xo, yo, name)


@gpu
@pytest.mark.parametrize('outer,R', [(1, MM_NB * 4096 + 4097), (16, 65536 + 5), (3, 4 * 256 * (4096 // 3) + 1001)],
                         ids=['reduce1-block-cap', 'apply1-cap-64', 'apply1-cap-4096/outer'])
def test_minmax_inner1_block_caps(dev, outer, R):
    """above 256 * 4096 elements minmax_reduce1 has its 256 blocks and every block strides further; minmax_apply1 loops above
    4 * 256 * 64 elements per entry at outer >= 16 and above 4 * 256 * (4096 / outer) below"""
    if outer == 1:
        assert -(-R // 4096) > MM_NB
    else:
        assert -(-(-(-R // 4)) // 256) > (64 if outer >= 16 else 4096 // outer)
    x = columns(np.random.default_rng(outer), outer, R, 1)
    x = place(x, R - 2, R // 2 + 1)                             # the extremes where only the last blocks / the tail look
    check_minmax(dev, x, 0, 0, 'caps')
    if outer == 1:
        check_minmax(dev, x, 1, 1, 'caps')


@gpu
@pytest.mark.parametrize('inner', [2, 3, 5, 256, 257, 1024])
def test_minmax_columns(dev, inner):
    """minmax_init / minmax_reduce / minmax_apply: extrema per (outer, inner) column by LDS atomics on the integer keys"""
    rng = np.random.default_rng(inner)
    offs = ((0, 0), (1, 0), (0, 1), (1, 1))
    n = 0
    for outer in (1, 3):
        for R in (1, 7, 3001):
            x = columns(rng, outer, R, inner)
            if R > 1:
                x = place(x, R - 1, 0)
            for xo, yo in {offs[n % 4], (0, 0)}:
                check_minmax(dev, x, xo, yo, 'columns')
            n += 1


@gpu
@pytest.mark.parametrize('outer,R,inner', [(1, 8195, 1024), (1100, 2, 1024)], ids=['reduce-block-cap', 'init-second-iteration'])
def test_minmax_columns_block_caps(dev, outer, R, inner):
    """minmax_reduce has at most 2048 blocks per entry (above 2048 * 4096 elements); minmax_init strides above 4096 * 256 columns"""
    assert -(-R * inner // 4096) > 2048 or outer * inner > GRID
    x = place(columns(np.random.default_rng(outer), outer, R, inner), R - 1, 0)
    check_minmax(dev, x, 0, 0, 'column caps')


@gpu
@pytest.mark.parametrize('outer,R,inner,xo,yo', [(3, 7, 5, 0, 0), (2, 1001, 3, 1, 1), (1, 64, 256, 0, 1)])
def test_minmax_columns_data_shapes(dev, outer, R, inner, xo, yo):
    for name, x in data_shapes(np.random.default_rng(R + inner), outer, R, inner):
        check_minmax(dev, x, xo, yo, name)


@gpu
def test_minmax_workspace(dev):
    lib = _lib.lib()
    for outer, inner in ((0, 1), (1, 1), (3, 1), (3, 5), (1, 1024)):
        assert int(lib.nrt_minmax_workspace_bytes(outer, inner)) == ws_bytes(outer, inner), (outer, inner)
    assert ws_bytes(0, 1) == 0 and ws_bytes(1, 1) == 2048 and ws_bytes(3, 5) == 120 and ws_bytes(1, 1024) == 8192
    for outer, R, inner in ((3, 9, 1), (3, 9, 5), (1, 2, 1024)):
        x = columns(np.random.default_rng(1), outer, R, inner)
        xb, yb = Buf(dev, x.size, 0, x), Buf(dev, x.size)
        nws = ws_bytes(outer, inner)
        ws = Bytes(dev, nws)
        assert status(dev, 'nrt_minmax_norm_f32', xb.p, yb.p, outer, R, inner, ws.p, nws - 1) == _lib.NRT_ERR_WORKSPACE
        assert status(dev, 'nrt_minmax_norm_f32', xb.p, yb.p, outer, R, inner, None, nws) == _lib.NRT_ERR_WORKSPACE
        torch.cuda.synchronize(dev)
        ws.check()
        assert (yb.get() == F(-12345.0)).all()                  # a refusal writes nothing
        assert status(dev, 'nrt_minmax_norm_f32', xb.p, yb.p, outer, R, inner, ws.p, nws) == _lib.NRT_OK
        ws.check()                                              # the reach of the workspace writes: none outside the stated size
        assert_bits(yb.get(x.shape), minmax_ref(x), 'exact workspace')
    one = Buf(dev, 2, 0, np.ones(2, F))
    ws = Bytes(dev, ws_bytes(1, 1))
    out = Buf(dev, 2)
    assert status(dev, 'nrt_minmax_f32', one.p, 2, out.p, ws.p, ws.n - 1) == _lib.NRT_ERR_WORKSPACE
    assert status(dev, 'nrt_bin_centers_f32', one.p, 2, 2, out.p, ws.p, ws.n - 1) == _lib.NRT_ERR_WORKSPACE
    torch.cuda.synchronize(dev)
    assert (out.get() == F(-12345.0)).all()


@gpu
def test_minmax_refusals_and_limits(dev):
    """inner > 1024 and outer > 65535 are refused before anything is launched (a one-element tensor is enough to ask); the largest
    outer that is accepted works"""
    one, out = Buf(dev, 1, 0, np.ones(1, F)), Buf(dev, 1)
    ws = Bytes(dev, 1 << 16)

    def st(outer, R, inner):
        return status(dev, 'nrt_minmax_norm_f32', one.p, out.p, outer, R, inner, ws.p, 1 << 40)
    assert st(1, 1, 1025) == _lib.NRT_ERR_UNSUPPORTED
    assert st(65536, 1, 1) == _lib.NRT_ERR_UNSUPPORTED
    assert st(1, 1, 0) == _lib.NRT_ERR_INVALID_ARG and st(-1, 1, 1) == _lib.NRT_ERR_INVALID_ARG and st(1, -1, 1) == _lib.NRT_ERR_INVALID_ARG
    assert st(0, 1, 1) == _lib.NRT_OK and st(1, 0, 1) == _lib.NRT_OK
    torch.cuda.synchronize(dev)
    ws.check()
    assert (out.get() == F(-12345.0)).all()
    # the Python wrapper raises on such a view, it does not return something else
    with pytest.raises(_lib.NeuriteAmdError, match='nrt_minmax_norm_f32'):
        ne.utils.minmax_norm(torch.zeros((1, 1, 1025), device=dev), axis=1)
    with pytest.raises(_lib.NeuriteAmdError, match='nrt_minmax_norm_f32'):
        ne.utils.minmax_norm(torch.zeros((65536, 1), device=dev), axis=1)
    rng = np.random.default_rng(2)
    check_minmax(dev, columns(rng, 65535, 2, 1), 0, 0, 'outer 65535')
    check_minmax(dev, columns(rng, 65535, 2, 2), 0, 0, 'outer 65535')
    # inner = 1024, the largest: 3 entries, unaligned
    check_minmax(dev, place(columns(rng, 3, 9, 1024), 8, 0), 1, 1, 'inner 1024')


def run_extrema(dev, x, off):
    xb, out = Buf(dev, x.size, off, x), Buf(dev, 2)
    ws = Bytes(dev, ws_bytes(1, 1))
    call(dev, 'nrt_minmax_f32', xb.p, x.size, out.p, ws.p, ws.n)
    ws.check()
    return out.get()


@gpu
@pytest.mark.parametrize('n', [1, 5, 4097, MM_NB * 4096 + 4097])
def test_minmax_f32(dev, n):
    """nrt_minmax_f32 = np.min / np.max exactly; the data shapes at the smaller sizes"""
    rng = np.random.default_rng(n)
    sets = data_shapes(rng, 1, n, 1) if n <= 4097 else [('mixed', place(columns(rng, 1, n, 1), n - 2, n // 2 + 1)),
                                                         ('all-negative', -np.abs(columns(rng, 1, n, 1)) - F(1))]
    for name, x in sets:
        mn, mx = extrema(x, 1)
        want = np.array([mn.ravel()[0], mx.ravel()[0]], F)
        assert want[0] == x.min() and want[1] == x.max()
        for off in (0, 1):
            assert_bits(run_extrema(dev, x, off), want, 'nrt_minmax_f32 %s n %d off %d' % (name, n, off))


def run_centers(dev, x, nb, off=0):
    xb, out = Buf(dev, x.size, off, x), Buf(dev, nb)
    ws = Bytes(dev, ws_bytes(1, 1))
    call(dev, 'nrt_bin_centers_f32', xb.p, x.size, nb, out.p, ws.p, ws.n)
    ws.check()
    return out.get()


NB_BINS = (1, 2, 16, 256, 257, 1000)


def bin_center_inputs():
    rng = np.random.default_rng(9)
    ends = rng.uniform(-4.9, -1.6, 1003).astype(F)              # extrema for which start + delta * (nb - 1) misses the stop by an ulp
    ends[501], ends[-1] = F(-4.969036), F(-1.5885116)
    return [rng.standard_normal(5001).astype(F), (rng.random(4097) * 3 + 100).astype(F), -np.abs(rng.standard_normal(37)).astype(F) - F(1),
            ends]


def test_bin_center_inputs_tell_the_exact_end():
    """no GPU: for at least one input and bin count start + delta * (nb - 1) is NOT max(x) in float32, so a kernel that leaves the last
    centre as computed is told from one that stores the maximum"""
    differ = 0
    for x in bin_center_inputs():
        for nb in NB_BINS[1:]:
            mn, mx = x.min(), x.max()
            delta = F((mx - mn) / F(nb - 1))
            differ += int(F(mn + F(delta * F(nb - 1))) != mx)
            c = npo.tf_linspace(mn, mx, nb)
            assert c.dtype == F and c[0] == mn and c[-1] == mx
    assert differ >= 3, differ


@gpu
@pytest.mark.parametrize('nb', NB_BINS)
def test_bin_centers(dev, nb):
    """tf.linspace(min, max, nb) bit for bit, the ends exact; 257 and 1000 make minmax_centers stride"""
    for j, x in enumerate(bin_center_inputs()):
        want = npo.tf_linspace(x.min(), x.max(), nb)
        for off in (0, 1):
            got = run_centers(dev, x, nb, off)
            assert_bits(got, want, 'bin centres nb %d input %d off %d' % (nb, j, off))
            assert got[0] == x.min() and (nb == 1 or got[-1] == x.max())
    got = run_centers(dev, np.full(333, -3.75, F), nb)
    assert (got == F(-3.75)).all()                              # a constant input: all centres equal
    big = bin_center_inputs()[0]
    big = np.tile(big, 211)[:MM_NB * 4096 + 4097].copy() if nb == 16 else None      # above the block cap of the reduction, once
    if big is not None:
        big[-2], big[len(big) // 2 + 1] = F(9.5), F(-11.25)
        assert_bits(run_centers(dev, big, nb), npo.tf_linspace(F(-11.25), F(9.5), nb), 'bin centres above the block cap')


@gpu
def test_extrema_refusals(dev):
    one, out = Buf(dev, 4, 0, np.ones(4, F)), Buf(dev, 4)
    ws = Bytes(dev, ws_bytes(1, 1))
    inv = _lib.NRT_ERR_INVALID_ARG
    assert status(dev, 'nrt_minmax_f32', None, 4, out.p, ws.p, ws.n) == inv
    assert status(dev, 'nrt_minmax_f32', one.p, 4, None, ws.p, ws.n) == inv
    assert status(dev, 'nrt_minmax_f32', one.p, 0, out.p, ws.p, ws.n) == inv
    assert status(dev, 'nrt_bin_centers_f32', None, 4, 4, out.p, ws.p, ws.n) == inv
    assert status(dev, 'nrt_bin_centers_f32', one.p, 4, 4, None, ws.p, ws.n) == inv
    assert status(dev, 'nrt_bin_centers_f32', one.p, 0, 4, out.p, ws.p, ws.n) == inv
    assert status(dev, 'nrt_bin_centers_f32', one.p, 4, 0, out.p, ws.p, ws.n) == inv
    assert status(dev, 'nrt_minmax_norm_f32', None, out.p, 1, 4, 1, ws.p, ws.n) == inv
    assert status(dev, 'nrt_minmax_norm_f32', one.p, None, 1, 4, 1, ws.p, ws.n) == inv
    torch.cuda.synchronize(dev)
    ws.check()
    assert (out.get() == F(-12345.0)).all()
