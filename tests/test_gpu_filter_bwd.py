"""
The backward kernels of the separable filter, min-max normalisation and the axis gather (csrc/filter.hip, csrc/synth.hip) through
the C ABI, on guarded buffers whose alignment is exact (tests/arm_buffers.py), against the NumPy restatements of
tests/filter_bwd_restatement.py (which tests/test_filter_bwd_cpu.py checks against torch float64 autograd without a GPU).

  dx      bit for bit against conv_dx_ref32 (the library is built with -ffp-contract=off), and within gamma_{W+1} S + ulp32 / 2 of
          conv_dx_ref64, S = sum |k| |g|: the bound of a sequential sum of W rounded products plus the rounding of the reference to
          float32 -- the forward test's bound, no measured margin.  Stride 1 runs on the forward's kernels, one case per arm (`arm_of`
          restates the dispatcher for the pass over grad_y); stride 2 and 3 run on conv1d_axis_bwd<VEC>.
  dk      within gamma_m S + ulp32 / 2 + T of conv_dk_ref64, S = sum |g| |x|, m = DK_PER_LANE = 16: a lane adds at most DK_PER_LANE
          rounded products in float32 (m roundings: one multiply and m - 1 additions that round), everything above that is float64.
          T = 2^-40 S covers the float64 stages (fewer than 2^12 additions of relative error 2^-53 each).  Two runs give the same bits.
  minmax  against minmax_bwd_ref64.  The kernel forms dx_i = fl32(g_i / r + tie terms) in float64 from float32 sums: Sg is a float64 sum
          of float32 runs of at most MB_CHAIN = 16 elements (15 rounded additions, gamma_15 sum |g|); Sgy likewise of products g y with
          y = fl(fl(x - m) / fl(M - m)) (three roundings) times g (one more): gamma_{15 + 4} sum |g y|.  So a tie of the minimum carries
          at most (gamma_19 sum |g y| + gamma_15 sum |g|) / (r n_min), a tie of the maximum gamma_19 sum |g y| / (r n_max), every element
          ulp32 / 2 of the final rounding, and 2^-40 of the magnitudes for the float64 stages.
  gather  bit for bit against gather_bwd_ref32.
"""

import numpy as np
import pytest
import torch

import filter_bwd_restatement as R
from arm_buffers import Buf, Bytes, call
from neurite_amd import _lib
from neurite_amd import utils as U

gpu = pytest.mark.gpu
F = np.float32
GRID = 4096 * 256                   # work items of one grid-stride iteration: fblocks() caps the grid at 4096 blocks of 256
DK_TB, DK_PER_LANE, DK_MAXB = 8, 16, 1024          # csrc/filter.hip
MB_CHAIN, MB_MAXB = 16, 256


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, F), np.ascontiguousarray(ref, F)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d values differ from the reference, the first at %s: got %r, reference %r'
                             % (what, int(bad.sum()), bad.size, at, got[at], ref[at]))


# ------------------------------------------------------------------------------------------------------------------------------
# dx
# ------------------------------------------------------------------------------------------------------------------------------

INNER_LDS, RUN4, AXIS_S, AXIS_V = 'conv1d_inner_lds', 'conv1d_axis_run4', 'conv1d_axis<false>', 'conv1d_axis<true>'
ROWS_S, ROWS_V = 'conv1d_axis_rows<false,8>', 'conv1d_axis_rows<true,8>'
BWD_S, BWD_V = 'conv1d_axis_bwd<false>', 'conv1d_axis_bwd<true>'


def arm_of(outer, inner, axis_len, W, stride, dil, go, xo):
    """the kernel nrt_conv1d_axis_bwd_f32 launches.  Stride 1: the dispatcher of the forward for a pass whose input is grad_y and whose
    output, of axis_len samples, is grad_x; go / xo: offsets of grad_y / grad_x from 16-byte alignment"""
    vec = inner % 4 == 0 and go == 0 and xo == 0
    if stride != 1:
        return BWD_V if vec else BWD_S
    fast = dil == 1 and W <= 256 and axis_len >= 8
    if fast and inner == 1 and outer >= 8 and xo == 0:
        return INNER_LDS
    if fast and ((vec and inner >= 64) or (not vec and inner >= 32)):
        return ROWS_V if vec else ROWS_S
    if inner == 1 and dil == 1 and axis_len >= 8 and W <= 1024:
        return RUN4
    return AXIS_V if vec else AXIS_S


def check_dx(dev, arm, outer, inner, n, W, stride=1, dil=1, padding='SAME', go=0, xo=0, seed=0):
    Aout, pad = R.geometry(n, W, stride, dil, padding)
    what = '%s outer %d inner %d n %d W %d stride %d dil %d %s go %d xo %d' % (arm, outer, inner, n, W, stride, dil, padding, go, xo)
    assert arm_of(outer, inner, n, W, stride, dil, go, xo) == arm, what
    rng = np.random.default_rng(seed)
    k = rng.standard_normal(W).astype(F)                        # mixed signs: Gaussian taps would hide order and mirror errors
    g = rng.standard_normal((outer, Aout, inner)).astype(F)
    gb, kb, xb = Buf(dev, g.size, go, g), Buf(dev, W, 0, k), Buf(dev, outer * n * inner, xo)
    call(dev, 'nrt_conv1d_axis_bwd_f32', gb.p, kb.p, xb.p, outer, n, inner, Aout, W, stride, dil, pad)
    got = xb.get((outer, n, inner))
    assert_bits(got, R.conv_dx_ref32(g, k, outer, n, inner, Aout, stride, dil, pad), what)
    worst = 0.0
    for o in range(outer):
        ref64, S = R.conv_dx_ref64(g[o], k, 1, n, inner, Aout, stride, dil, pad)
        bound = R.gamma(W + 1) * S + R.ulp32(ref64) / 2
        err = np.abs(got[o].astype(np.float64) - ref64[0])
        assert (err <= bound[0]).all(), what
        worst = max(worst, float((err / bound[0]).max()))
    print('%s: largest error / bound = %.3g' % (what, worst))


STRIDE1 = [
    # the boundary shapes of the forward's dispatch table, for the pass over grad_y
    (INNER_LDS, dict(outer=9, inner=1, n=40, W=5)),
    (INNER_LDS, dict(outer=9, inner=1, n=40, W=4, padding='VALID')),           # an even width: the mirrored padding is asymmetric
    (INNER_LDS, dict(outer=9, inner=1, n=40, W=256)),
    (RUN4, dict(outer=9, inner=1, n=40, W=257)),
    (INNER_LDS, dict(outer=9, inner=1, n=8, W=5)),
    (AXIS_S, dict(outer=9, inner=1, n=7, W=5)),
    (RUN4, dict(outer=8, inner=1, n=40, W=5, xo=1)),                           # grad_x unaligned
    (RUN4, dict(outer=7, inner=1, n=40, W=5)),
    (AXIS_S, dict(outer=2, inner=31, n=13, W=4)),
    (AXIS_V, dict(outer=2, inner=32, n=13, W=4)),
    (ROWS_S, dict(outer=2, inner=32, n=13, W=4, go=1)),                        # grad_y unaligned
    (AXIS_V, dict(outer=2, inner=60, n=13, W=7)),
    (ROWS_V, dict(outer=2, inner=64, n=13, W=7)),
    (ROWS_V, dict(outer=2, inner=64, n=21, W=19, padding='VALID')),
    (AXIS_S, dict(outer=2, inner=3, n=13, W=4, dil=2)),                        # dilation at stride 1: the plain arm
    (AXIS_V, dict(outer=2, inner=4, n=5, W=7)),                                # wider than the axis
]


@gpu
@pytest.mark.parametrize('arm,c', STRIDE1, ids=['%s-%s' % (a, '-'.join('%s%s' % kv for kv in c.items())) for a, c in STRIDE1])
def test_dx_stride1_on_the_forward_arms(dev, arm, c, monkeypatch):
    monkeypatch.delenv('NRT_CONV1D_GENERIC', raising=False)
    check_dx(dev, arm, **c)


@gpu
@pytest.mark.parametrize('padding', ['SAME', 'VALID'])
@pytest.mark.parametrize('W', [4, 7])
@pytest.mark.parametrize('inner', [3, 4])
@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('stride', [2, 3])
def test_dx_strided(dev, stride, dil, inner, W, padding):
    """13 and 20 are no multiples of the stride or one of them is; inner 4 is the float4 kernel, 3 the scalar one"""
    for n in (13, 20):
        check_dx(dev, BWD_V if inner == 4 else BWD_S, 3, inner, n, W, stride, dil, padding, seed=n)


@gpu
def test_dx_strided_unaligned_and_wide(dev):
    check_dx(dev, BWD_S, 2, 4, 13, 4, 2, 1, 'SAME', go=1)
    check_dx(dev, BWD_S, 2, 4, 13, 4, 2, 1, 'SAME', xo=1)
    check_dx(dev, BWD_S, 2, 1, 9, 19, 2, 3, 'SAME')             # wider than the axis, dilation and stride coprime
    check_dx(dev, BWD_V, 2, 8, 30, 5, 4, 2, 'SAME')             # gcd(dil, stride) = 2: taps 2 apart, odd residues receive nothing


@gpu
def test_dx_second_grid_stride_iteration(dev):
    outer, inner, n = 1, 3001, 350
    assert outer * n * inner > GRID
    check_dx(dev, BWD_S, outer, inner, n, 3, 2, 1, 'SAME')
    outer, inner, n = 1, 3000 * 4, 350
    assert outer * n * inner // 4 > GRID
    check_dx(dev, BWD_V, outer, inner, n, 3, 2, 1, 'SAME')


# ------------------------------------------------------------------------------------------------------------------------------
# dk
# ------------------------------------------------------------------------------------------------------------------------------

def dk_blocks(total):
    unit = 256 * DK_PER_LANE
    nsub = max(-(-total // unit), 1)
    per = -(-nsub // DK_MAXB)
    return -(-nsub // per), per


DK_CASES = [dict(outer=5, inner=3, n=333, W=W, stride=1) for W in (1, 8, 9, 19)] + [
    dict(outer=7, inner=1, n=700, W=19, stride=1),
    dict(outer=5, inner=3, n=333, W=9, stride=2),
    dict(outer=7, inner=1, n=701, W=4, stride=2, dil=2),
    dict(outer=2, inner=3, n=13, W=7, stride=1, padding='VALID'),
    dict(outer=1, inner=4000, n=1100, W=2, stride=1),                          # above the block cap: more than one run per block
]


@gpu
@pytest.mark.parametrize('c', DK_CASES, ids=['-'.join('%s%s' % kv for kv in c.items()) for c in DK_CASES])
def test_dk(dev, c):
    outer, inner, n, W, stride = c['outer'], c['inner'], c['n'], c['W'], c['stride']
    dil, padding = c.get('dil', 1), c.get('padding', 'SAME')
    Aout, pad = R.geometry(n, W, stride, dil, padding)
    rng = np.random.default_rng(W)
    x = rng.standard_normal((outer, n, inner)).astype(F)
    g = rng.standard_normal((outer, Aout, inner)).astype(F)
    nblocks, per = dk_blocks(outer * Aout * inner)
    assert (per > 1) == (outer * Aout * inner > DK_MAXB * 256 * DK_PER_LANE)
    need = _lib.lib().nrt_conv1d_axis_bwd_kernel_workspace_bytes(outer, Aout, inner, W)
    assert need == nblocks * (-(-W // DK_TB) * DK_TB) * 8
    xb, gb = Buf(dev, x.size, 0, x), Buf(dev, g.size, 0, g)
    runs = []
    for _ in range(2):
        kb, ws = Buf(dev, W), Bytes(dev, need)
        call(dev, 'nrt_conv1d_axis_bwd_kernel_f32', xb.p, gb.p, kb.p, outer, n, inner, Aout, W, stride, dil, pad, ws.p, need)
        ws.check()
        runs.append(kb.get())
    assert_bits(runs[0], runs[1], 'two runs')
    ref, S = R.conv_dk_ref64(x, g, W, outer, n, inner, Aout, stride, dil, pad)
    m = DK_PER_LANE                                             # the longest float32 chain: DK_PER_LANE products per lane, csrc/filter.hip
    bound = R.gamma(m) * S + R.ulp32(ref) / 2 + 2.0 ** -40 * S
    err = np.abs(runs[0].astype(np.float64) - ref)
    print('dk %s: %d blocks, largest error / bound = %.3g' % (c, nblocks, float((err / bound).max())))
    assert (err <= bound).all(), (c, err, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# minmax_norm backward
# ------------------------------------------------------------------------------------------------------------------------------

def check_minmax(dev, x, g, outer, Rn, inner, what):
    need = _lib.lib().nrt_minmax_norm_bwd_workspace_bytes(outer, Rn, inner)
    xb, gb, db, ws = Buf(dev, x.size, 0, x), Buf(dev, g.size, 0, g), Buf(dev, x.size), Bytes(dev, need)
    call(dev, 'nrt_minmax_norm_bwd_f32', xb.p, gb.p, db.p, outer, Rn, inner, ws.p, need)
    ws.check()
    got = db.get((outer, Rn, inner))
    ref, s = R.minmax_bwd_ref64(x, g, outer, Rn, inner)
    e_sgy, e_sg = R.gamma(MB_CHAIN - 1 + 4) * s['abs_gy'], R.gamma(MB_CHAIN - 1) * s['abs_g']
    tie_min, tie_max = (e_sgy + e_sg) / (s['r'] * s['nmin']), e_sgy / (s['r'] * s['nmax'])
    mag = np.abs(g.reshape(ref.shape)) / s['r'] + s['is_min'] * (s['abs_gy'] + s['abs_g']) / (s['r'] * s['nmin']) \
        + s['is_max'] * s['abs_gy'] / (s['r'] * s['nmax'])
    bound = s['is_min'] * tie_min + s['is_max'] * tie_max + R.ulp32(ref) / 2 + 2.0 ** -40 * mag
    bound = np.where(s['flat'], 0.0, bound)                     # a constant group: exact zeros
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), (what, float(err.max()))
    ties = s['is_min'] | s['is_max']
    print('minmax %s: largest error / bound at ties %.3g' % (what, float((err[ties & ~s['flat']] / bound[ties & ~s['flat']]).max(initial=0))))
    return got, s


def minmax_data(outer, Rn, inner, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((outer, Rn, inner)).astype(F), rng.standard_normal((outer, Rn, inner)).astype(F)


@gpu
@pytest.mark.parametrize('inner', [1, 3, 300])
def test_minmax_bwd_ties_and_constant_groups(dev, inner):
    """inner 1: the forward's block-pair extrema; 3: its key table; 300: two column tiles of the backward"""
    outer, Rn = 4, 1000 if inner < 300 else 37
    x, g = minmax_data(outer, Rn, inner, inner)
    c = inner - 1
    x[0, 3, c] = x[0, Rn - 1, c] = x[0, :, c].min() - 1         # a tie of the minimum, one of them the last element
    x[1, 5, 0] = x[1, 6, 0] = x[1, 20, 0] = x[1, :, 0].max() + 1 # a three-way tie of the maximum
    x[2, :, c] = -1.75                                          # a constant group
    x[3, :, 0] = np.abs(x[3, :, 0]) + F(0.5)
    x[3, 4, 0], x[3, 11, 0] = -0.0, 0.0                         # -0 ties with +0 at the minimum
    got, s = check_minmax(dev, x, g, outer, Rn, inner, 'inner %d' % inner)
    assert (got[2, :, c].view(np.uint32) == 0).all()
    assert int(s['nmin'][0, 0, c]) == 2 and int(s['nmax'][1, 0, 0]) == 3 and int(s['nmin'][3, 0, 0]) == 2


@gpu
def test_minmax_bwd_reduce_len_1(dev):
    for inner in (1, 5):
        x, g = minmax_data(3, 1, inner, 9)
        got, _ = check_minmax(dev, x, g, 3, 1, inner, 'R 1 inner %d' % inner)
        assert (got.view(np.uint32) == 0).all()


@gpu
def test_minmax_bwd_inner1_block_caps(dev):
    """256 x 4096 + 5 elements: the forward's reduce at its cap of 256 blocks, and the backward above its own cap of 256 blocks of
    256 x 16 rows (two runs of rows per block)"""
    Rn = 256 * 4096 + 5
    assert -(-Rn // (256 * 16)) > 256 and -(-Rn // (256 * MB_CHAIN)) > MB_MAXB
    x, g = minmax_data(2, Rn, 1, 1)
    x[0, Rn - 1, 0] = x[0, 7, 0] = x[0].max() + 1
    check_minmax(dev, x, g, 2, Rn, 1, 'inner-1 caps')


@gpu
def test_minmax_bwd_columns_block_cap(dev):
    """2048 x 4096 + 3 elements of 3 columns: the forward's key reduce at its cap of 2048 blocks"""
    inner = 3
    Rn = (2048 * 4096) // inner + 2
    assert -(-Rn * inner // 4096) > 2048
    x, g = minmax_data(1, Rn, inner, 2)
    x[0, Rn - 1, 2] = x[0, 0, 2] = x[0, :, 2].min() - 1
    check_minmax(dev, x, g, 1, Rn, inner, 'column caps')


# ------------------------------------------------------------------------------------------------------------------------------
# axis gather backward
# ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('inner,go', [(3, 0), (4, 0), (4, 1)], ids=['scalar', 'float4', 'inner4-unaligned'])
@pytest.mark.parametrize('mode', ['upsampled', 'downsampled', 'thick1'])
def test_gather_bwd(dev, mode, inner, go):
    outer, A = 3, 20
    down, up = U.subsample_axis_indices(A, 1.0 if mode == 'thick1' else 3.3)
    index = down if mode == 'downsampled' else down[up]
    rs = R.run_starts(index, A)
    lens = np.diff(rs)
    if mode == 'upsampled':
        assert index.size == A and lens.max() > 1 and (lens == 0).any()
    elif mode == 'downsampled':
        assert index.size < A and (lens == 0).any() and lens.max() == 1        # unread slices
    else:
        assert (index == np.arange(A)).all()
    g = np.random.default_rng(4).standard_normal((outer, index.size, inner)).astype(F)
    gb, xb = Buf(dev, g.size, go, g), Buf(dev, outer * A * inner)
    rb = torch.from_numpy(rs).to(dev)
    call(dev, 'nrt_synth_axis_gather_bwd_f32', gb.p, _lib.ptr(rb), xb.p, outer, A, index.size, inner)
    got = xb.get((outer, A, inner))
    assert_bits(got, R.gather_bwd_ref32(g, index, outer, A, inner), mode)
    assert (got[:, lens == 0].view(np.uint32) == 0).all()
