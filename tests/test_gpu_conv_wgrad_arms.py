"""
Every dispatch arm of the convolution weight gradient (csrc/conv_bwd.hip: nrt_conv3d_wgrad2_f32 / nrt_conv3d_wgrad_f32,
nrt_hyperconv3d_wgrad_f32, nrt_conv3d_wgrad_s2d_f32, nrt_upsample_sum_f32), each under an id that names the kernel instance the
dispatcher takes.  `plan` below restates the dispatcher (channel-chunk sizes from cin and cout, the LDS fallback loop, the `quads`
rule, the grid size) and every test asserts that the instance in its id is the one `plan` derives; a kernel trace of this file and
tools/arm_coverage.py --families conv_wgrad confirm it on the device (profiles/dispatch_arms/README.md).

The C ABI is called directly on guarded buffers (tests/arm_buffers.py): every pointer is 16-byte aligned, grad_weights and grad_bias
are zero-filled by the caller as the header asks, and a write outside them is caught.

Every case is checked twice on the same shapes against the float64 reference of oracle/conv_wgrad_oracle.py:

  exact     inputs from the integers -3 .. 3.  9 n < 2^24 (asserted), so every float32 product and partial sum is an integer that
            float32 holds exactly, in any order, float atomics included: the result must equal the reference BIT FOR BIT, every
            element.  One dropped, doubled or misplaced voxel, tap or channel fails it, at any volume size.
  Gaussian  standard normal inputs, |got - ref| <= (n + 1) 2^-24 A element-wise, A the sum of the absolute terms and n the number
            of terms of an element; exactly 0 where A = 0.  Each id prints its worst err / bound in a BOUND line
            (profiles/dispatch_arms/conv_wgrad_bounds.txt is the record of one run).

Each of the two runs with and without grad_bias.  (With NULL the weights of the exact check are bit-identical to those with a bias
because both equal the reference; the Gaussian weights of two launches differ by the order of the float atomics and are both held
to the bound.)  The per-entry form gets different data per entry, and a run in which one entry of x is all zeros: that entry's
slice of grad_weights must be exactly zero.

Shapes, the smallest at which the 4 x 4 x 8 voxel tile can go wrong: (1,1,1) x 1 -- one voxel, everything else halo; (4,4,8) x 1 --
exactly one tile; (5,6,9) x 2 -- two tiles per axis, the last of each partial, two entries; with dilation 2 also (3,2,5) x 1, every
extent below the halo.  With a second source the shapes are multiples of the up-sampling factor: the factor itself (one
low-resolution voxel), one tile, two partial tiles per axis x 2.
"""

import zlib

import numpy as np
import pytest
import torch

from arm_buffers import Buf, call
from neurite_amd import _lib
from oracle import conv_wgrad_oracle as cwo

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = (((1, 1, 1), 1), ((4, 4, 8), 1), ((5, 6, 9), 2))
DIL2_SHAPE = ((3, 2, 5), 1)
UP_SHAPES = {(2, 2, 2): (((2, 2, 2), 1), ((4, 4, 8), 1), ((6, 6, 10), 2)),
             (2, 1, 4): (((2, 1, 4), 1), ((4, 4, 8), 1), ((6, 5, 12), 2)),
             (3, 1, 2): (((3, 1, 2), 1), ((3, 4, 8), 1), ((6, 5, 10), 2))}
K1, K3 = (1, 1, 1), (3, 3, 3)


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatcher, restated: which instance, how many blocks
# ------------------------------------------------------------------------------------------------------------------------------

def _pow2(v):
    return v & (v - 1) == 0


def plan(pe, c0, c1, up, cout, ksize, dil, shape, B):
    """nrt_conv3d_wgrad2_f32 (pe = False) / nrt_hyperconv3d_wgrad_f32 (pe = True) with launch_wgrad_taps and launch_wgrad:
    (instance, blocks in x, tiles a block loop runs over, launches)"""
    ksize = tuple(ksize)
    cin = c0 + c1
    if not pe and cin == 1 and ksize == K3 and dil == 1 and cout % 16 == 0 and cout <= 64:
        return 'conv3d_c1_wgrad<%d>' % (cout // 16), None, None, 1
    im2col = cin == 1 and ksize == K3
    kk = K1 if im2col else ksize
    if im2col:
        cin = 27
    if not pe and ksize == K1 and c1 == 0 and c0 == 16 and cout % 16 == 0 and cout <= 64:
        return 'conv1x1_wgrad16<%d>' % (cout // 16), None, None, 1
    nb = 1 if cout <= 16 else 2
    for na in range(1 if cin <= 16 else 2 if cin <= 32 else 3, 0, -1):                 # the LDS fallback loop
        CC, CO = 16 * na, 16 * nb
        RSA, RSB = CC + 16 if CC % 32 == 0 else CC, CO + 16 if CO % 32 == 0 else CO
        h = [(k - 1) * dil for k in kk]
        lds = ((4 + h[0]) * (4 + h[1]) * (8 + h[2]) * RSA + 128 * RSB) * 4
        if lds > 160 * 1024:
            continue
        chunks = -(-cin // CC) * -(-cout // CO)
        tpv = -(-shape[0] // 4) * -(-shape[1] // 4) * -(-shape[2] // 8)
        per_cu = 1 if lds > 80 * 1024 else 2
        if pe:
            bx, tiles = min(max(-(-(256 * per_cu // chunks) // B), -(-64 // B)), tpv), tpv
        else:
            bx, tiles = min(max(256 * per_cu // chunks, 64), tpv * B), tpv * B
        quads = cout % 4 == 0 and (im2col or (cin % 4 == 0 and (not c1 or (c0 % 4 == 0 and c1 % 4 == 0 and all(_pow2(u) for u in up)))))
        km = 0 if not quads else 3 if (kk == K3 and dil == 1 and not im2col) else 1 if kk == K1 else 0
        return 'conv3d_wgrad<%d,%d,%d,7,%s>' % (na, nb, km, 'true' if pe else 'false'), bx, tiles, -(-(kk[0] * kk[1] * kk[2]) // 28)
    raise AssertionError('no chunk size fits the LDS')


def plan_fold(cin, group, shape, B):
    """nrt_conv3d_wgrad_s2d_f32 with launch_wgrad_fold (aligned pointers): (instance, blocks in x, tiles)"""
    na = 1 if cin <= 16 else 2
    chunks = -(-cin // (16 * na)) * -(-group // 16)
    tiles = -(-shape[0] // 4) * -(-shape[1] // 4) * -(-shape[2] // 8) * B
    return 'conv3d_wgrad_fold<%d>' % na, min(max(256 // chunks, 32), tiles), tiles


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, the launch, the comparison
# ------------------------------------------------------------------------------------------------------------------------------

def draw(rng, shape, kind):
    return cwo.integers(rng, shape) if kind == 'exact' else rng.standard_normal(shape).astype(F)


def launch(dev, pe, x, lo, up, g, ksize, dil, bias=True):
    """the shared or per-entry entry point on guarded, zero-filled outputs: (grad_weights, grad_bias or None) as float32 arrays"""
    B, S, c0, cout = x.shape[0], x.shape[1:4], x.shape[-1], g.shape[-1]
    c1 = 0 if lo is None else lo.shape[-1]
    lead = (B,) if pe else ()
    wshape, bshape = lead + tuple(ksize) + (c0 + c1, cout), lead + (cout,)
    xb, gb = Buf(dev, x.size, 0, x), Buf(dev, g.size, 0, g)
    lb = None if lo is None else Buf(dev, lo.size, 0, lo)
    wb, bb = Buf(dev, int(np.prod(wshape))), Buf(dev, int(np.prod(bshape))) if bias else None
    wb.t.zero_()
    if bias:
        bb.t.zero_()
    if pe:
        assert lo is None
        call(dev, 'nrt_hyperconv3d_wgrad_f32', xb.p, gb.p, wb.p, bb.p if bias else None, B, _lib.ints(S), c0, cout, _lib.ints(ksize), dil)
    else:
        call(dev, 'nrt_conv3d_wgrad2_f32', xb.p, c0, None if lb is None else lb.p, c1, None if lb is None else _lib.ints(up), gb.p, wb.p,
             bb.p if bias else None, B, _lib.ints(S), cout, _lib.ints(ksize), dil)
    return wb.get(wshape), bb.get(bshape) if bias else None


class Worst:
    """the worst err / bound of an id's Gaussian checks, printed once per id"""

    def __init__(self, arm):
        self.arm, self.w, self.b = arm, 0.0, 0.0

    def report(self):
        print('BOUND %-72s worst err / bound: grad_weights %.3g grad_bias %.3g' % (self.arm, self.w, self.b))


def compare(worst, kind, r, gw, gb, what):
    if kind == 'exact':
        cwo.exact_condition(r['n'])
        cwo.check_exact(gw, r['dW'], what + ' grad_weights')
        if gb is not None:
            cwo.check_exact(gb, r['dB'], what + ' grad_bias')
    else:
        worst.w = max(worst.w, cwo.check(gw, r['dW'], cwo.bound(r['n'], r['A_W']), what + ' grad_weights'))
        if gb is not None:
            worst.b = max(worst.b, cwo.check(gb, r['dB'], cwo.bound(r['n'], r['A_B']), what + ' grad_bias'))


def run_arm(dev, arm, pe, c0, c1, up, cout, ksize, dil, shapes, zero_entry=None):
    """both checks, with and without grad_bias, on every shape; zero_entry: ((shape, B), entry) -- one more run in which that entry
    of x is all zeros"""
    w = Worst(arm)
    runs = [(s, B, None) for s, B in shapes] + ([(zero_entry[0][0], zero_entry[0][1], zero_entry[1])] if zero_entry else [])
    for S, B, zero in runs:
        assert plan(pe, c0, c1, up, cout, ksize, dil, S, B)[0] == arm.split(' ')[0], (arm, plan(pe, c0, c1, up, cout, ksize, dil, S, B))
        for kind in ('exact', 'gauss'):
            rng = np.random.default_rng(zlib.crc32(('%s %s %d %s' % (arm, S, B, kind)).encode()))
            x, g = draw(rng, (B,) + S + (c0,), kind), draw(rng, (B,) + S + (cout,), kind)
            lo = draw(rng, (B,) + tuple(s // u for s, u in zip(S, up)) + (c1,), kind) if c1 else None
            if zero is not None:
                x[zero] = 0
            r = cwo.conv_wgrad(x, g, ksize, dil, lo, up, per_entry=pe)
            what = '%s %s x %d %s' % (arm, S, B, kind)
            gw, gb = launch(dev, pe, x, lo, up, g, ksize, dil, True)
            compare(w, kind, r, gw, gb, what)
            gw0, _ = launch(dev, pe, x, lo, up, g, ksize, dil, False)
            compare(w, kind, r, gw0, None, what + ' no bias')
            if zero is not None:
                assert not gw[zero].any() and not gw0[zero].any(), what + ': a zero entry of x has a non-zero weight gradient'
                assert np.abs(gw).sum() > 0
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# conv3d_wgrad<NA, NB, KM, 7, PE>, conv1x1_wgrad16<NB>, conv3d_c1_wgrad<NB>: one source
# ------------------------------------------------------------------------------------------------------------------------------

# (NA, NB, KM) or the streaming kernel, cin, cout, ksize, dilation
SHARED = (
    # KM = 3, every channel count a multiple of 4 that is no multiple of 16 on at least one side: partial 16-blocks in the staging
    ((1, 1, 3), 12, 8, K3, 1), ((1, 2, 3), 16, 24, K3, 1), ((2, 1, 3), 20, 16, K3, 1), ((2, 2, 3), 20, 24, K3, 1),
    ((3, 1, 3), 36, 12, K3, 1), ((3, 2, 3), 52, 40, K3, 1),                       # 52 -> 40: two chunks on both sides, the last partial
    # KM = 1: the four waves split the 32 k-steps
    ((1, 1, 1), 8, 8, K1, 1), ((1, 2, 1), 16, 20, K1, 1), ((2, 1, 1), 32, 16, K1, 1), ((2, 2, 1), 20, 24, K1, 1),
    ((3, 1, 1), 48, 16, K1, 1), ((3, 2, 1), 64, 36, K1, 1),
    ((2, 1, 1), 1, 8, K3, 1), ((2, 1, 1), 1, 16, K3, 2),                          # im2col: 27 taps as the channels of a 1x1x1 tile
    # KM = 0
    ((1, 1, 0), 8, 3, K3, 1), ((1, 2, 0), 8, 24, K3, 2), ((2, 1, 0), 20, 12, (1, 3, 3), 1), ((2, 2, 0), 18, 20, K3, 1),
    ((3, 1, 0), 40, 7, K3, 1), ((3, 2, 0), 36, 20, (3, 1, 3), 1), ((2, 1, 0), 1, 5, K3, 1),          # 1 -> 5: im2col, scalar loader
    ((1, 1, 0), 5, 6, (2, 2, 2), 1), ((1, 1, 0), 5, 6, (2, 3, 1), 1), ((1, 1, 0), 5, 6, (4, 4, 4), 1),       # 64 taps: three launches
    # the LDS fallback: the halo tile of NA = 3 and NA = 2 is over 160 KB, the cin chunk shrinks to 16
    ((1, 2, 0), 36, 20, K3, 2), ((1, 1, 0), 20, 8, (4, 4, 4), 2),
)
STREAMING = tuple(('conv1x1_wgrad16<%d>' % k, 16, 16 * k, K1, 1) for k in (1, 2, 3, 4)) + \
    tuple(('conv3d_c1_wgrad<%d>' % k, 1, 16 * k, K3, 1) for k in (1, 2, 3, 4))
PER_ENTRY = tuple(c for c in SHARED) + (((2, 1, 1), 1, 16, K3, 1), ((1, 1, 1), 16, 16, K1, 1))       # no streaming shortcut per entry


def _name(inst, pe):
    return inst if isinstance(inst, str) else 'conv3d_wgrad<%d,%d,%d,7,%s>' % (inst + ('true' if pe else 'false',))


def _ids(cases, pe):
    return ['%s %d->%d %s dil %d' % (_name(c[0], pe), c[1], c[2], 'x'.join(str(k) for k in c[3]), c[4]) for c in cases]


def _shapes(dil):
    return SHAPES + ((DIL2_SHAPE,) if dil == 2 else ())


@pytest.mark.parametrize('arm,case', list(zip(_ids(SHARED + STREAMING, False), SHARED + STREAMING)), ids=_ids(SHARED + STREAMING, False))
def test_shared(dev, arm, case):
    """nrt_conv3d_wgrad2_f32 without a second source (what nrt_conv3d_wgrad_f32 forwards to)"""
    _, cin, cout, ksize, dil = case
    run_arm(dev, arm, False, cin, 0, None, cout, ksize, dil, _shapes(dil))


@pytest.mark.parametrize('arm,case', list(zip(_ids(PER_ENTRY, True), PER_ENTRY)), ids=_ids(PER_ENTRY, True))
def test_per_entry(dev, arm, case):
    """nrt_hyperconv3d_wgrad_f32: the PE = true twin of every shared case (grid.z = entry, the entry's slice of both outputs), and a
    run of three entries whose middle one has x = 0"""
    _, cin, cout, ksize, dil = case
    run_arm(dev, arm, True, cin, 0, None, cout, ksize, dil, _shapes(dil), zero_entry=(((5, 6, 9), 3), 1))


def test_forwarding_entry_point(dev):
    """nrt_conv3d_wgrad_f32 is nrt_conv3d_wgrad2_f32 without a second source: same exact result"""
    rng = np.random.default_rng(3)
    S, B, cin, cout = (5, 6, 9), 2, 12, 8
    x, g = cwo.integers(rng, (B,) + S + (cin,)), cwo.integers(rng, (B,) + S + (cout,))
    r = cwo.conv_wgrad(x, g, K3)
    xb, gb, wb, bb = Buf(dev, x.size, 0, x), Buf(dev, g.size, 0, g), Buf(dev, 27 * cin * cout), Buf(dev, cout)
    wb.t.zero_()
    bb.t.zero_()
    call(dev, 'nrt_conv3d_wgrad_f32', xb.p, gb.p, wb.p, bb.p, B, _lib.ints(S), cin, cout, _lib.ints(K3), 1)
    cwo.check_exact(wb.get(K3 + (cin, cout)), r['dW'])
    cwo.check_exact(bb.get(), r['dB'])


# ------------------------------------------------------------------------------------------------------------------------------
# the fused loader: concat(x, UpSampling3D(x_lo)) read from its two sources
# ------------------------------------------------------------------------------------------------------------------------------

# instance, c0, c1, cout, up: the source boundary inside a 16-block (20 | 12, 8 | 12) and on one (16 | 16) on the KM = 3 staging; on
# the KM = 0 loader c1 % 4 != 0 (the scalar tail) and an up-sampling factor that is no power of two
FUSED = (((2, 1, 3), 20, 12, 16, (2, 2, 2)), ((2, 2, 3), 8, 12, 24, (2, 2, 2)), ((2, 1, 3), 16, 16, 16, (2, 1, 4)),
         ((1, 1, 0), 8, 6, 8, (2, 2, 2)), ((1, 1, 0), 8, 8, 8, (3, 1, 2)))
FUSED_IDS = ['%s %d+%d->%d up %s' % (_name(c[0], False), c[1], c[2], c[3], 'x'.join(str(u) for u in c[4])) for c in FUSED]


@pytest.mark.parametrize('arm,case', list(zip(FUSED_IDS, FUSED)), ids=FUSED_IDS)
def test_fused_loader(dev, arm, case):
    _, c0, c1, cout, up = case
    run_arm(dev, arm, False, c0, c1, up, cout, K3, 1, UP_SHAPES[up])


# ------------------------------------------------------------------------------------------------------------------------------
# the second iteration of the tile loop: more tiles than blocks
# ------------------------------------------------------------------------------------------------------------------------------

# instance, per entry, cin, cout, ksize, shape, B: channel counts whose chunk count brings the grid to its floor of 64 blocks
# (ceil(64 / B) per entry), the smallest volume of whole tiles with more tiles than that
SECOND = (((3, 2, 3), False, 96, 64, K3, (12, 12, 32), 2), ((3, 2, 1), False, 100, 68, K1, (12, 12, 32), 2),
          ((3, 2, 0), False, 98, 66, (1, 3, 3), (12, 12, 32), 2), ((3, 2, 3), True, 96, 64, K3, (12, 12, 32), 2))
SECOND_IDS = ['%s %d->%d second-tile' % (_name(c[0], c[1]), c[2], c[3]) for c in SECOND]


@pytest.mark.parametrize('arm,case', list(zip(SECOND_IDS, SECOND)), ids=SECOND_IDS)
def test_second_tile_iteration(dev, arm, case):
    """`for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)` runs twice in the first blocks: the accumulators carry over, the
    LDS tiles are restaged behind the barrier.  The exact check is the one that matters; the Gaussian bound is loose at this n."""
    _, pe, cin, cout, ksize, S, B = case
    _, bx, tiles, _ = plan(pe, cin, 0, None, cout, ksize, 1, S, B)
    assert bx == -(-64 // (B if pe else 1)) and bx < tiles <= 2 * bx, (bx, tiles)
    run_arm(dev, arm, pe, cin, 0, None, cout, ksize, 1, ((S, B),))


# ------------------------------------------------------------------------------------------------------------------------------
# conv3d_wgrad_fold<1|2>: nrt_conv3d_wgrad_s2d_f32
# ------------------------------------------------------------------------------------------------------------------------------

def launch_fold(dev, lo, s2d, group, expect=_lib.NRT_OK):
    B, S, cin = lo.shape[0], lo.shape[1:4], lo.shape[-1]
    lb, gb, wb = Buf(dev, lo.size, 0, lo), Buf(dev, s2d.size, 0, s2d), Buf(dev, 64 * cin * group)
    wb.t.zero_()
    args = (lb.p, gb.p, wb.p, B, _lib.ints(S), cin, group)
    if expect != _lib.NRT_OK:
        with torch.cuda.device(dev):
            assert _lib.lib().nrt_conv3d_wgrad_s2d_f32(*args, _lib.stream_ptr(dev)) == expect
    else:
        call(dev, 'nrt_conv3d_wgrad_s2d_f32', *args)
    return wb.get((8, 8, cin, group))


def run_fold(dev, arm, cin, group, shapes):
    w = Worst(arm)
    for S, B in shapes:
        assert plan_fold(cin, group, S, B)[0] == arm.split(' ')[0]
        for kind in ('exact', 'gauss'):
            rng = np.random.default_rng(zlib.crc32(('%s %s %d %s' % (arm, S, B, kind)).encode()))
            lo = draw(rng, (B,) + S + (cin,), kind)
            s2d = cwo.space_to_depth2(draw(rng, (B,) + tuple(2 * s for s in S) + (group,), kind))      # built in numpy
            r = cwo.fold_wgrad(lo, s2d, group)
            r['dB'] = r['A_B'] = None
            compare(w, kind, r, launch_fold(dev, lo, s2d, group), None, '%s %s x %d %s' % (arm, S, B, kind))
    print('BOUND %-72s worst err / bound: grad_folded %.3g' % (arm, w.w))


FOLD = ((1, 4, 4), (1, 16, 16), (2, 20, 12), (2, 36, 32))          # 36 -> 32: two cin chunks and two cout chunks, the last cin chunk partial
FOLD_IDS = ['conv3d_wgrad_fold<%d> %d->%d' % c for c in FOLD]


@pytest.mark.parametrize('arm,case', list(zip(FOLD_IDS, FOLD)), ids=FOLD_IDS)
def test_fold(dev, arm, case):
    """grad_folded [8 groups][8 taps][cin][group] = sum_q x_lo[q + p + t - 1] (x) grad_pre_s2d[q][P], on low-resolution shapes"""
    run_fold(dev, arm, case[1], case[2], SHAPES)


def test_fold_second_tile_iteration(dev):
    """id conv3d_wgrad_fold<2> 100->32 second-tile: 4 x 2 chunks bring the grid to its floor of 32 blocks, (12, 12, 16) x 2 has 36 tiles"""
    S, B, cin, group = (12, 12, 16), 2, 100, 32
    _, bx, tiles = plan_fold(cin, group, S, B)
    assert bx == 32 and bx < tiles <= 2 * bx
    run_fold(dev, 'conv3d_wgrad_fold<2> 100->32 second-tile', cin, group, ((S, B),))


def test_fold_refuses_a_group_over_32(dev):
    """one cout chunk pair per parity group: group = 36 is NRT_ERR_UNSUPPORTED and nothing is written"""
    rng = np.random.default_rng(36)
    lo, s2d = cwo.integers(rng, (1, 4, 4, 8, 16)), cwo.integers(rng, (1, 4, 4, 8, 8 * 36))
    assert not launch_fold(dev, lo, s2d, 36, expect=_lib.NRT_ERR_UNSUPPORTED).any()


# ------------------------------------------------------------------------------------------------------------------------------
# upsample_sum: nrt_upsample_sum_f32
# ------------------------------------------------------------------------------------------------------------------------------

UPSUM = (((2, 2, 2), 12, 4, 5), ((2, 2, 2), 5, 0, 5), ((3, 1, 2), 12, 4, 5), ((3, 1, 2), 5, 0, 5))        # up, grad_channels, offset, channels
UPSUM_IDS = ['upsample_sum up %s channels %d+%d of %d' % ('x'.join(str(u) for u in c[0]), c[2], c[3], c[1]) for c in UPSUM]


@pytest.mark.parametrize('arm,case', list(zip(UPSUM_IDS, UPSUM)), ids=UPSUM_IDS)
def test_upsample_sum(dev, arm, case):
    """grad_lo[v] = the sum of a channel slice over the up^3 block: a slice inside the tensor and the whole tensor, 150 elements (less
    than one block) and 1350 (six blocks, the last partial).  The output is not zero-filled: the kernel writes every element."""
    up, gc, off, ch = case
    worst = 0.0
    for S, B in (((3, 2, 5), 2), ((5, 6, 9), 2)):
        assert (S == (3, 2, 5)) == (int(np.prod(S)) * ch < 256)
        for kind in ('exact', 'gauss'):
            rng = np.random.default_rng(zlib.crc32(('%s %s %s' % (arm, S, kind)).encode()))
            gu = draw(rng, (B,) + tuple(s * u for s, u in zip(S, up)) + (gc,), kind)
            r = cwo.upsample_sum(gu, off, ch, up)
            gb, ob = Buf(dev, gu.size, 0, gu), Buf(dev, B * int(np.prod(S)) * ch)
            call(dev, 'nrt_upsample_sum_f32', gb.p, gc, off, ob.p, ch, B, _lib.ints(S), _lib.ints(up))
            got = ob.get((B,) + S + (ch,))
            if kind == 'exact':
                cwo.exact_condition(r['n'])
                cwo.check_exact(got, r['grad_lo'], arm)
            else:
                worst = max(worst, cwo.check(got, r['grad_lo'], cwo.bound(r['n'], r['A']), arm))
    print('BOUND %-72s worst err / bound: grad_lo %.3g' % (arm, worst))
