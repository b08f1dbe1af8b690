"""
Every dispatch arm of the U-Net head and glue kernels (csrc/conv.hip, csrc/conv_bwd.hip), each once, at the smallest voxel counts
at which its indexing can still go wrong.  The host-side dispatchers pick one template instance from the channel count and the
pointer alignment; a kernel can be wrong at one instance only, so one pytest id is one arm (the id names the kernel the dispatcher
takes; profiles/dispatch_arms/README.md says how a kernel trace of this file and tools/arm_coverage.py confirm that).

Each case compares the HIP result with a float64 numpy / torch evaluation of the same formula, asserts the output shape, and --
where the test owns the output buffer -- that the floats on both sides of the output keep their fill value.

Tolerances are the ones the suite already applies to the same kernels:
  1x1 head, channel softmax, element-wise forward    close() of tests/test_gpu_unet.py (1e-5, relative + of the largest value)
  gradients                                          2e-4 of the gradient scale (tests/test_gpu_conv_backward.py)
  softmax backward                                   1e-5 of the scale (test_small_layer_backward)
  pooling forward / backward, channel_axpby, act_bwd for none / relu:  bit for bit
"""

import numpy as np
import pytest
import torch

from arm_buffers import Buf, call
from neurite_amd import _lib
from neurite_amd import models as M
from oracle import torch_unet_oracle as tuo

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 2e-4                  # gradients, of the gradient scale


# ------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------------------------------------

def N(t):
    return t.detach().cpu().numpy()


def G(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_() if grad else t


def close(got, ref, tol=1e-5, what=''):
    """close() of tests/test_gpu_unet.py"""
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))
    print('%s: max err / max |ref| = %.3g' % (what, err))
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * max(1e-30, np.abs(ref).max()), err_msg=what)


def close_grad(got, want, what='', tol=TOL):
    """close() of tests/test_gpu_conv_backward.py"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    print('%s: max err / scale = %.3g' % (what, err))
    assert err < tol, '%s: max err / scale = %.3g' % (what, err)


def softmax64(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------
# the 1x1 head: nrt_conv1x1_softmax_f32
# ------------------------------------------------------------------------------------------------------------------------------

HEAD_MODES = (('linear', 0, 0), ('elu', 0, 1), ('relu', 0, 2), ('softmax', 1, 0))
# 1, 17, 420 = 2*5*6*7: the last 16-voxel tile of conv1x1_rows is partial and its clamped load index is used; 257 = 4 * 64 + 1: a
# second block with one live voxel
HEAD_NVOX = (1, 17, 420, 257)
HEAD_ARMS = (
    [('conv1x1_rows<%d,%d>' % (co // 4, ci), ci, co) for ci in (16, 32) for co in (16, 32, 64)] +
    # cin outside 16 / 32: the rows dispatcher declines and conv1x1_vec<cout / 4> runs; (64, 16) is the input gradient of a 64-label head
    [('conv1x1_vec<1>', 8, 4), ('conv1x1_vec<2>', 8, 8), ('conv1x1_vec<4>', 20, 16), ('conv1x1_vec<4>-dgrad64', 64, 16),
     ('conv1x1_vec<8>', 12, 32), ('conv1x1_vec<16>', 8, 64)] +
    # cout no multiple of 4: one thread per voxel
    [('conv1x1_softmax<16>', 7, 5), ('conv1x1_softmax<32>', 7, 20), ('conv1x1_softmax<64>', 7, 50)])


def head_inputs(rng, nvox, cin, cout):
    x = rng.standard_normal((nvox, cin)).astype(F)
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(F)
    b = rng.standard_normal(cout).astype(F)
    return x, w, b


def head_ref(x, w, b, mode):
    lin = x.astype(np.float64) @ w.astype(np.float64) + (0.0 if b is None else b.astype(np.float64))
    if mode == 'elu':
        return np.where(lin > 0, lin, np.exp(np.minimum(lin, 0)) - 1)
    if mode == 'relu':
        return np.maximum(lin, 0)
    if mode == 'softmax':
        return softmax64(lin)
    return lin


def run_head(dev, x, w, b, softmax, act, xo=0, yo=0, wo=0, bo=0):
    nvox, cin = x.shape
    cout = w.shape[1]
    xb, wb = Buf(dev, x.size, xo, x), Buf(dev, w.size, wo, w)
    bb = None if b is None else Buf(dev, cout, bo, b)
    yb = Buf(dev, nvox * cout, yo)
    call(dev, 'nrt_conv1x1_softmax_f32', xb.p, wb.p, None if bb is None else bb.p, yb.p, nvox, cin, cout, softmax, act)
    return yb.get((nvox, cout))


@pytest.mark.parametrize('arm,cin,cout', HEAD_ARMS, ids=[a[0] for a in HEAD_ARMS])
def test_head_arm(dev, arm, cin, cout):
    rng = np.random.default_rng(cin * 100 + cout)
    for nvox in HEAD_NVOX:
        x, w, b = head_inputs(rng, nvox, cin, cout)
        for mode, softmax, act in HEAD_MODES:
            got = run_head(dev, x, w, b, softmax, act)
            close(got, head_ref(x, w, b, mode), what='%s nvox %d %s' % (arm, nvox, mode))
            if softmax:
                np.testing.assert_allclose(got.sum(-1), 1.0, rtol=1e-5)
    if arm.startswith('conv1x1_rows'):                       # the rows kernel reads the bias as one float4 per lane, or not at all
        x, w, b = head_inputs(rng, 420, cin, cout)
        for mode, softmax, act in HEAD_MODES:
            close(run_head(dev, x, w, None, softmax, act), head_ref(x, w, None, mode), what='%s no bias %s' % (arm, mode))


HEAD_FALLBACKS = [('x+1->conv1x1_vec<8>', dict(xo=1)), ('w+1->conv1x1_vec<8>', dict(wo=1)), ('bias+1->conv1x1_vec<8>', dict(bo=1)),
                  ('y+1->conv1x1_softmax<32>', dict(yo=1)), ('x+1,y+1->conv1x1_softmax<32>', dict(xo=1, yo=1))]


@pytest.mark.parametrize('arm,offs', HEAD_FALLBACKS, ids=[a[0] for a in HEAD_FALLBACKS])
def test_head_alignment_fallback(dev, arm, offs):
    """16 -> 32 would take conv1x1_rows<8,16>; a tensor that starts one float into its storage must take the arm that does no
    16-byte access to it, and still match.  (The Python wrapper hands over whatever address the tensor has: a view is not realigned.)"""
    rng = np.random.default_rng(7)
    for nvox in (17, 420):
        x, w, b = head_inputs(rng, nvox, 16, 32)
        for mode, softmax, act in HEAD_MODES:
            close(run_head(dev, x, w, b, softmax, act, **offs), head_ref(x, w, b, mode), what='%s nvox %d %s' % (arm, nvox, mode))


# the smallest outputs past the block caps of the two grid-stride loops: conv1x1_rows launches at most 1280 blocks of 4 waves x 64
# voxels, conv1x1_vec<1> at most 8192 blocks of 256 voxels
HEAD_STRIDE = [('conv1x1_rows<4,16>', 16, 16, 1280 * 4 * 64 + 100), ('conv1x1_vec<1>', 4, 4, 8192 * 256 + 100)]


@pytest.mark.parametrize('arm,cin,cout,nvox', HEAD_STRIDE, ids=[a[0] for a in HEAD_STRIDE])
def test_head_second_grid_stride_iteration(dev, arm, cin, cout, nvox):
    rng = np.random.default_rng(11)
    x, w, b = head_inputs(rng, nvox, cin, cout)
    for mode, softmax, act in (HEAD_MODES[1], HEAD_MODES[3]):
        close(run_head(dev, x, w, b, softmax, act), head_ref(x, w, b, mode), what='%s nvox %d %s' % (arm, nvox, mode))


# ------------------------------------------------------------------------------------------------------------------------------
# channel softmax, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------

def softmax_arm(kernel, C):
    return '%s_vec<%d>' % (kernel, C // 4) if C in (4, 8, 16, 32, 64) else '%s-C%d' % (kernel, C)


def softmax_case(rng, nvox, C):
    z = (rng.standard_normal((nvox, C)) * 4).astype(F)
    g = rng.standard_normal((nvox, C)).astype(F)
    return z, g, softmax64(z.astype(np.float64))


def run_softmax(dev, z, off=0):
    nvox, C = z.shape
    zb, yb = Buf(dev, z.size, off, z), Buf(dev, z.size, off)
    call(dev, 'nrt_softmax_lastdim_f32', zb.p, yb.p, nvox, C)
    return yb.get((nvox, C))


def run_softmax_bwd(dev, y, g, off=0):
    nvox, C = y.shape
    yb, gb, db = Buf(dev, y.size, off, y), Buf(dev, y.size, off, g), Buf(dev, y.size, off)
    call(dev, 'nrt_softmax_bwd_f32', yb.p, gb.p, db.p, nvox, C)
    return db.get((nvox, C))


def softmax_bwd_ref(y, g):
    """the analytic gradient of softmax through its OUTPUT, which is what the kernel is given: dz = y (g - sum_c g_c y_c)"""
    y, g = y.astype(np.float64), g.astype(np.float64)
    return y * (g - (g * y).sum(-1, keepdims=True))


SOFTMAX_C = (4, 8, 16, 32, 64, 5, 33)


@pytest.mark.parametrize('C', SOFTMAX_C, ids=[softmax_arm('softmax_lastdim', C) for C in SOFTMAX_C])
def test_softmax_forward_arm(dev, C):
    rng = np.random.default_rng(C)
    for nvox in (1, 420):
        z, _, want = softmax_case(rng, nvox, C)
        close(run_softmax(dev, z), want, what='softmax C %d nvox %d' % (C, nvox))


@pytest.mark.parametrize('C', SOFTMAX_C, ids=[softmax_arm('softmax_bwd', C) for C in SOFTMAX_C])
def test_softmax_backward_arm(dev, C):
    rng = np.random.default_rng(100 + C)
    for nvox in (1, 420):
        z, g, y64 = softmax_case(rng, nvox, C)
        y = y64.astype(F)
        close_grad(run_softmax_bwd(dev, y, g), softmax_bwd_ref(y, g), 'softmax bwd C %d nvox %d' % (C, nvox), 1e-5)


def test_softmax_misaligned_takes_the_scalar_kernels(dev):
    rng = np.random.default_rng(5)
    z, g, y64 = softmax_case(rng, 420, 32)
    close(run_softmax(dev, z, off=1), y64, what='softmax_lastdim, C 32 one float off')
    y = y64.astype(F)
    close_grad(run_softmax_bwd(dev, y, g, off=1), softmax_bwd_ref(y, g), 'softmax_bwd, C 32 one float off', 1e-5)


def test_softmax_second_block_range_iteration(dev):
    """C = 64 (16 lanes per voxel, 16 voxels per block) at 4096 * 16 + 7 voxels: one more than the block cap covers in one pass, so
    niter = 2 in softmax_bwd_vec<16> (a block's contiguous range) and in softmax_lastdim_vec<16> (grid stride)"""
    rng = np.random.default_rng(6)
    z, g, y64 = softmax_case(rng, 4096 * 16 + 7, 64)
    close(run_softmax(dev, z), y64, what='softmax_lastdim_vec<16> niter 2')
    y = y64.astype(F)
    close_grad(run_softmax_bwd(dev, y, g), softmax_bwd_ref(y, g), 'softmax_bwd_vec<16> niter 2', 1e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradients: the likelihood layer (conv1x1_wgrad16<NB>) and the single-channel first layer (conv3d_c1_wgrad<NB>)
# ------------------------------------------------------------------------------------------------------------------------------

def conv_case(rng, dev, cin, cout, ks, dil, act, B, S):
    conv = M._Conv('c', cin, cout, ks, dilation=dil, padding='same', activation=act).to(dev)
    kern = (rng.standard_normal(tuple(ks) + (cin, cout)) * 0.2).astype(F)
    bias = (rng.standard_normal(cout) * 0.1).astype(F)
    with torch.no_grad():
        conv.kernel.copy_(G(kern, dev)); conv.bias.copy_(G(bias, dev))
    x = rng.standard_normal((B,) + tuple(S) + (cin,)).astype(F)
    return conv, kern, bias, x


def autograd_vs_oracle(rng, dev, cin, cout, ks, act, B, S, grad_x, what):
    conv, kern, bias, x = conv_case(rng, dev, cin, cout, ks, 1, act, B, S)
    w = rng.standard_normal((B,) + tuple(S) + (cout,)).astype(F)
    xg = G(x, dev, grad_x)
    y = conv(xg)
    assert tuple(y.shape) == (B,) + tuple(S) + (cout,)
    (y * G(w, dev)).sum().backward()
    xo = torch.from_numpy(x).double().requires_grad_()
    ko = torch.from_numpy(kern).double().requires_grad_()
    bo = torch.from_numpy(bias).double().requires_grad_()
    yo = tuo.conv3d_same(xo, ko, bo, 1, act)
    (yo * torch.from_numpy(w).double()).sum().backward()
    close_grad(N(y), yo.detach().numpy(), what + ' forward', 1e-4)
    assert tuple(conv.kernel.grad.shape) == tuple(ks) + (cin, cout) and tuple(conv.bias.grad.shape) == (cout,)
    close_grad(N(conv.kernel.grad), ko.grad.numpy(), what + ' grad_kernel')
    close_grad(N(conv.bias.grad), bo.grad.numpy(), what + ' grad_bias')
    if grad_x:
        close_grad(N(xg.grad), xo.grad.numpy(), what + ' grad_x')


def wgrad_without_bias(rng, dev, cin, cout, ks, B, S, what):
    """nrt_conv3d_wgrad2_f32 with grad_bias = NULL (the kernels skip the all-ones MFMA), into a guarded buffer"""
    x = rng.standard_normal((B,) + tuple(S) + (cin,)).astype(F)
    dz = rng.standard_normal((B,) + tuple(S) + (cout,)).astype(F)
    nw = int(np.prod(ks)) * cin * cout
    xb, zb = Buf(dev, x.size, 0, x), Buf(dev, dz.size, 0, dz)
    dw = Buf(dev, nw, 0, np.zeros(nw, F))
    call(dev, 'nrt_conv3d_wgrad2_f32', xb.p, cin, None, 0, None, zb.p, dw.p, None, B, _lib.ints(S), cout, _lib.ints(ks), 1)
    ko = torch.zeros(tuple(ks) + (cin, cout), dtype=torch.float64).requires_grad_()
    (tuo.conv3d_same(torch.from_numpy(x).double(), ko, None, 1, None) * torch.from_numpy(dz).double()).sum().backward()
    close_grad(dw.get(tuple(ks) + (cin, cout)), ko.grad.numpy(), what + ' grad_kernel without grad_bias')


# B * X * Y * Z = 1: fewer voxels than one wave's span; 420; 2 * 9 * 10 * 17 = 3060: ragged against the 128-voxel block unit
LIKELIHOOD_SHAPES = ((1, (1, 1, 1)), (2, (5, 6, 7)), (2, (9, 10, 17)))


@pytest.mark.parametrize('cout', (16, 32, 48, 64), ids=['conv1x1_wgrad16<%d>' % nb for nb in (1, 2, 3, 4)])
def test_likelihood_weight_gradient_arm(dev, cout):
    """_Conv 1x1x1, 16 -> cout.  The input gradient of the same layer is conv1x1_rows<4,16> (cout 16), conv1x1_rows<4,32> (cout 32,
    the benchmarked model) and conv1x1_vec<4> (48, 64)."""
    rng = np.random.default_rng(cout)
    for B, S in LIKELIHOOD_SHAPES:
        what = '16->%d %s x %d' % (cout, S, B)
        autograd_vs_oracle(rng, dev, 16, cout, (1, 1, 1), None, B, S, True, what)
        wgrad_without_bias(rng, dev, 16, cout, (1, 1, 1), B, S, what)


# B * X * Y = 35 rows (no multiple of the 4 rows a block takes); Z = 10: one partial z0 pass, 33 and 70: two and three z0 passes of
# 32 voxels and a Z that is no multiple of 4; B = 2, (3, 2, 33): 12 rows, three blocks of 4
C1_WGRAD_SHAPES = ((1, (5, 7, 10)), (1, (5, 7, 33)), (1, (5, 7, 70)), (2, (3, 2, 33)))


@pytest.mark.parametrize('cout', (16, 32, 48, 64), ids=['conv3d_c1_wgrad<%d>' % nb for nb in (1, 2, 3, 4)])
def test_first_layer_weight_gradient_arm(dev, cout):
    rng = np.random.default_rng(200 + cout)
    for B, S in C1_WGRAD_SHAPES:
        what = '1->%d %s x %d' % (cout, S, B)
        autograd_vs_oracle(rng, dev, 1, cout, (3, 3, 3), 'elu', B, S, False, what)
        wgrad_without_bias(rng, dev, 1, cout, (3, 3, 3), B, S, what)


# ------------------------------------------------------------------------------------------------------------------------------
# the single-channel first layer, forward: conv3d_c1_mfma<cout / 16> (3x3x3, dilation 1) and conv3d_c1_vec<cout / 4> (the rest)
# ------------------------------------------------------------------------------------------------------------------------------

C1_FORWARD = (
    [('conv3d_c1_mfma<%d>' % (co // 16), co, (3, 3, 3), 1, act) for co, act in ((16, 'elu'), (32, None), (48, 'relu'), (64, 'elu'))] +
    [('conv3d_c1_vec<1>', 4, (3, 3, 3), 1, 'elu'), ('conv3d_c1_vec<2>', 8, (3, 3, 3), 1, None), ('conv3d_c1_vec<4>', 16, (3, 3, 3), 2, 'relu'),
     ('conv3d_c1_vec<8>', 32, (1, 3, 3), 1, 'elu'), ('conv3d_c1_vec<16>', 64, (3, 3, 3), 2, 'elu')])


@pytest.mark.parametrize('arm,cout,ks,dil,act', C1_FORWARD, ids=[a[0] for a in C1_FORWARD])
def test_first_layer_forward_arm(dev, arm, cout, ks, dil, act):
    """(5, 7, 19): two 4-voxel tiles in x and y and two 16-voxel tiles in z, the last of each partial; (1, 1, 1): halo only.
    Tolerance: a float32 dot product of 27 terms plus the bias is within 28 * 2^-24 of the sum of its absolute terms, the hardware
    exponential of the elu epilogue within 2e-6 -- both below close()'s 1e-5 of the largest output."""
    rng = np.random.default_rng(cout + dil)
    for B, S in ((2, (5, 7, 19)), (1, (1, 1, 1))):
        conv, kern, bias, x = conv_case(rng, dev, 1, cout, ks, dil, act, B, S)
        with torch.no_grad():
            y = conv(G(x, dev))
        assert tuple(y.shape) == (B,) + S + (cout,)
        want = tuo.conv3d_same(torch.from_numpy(x).double(), torch.from_numpy(kern).double(), torch.from_numpy(bias).double(), dil, act)
        close(N(y), want.numpy(), what='%s %s x %d' % (arm, S, B))


# ------------------------------------------------------------------------------------------------------------------------------
# max pooling, forward and backward, with ties
# ------------------------------------------------------------------------------------------------------------------------------

def pool_ref(x, g, pool, same):
    """explicit loop: the window's maximum and the gradient sent to its FIRST maximum in x, y, z scan order (csrc/conv_bwd.hip:
    maxpool_bwd); voxels outside every window ('valid', ragged) get zero"""
    B, X, Y, Z, C = x.shape
    O = [(s + p - 1) // p if same else s // p for s, p in zip((X, Y, Z), pool)]
    x = x.astype(np.float64)
    y = np.zeros([B] + O + [C], np.float64)
    dx = np.zeros(x.shape, np.float64)
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
    for ox in range(O[0]):
        for oy in range(O[1]):
            for oz in range(O[2]):
                best = np.full((B, C), -np.inf)
                arg = np.full((3, B, C), -1)
                for i in range(pool[0]):
                    for j in range(pool[1]):
                        for k in range(pool[2]):
                            xx, yy, zz = ox * pool[0] + i, oy * pool[1] + j, oz * pool[2] + k
                            if xx >= X or yy >= Y or zz >= Z:
                                continue
                            v = x[:, xx, yy, zz, :]
                            take = (arg[0] < 0) | (v > best)
                            best = np.where(take, v, best)
                            arg = np.where(take[None], np.array([xx, yy, zz]).reshape(3, 1, 1), arg)
                y[:, ox, oy, oz, :] = best
                dx[bi, arg[0], arg[1], arg[2], ci] = g[:, ox, oy, oz, :]
    return y, dx


POOL_CASES = [(pool, pad, kind) for pool in ((2, 2, 2), (3, 1, 2)) for pad in ('same', 'valid') for kind in ('relu', 'three-values')]


@pytest.mark.parametrize('pool,padding,kind', POOL_CASES, ids=['%s-%s-%s' % ('x'.join(map(str, p)), pad, k) for p, pad, k in POOL_CASES])
def test_maxpool_backward_with_ties(dev, pool, padding, kind):
    """After relu, zeros tie in most windows, and the rule for ties decides where the gradient goes.  The kernel documents "the first
    maximum in x, y, z scan order", and that is the reference here.  Keras has no rule of its own (MaxPooling3D hands over to
    tf.nn.max_pool3d); TensorFlow's gradient depends on the device: its GPU kernel (cuDNN / MIOpen) gives a window's gradient to one
    maximum, its CPU kernel (MaxPooling3dGradOp) to every element that equals the maximum.  The documented rule is the GPU one, and it
    keeps the sum of the gradient.  oracle/torch_unet_oracle.maxpool_same (torch CPU max_pool3d) breaks ties the same way -- first
    maximum in scan order -- which the 'same' cases assert too."""
    rng = np.random.default_rng(sum(pool))
    S, C, B = (7, 5, 9), 3, 2                           # no extent divisible by its pool size
    if kind == 'relu':
        x = np.maximum(rng.standard_normal((B,) + S + (C,)), 0).astype(F)
    else:
        x = rng.integers(0, 3, (B,) + S + (C,)).astype(F) - 1
    same = padding == 'same'
    O = [(s + p - 1) // p if same else s // p for s, p in zip(S, pool)]
    g = rng.standard_normal([B] + O + [C]).astype(F)
    want_y, want_dx = pool_ref(x, g, pool, same)
    got_y = M._maxpool(G(x, dev), pool, padding)
    assert tuple(got_y.shape) == tuple(want_y.shape)
    assert np.array_equal(N(got_y), want_y.astype(F))
    xb, gb, db = Buf(dev, x.size, 0, x), Buf(dev, g.size, 0, g), Buf(dev, x.size)
    call(dev, 'nrt_maxpool3d_bwd_f32', xb.p, gb.p, db.p, B, _lib.ints(S), C, _lib.ints(pool), int(same))
    got = db.get(x.shape)
    assert np.array_equal(got, want_dx.astype(F)), '%d of %d gradient entries differ' % ((got != want_dx.astype(F)).sum(), got.size)
    if same:
        xo = torch.from_numpy(x).double().requires_grad_()
        (tuo.maxpool_same(xo, pool) * torch.from_numpy(g).double()).sum().backward()
        assert np.array_equal(xo.grad.numpy(), want_dx)


# ------------------------------------------------------------------------------------------------------------------------------
# element-wise: nrt_add_act_affine_f32 (add_act_affine_v4 / add_act_affine) and nrt_act_bwd_f32 (act_bwd / act_bwd_tail)
# ------------------------------------------------------------------------------------------------------------------------------

ACT_NAMES = {v: k for k, v in M._ACTS.items() if k is not None}          # id -> Keras name, 0 .. ACT_LAST
ACT_LAST = 10


def ew_ref(a, b, sc, sh, act, mul):
    v = torch.from_numpy(a).double()
    if mul:
        v = tuo.keras_activation(v, ACT_NAMES[act]) * torch.from_numpy(b).double()
    else:
        if b is not None:
            v = v + torch.from_numpy(b).double()
        v = tuo.keras_activation(v, ACT_NAMES[act])
    if sc is not None:
        v = v * torch.from_numpy(sc).double() + torch.from_numpy(sh).double()
    return v.numpy()


def run_ew(dev, a, b, sc, sh, act, mul, off=0):
    rows, C = a.shape
    ab, yb = Buf(dev, a.size, off, a), Buf(dev, a.size, off)
    bb = None if b is None else Buf(dev, a.size, off, b)
    scb = None if sc is None else Buf(dev, C, 0, sc)
    shb = None if sh is None else Buf(dev, C, 0, sh)
    call(dev, 'nrt_add_act_affine_f32', ab.p, None if bb is None else bb.p, None if scb is None else scb.p,
         None if shb is None else shb.p, yb.p, a.size, C, int(act) | (M._ACT_MUL_B if mul else 0))
    return yb.get(a.shape)


# rows x C; 45 x 24: n / 4 = 270 float4 (two blocks), 6 float4 per row (256 % 6 != 0: the channel of a thread's float4 moves)
EW_ARMS = [('add_act_affine_v4', 45, 24, 0, True), ('add_act_affine_v4-no-affine', 46, 6, 0, False),
           ('add_act_affine-n%4', 37, 5, 0, True), ('add_act_affine-C%4', 10, 6, 0, True), ('add_act_affine-misaligned', 45, 24, 1, True)]


@pytest.mark.parametrize('arm,rows,C,off,affine', EW_ARMS, ids=[a[0] for a in EW_ARMS])
def test_add_act_affine_arm(dev, arm, rows, C, off, affine):
    rng = np.random.default_rng(rows * C)
    a, b = rng.standard_normal((rows, C)).astype(F), rng.standard_normal((rows, C)).astype(F)
    sc, sh = (rng.standard_normal(C).astype(F), rng.standard_normal(C).astype(F)) if affine else (None, None)
    assert ACT_LAST == max(ACT_NAMES)
    for act in range(ACT_LAST + 1):
        for bb, mul in ((None, False), (b, False), (b, True)):
            what = '%s act %s%s' % (arm, ACT_NAMES[act], ' * b' if mul else (' + b' if bb is not None else ''))
            close(run_ew(dev, a, bb, sc, sh, act, mul, off), ew_ref(a, bb, sc, sh, act, mul), what=what)
        if affine:                                        # the affine and no b, no scale at all
            close(run_ew(dev, a, None, None, None, act, False, off), ew_ref(a, None, None, None, act, False), what=arm + ' plain')


def test_add_act_affine_v4_second_pass(dev):
    """more than 4096 * 256 float4: a block of add_act_affine_v4 makes a second pass over its range, where the channel of its float4
    has advanced by 256 % (C / 4) and wrapped"""
    rng = np.random.default_rng(9)
    rows, C = 174800, 24
    assert rows * C // 4 > 4096 * 256
    a, b = rng.standard_normal((rows, C)).astype(F), rng.standard_normal((rows, C)).astype(F)
    sc, sh = rng.standard_normal(C).astype(F), rng.standard_normal(C).astype(F)
    close(run_ew(dev, a, b, sc, sh, 1, False), ew_ref(a, b, sc, sh, 1, False), what='add_act_affine_v4 second pass')


def slope64(y, act):
    """d act / d pre-activation through the output y (csrc/activations.h nrt_activate_slope), float64"""
    y = y.astype(np.float64)
    one = np.ones_like(y)
    return {0: one, 1: np.where(y > 0, 1.0, y + 1), 2: np.where(y > 0, 1.0, 0.0), 3: y * (1 - y), 4: 1 - y * y, 5: 1 - np.exp(-y),
            6: (1 - np.abs(y)) ** 2, 7: np.where(y > 0, 1.05070098735548049342, y + 1.05070098735548049342 * 1.67326324235437728481),
            8: y, 9: np.where((y > 0) & (y < 1), 0.2, 0.0), 10: np.where(y > 0, 1.0, 0.2)}[act]


ACT_BWD = [(n, off) for n in (3, 1027, 1202) for off in (0, 1)]


@pytest.mark.parametrize('n,off', ACT_BWD, ids=['n%d-%s' % (n, 'misaligned-act_bwd_tail' if off else ('act_bwd+tail' if n >= 4 else 'act_bwd_tail')) for n, off in ACT_BWD])
def test_act_bwd_arm(dev, n, off):
    """n = 3: no float4 at all; 1027 = 4 * 256 + 3 and 1202 = 4 * 300 + 2: one and two blocks of act_bwd and a tail launch; one float
    off alignment: n4 = 0, everything goes through ceil(n / 256) tail launches"""
    rng = np.random.default_rng(n + off)
    g = rng.standard_normal(n).astype(F)
    for act in range(ACT_LAST + 1):
        pre = torch.from_numpy(rng.standard_normal(n)).double()
        y = tuo.keras_activation(pre, ACT_NAMES[act]).numpy().astype(F)
        gb, yb, db = Buf(dev, n, off, g), Buf(dev, n, off, y), Buf(dev, n, off)
        call(dev, 'nrt_act_bwd_f32', gb.p, yb.p, act, db.p, n)
        got, want = db.get(), g.astype(np.float64) * slope64(y, act)
        if act in (0, 2):
            assert np.array_equal(got, want.astype(F)), ACT_NAMES[act]
        else:
            close_grad(got, want, 'act_bwd %s n %d' % (ACT_NAMES[act], n))


# ------------------------------------------------------------------------------------------------------------------------------
# batch norm: nrt_channel_sums_f32 / nrt_channel_axpby_f32
# ------------------------------------------------------------------------------------------------------------------------------

# test_unet_training_with_batch_norm runs 8 features without feat_mult: C = 8 throughout (256 % C == 0, a thread owns one channel).
# 24, 48, 300: the arm with one LDS atomic per element; 300 > 256: the per-channel loops over the block make a second pass.
# rows * C is no multiple of 256 in any case, and more than one block (8192 elements per block) in every case.
BN_CASES = [(8, 2051), (24, 683), (48, 171), (300, 37)]


@pytest.mark.parametrize('C,rows', BN_CASES, ids=['C%d-%s' % (C, 'thread-owns-channel' if 256 % C == 0 else 'lds-atomic') for C, rows in BN_CASES])
def test_channel_sums_and_axpby_arm(dev, C, rows):
    assert (rows * C) % 256 and rows * C > 8192
    rng = np.random.default_rng(C)
    a, b = rng.standard_normal((rows, C)).astype(F), rng.standard_normal((rows, C)).astype(F)
    for bb in (None, b):
        ab, ob = Buf(dev, a.size, 0, a), Buf(dev, C, 0, np.zeros(C, F))
        bbuf = None if bb is None else Buf(dev, a.size, 0, bb)
        call(dev, 'nrt_channel_sums_f32', ab.p, None if bbuf is None else bbuf.p, rows, C, ob.p)
        terms = a.astype(np.float64) * (1.0 if bb is None else bb.astype(np.float64))
        want = terms.sum(0)
        # any order of float32 additions of `rows` rounded products: |error| <= (rows + 1) 2^-24 sum |terms| (first order)
        bound = (rows + 1) * 2.0 ** -24 * np.abs(terms).sum(0)
        err = np.abs(ob.get() - want)
        print('channel_sums C %d: worst error / bound = %.3g' % (C, float((err / bound).max())))
        assert (err <= bound).all(), 'channel_sums C %d: %.3g x the summation bound' % (C, float((err / bound).max()))
    cA, cB, cC = (rng.standard_normal(C).astype(F) for _ in range(3))
    ab, bbuf, yb = Buf(dev, a.size, 0, a), Buf(dev, a.size, 0, b), Buf(dev, a.size)
    coef = [Buf(dev, C, 0, c) for c in (cA, cB, cC)]
    call(dev, 'nrt_channel_axpby_f32', ab.p, bbuf.p, coef[0].p, coef[1].p, coef[2].p, yb.p, a.size, C)
    assert np.array_equal(yb.get(a.shape), (cA * a + cB * b) + cC)        # float32, one rounding per operation, no contraction
