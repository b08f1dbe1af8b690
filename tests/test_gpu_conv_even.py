"""
GPU tests of convolutions with EVEN kernel sizes (models._Conv / models._ConvFn, layers.HyperConv) against float64
torch.nn.functional.conv3d on the CPU with explicit asymmetric zero padding: 'same' pads p = (k - 1) * dilation // 2 before and
(k - 1) * dilation - p after (TensorFlow's rule), so the input gradient -- the transposed convolution -- pads (k - 1) * dilation - p
BEFORE.  For odd kernels the two coincide; for even ones the input gradient is shifted by one voxel if the forward's padding is reused.

  forward      element-wise |err| <= 8 * 2^-24 * S, S = |b| + sum |x_i| |w_i| (the criterion of tests/test_gpu_unet.py; ELU adds the 3e-6
               of the hardware exponential, as there); a repeated call gives the same bits
  gx, gw, gb   within 2e-4 of the gradient's scale against float64 autograd (the criterion of tests/test_gpu_conv_backward.py); gx of a
               repeated call has the same bits (gw and gb are accumulated with float atomics and are not run-to-run identical)
"""

import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from neurite_amd import layers as L
from neurite_amd import models as M

pytestmark = pytest.mark.gpu
F = np.float32
B = 2
TOL = 2e-4

KSIZES = [(2, 2, 2), (2, 3, 1), (4, 4, 4)]
SHAPES = [(5, 6, 7), (8, 8, 16), (9, 7, 18)]
CHANNELS = [(1, 4), (3, 5), (8, 16), (16, 16), (32, 64)]


def _cases():
    out = []
    for ks, dil, padding, shape, (cin, cout) in itertools.product(KSIZES, (1, 2), ('same', 'valid'), SHAPES, CHANNELS):
        if padding == 'valid' and any(shape[d] - (ks[d] - 1) * dil < 1 for d in range(3)):
            continue                                            # the size does not allow it
        out.append((ks, dil, padding, shape, cin, cout))
    return out


def _ref_conv(x, w, b, ks, dil, padding, act):
    """x [B, X, Y, Z, Cin], w [kx, ky, kz, Cin, Cout] float64 torch tensors -> (activated output, pre-activation) channels-last"""
    xc = x.permute(0, 4, 1, 2, 3)
    if padding == 'same':
        pads = []
        for d in (2, 1, 0):                                     # F.pad takes the last axis first
            tot = (ks[d] - 1) * dil
            pads += [tot // 2, tot - tot // 2]
        xc = TF.pad(xc, pads)
    pre = TF.conv3d(xc, w.permute(4, 3, 0, 1, 2), b, dilation=dil).permute(0, 2, 3, 4, 1)
    return (TF.elu(pre) if act == 'elu' else pre), pre


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert err < TOL, '%s: max err / scale = %.3g' % (what, err)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _setup(ks, cin, cout, shape, seed):
    rng = np.random.default_rng(seed)
    fan = int(np.prod(ks)) * cin
    kern = (rng.standard_normal(ks + (cin, cout)) / np.sqrt(fan)).astype(F)
    bias = (rng.standard_normal(cout) * 0.1).astype(F)
    x = rng.standard_normal((B,) + shape + (cin,)).astype(F)
    return rng, kern, bias, x


@pytest.mark.parametrize('act', ['elu', None])
@pytest.mark.parametrize('ks,dil,padding,shape,cin,cout', _cases())
def test_even_kernel_forward_and_gradients(dev, ks, dil, padding, shape, cin, cout, act):
    rng, kern, bias, x = _setup(ks, cin, cout, shape, sum(ks) * 1000 + dil * 100 + cin + cout + shape[2])
    conv = M._Conv('c', cin, cout, ks, dilation=dil, padding=padding, activation=act).to(dev)
    with torch.no_grad():
        conv.kernel.copy_(torch.from_numpy(kern)); conv.bias.copy_(torch.from_numpy(bias))
    xo = torch.from_numpy(x).double().requires_grad_()
    ko = torch.from_numpy(kern).double().requires_grad_()
    bo = torch.from_numpy(bias).double().requires_grad_()
    yo, pre = _ref_conv(xo, ko, bo, ks, dil, padding, act)
    w = rng.standard_normal(tuple(yo.shape)).astype(F)
    (yo * torch.from_numpy(w).double()).sum().backward()
    with torch.no_grad():
        _, absref = _ref_conv(xo.abs(), ko.abs(), bo.abs(), ks, dil, padding, None)

    xg = torch.from_numpy(x).to(dev).requires_grad_()
    y = conv(xg)
    assert tuple(y.shape) == tuple(yo.shape)
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    gx1 = xg.grad.clone()
    # the same call again: same bits in the forward and in the input gradient
    xg2 = torch.from_numpy(x).to(dev).requires_grad_()
    conv.kernel.grad = None; conv.bias.grad = None
    y2 = conv(xg2)
    (y2 * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y), _bits(y2)), 'forward differs between two calls'
    assert np.array_equal(_bits(gx1), _bits(xg2.grad)), 'gx differs between two calls'

    err = np.abs(y.detach().cpu().numpy().astype(np.float64) - yo.detach().numpy())
    bound = 8 * 2.0 ** -24 * absref.numpy() + (3e-6 if act == 'elu' else 0.0) + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, 'forward error %.2f x the float32 dot-product bound' % worst
    _close(xg2.grad.cpu().numpy(), xo.grad.numpy(), 'grad_x')
    _close(conv.kernel.grad.cpu().numpy(), ko.grad.numpy(), 'grad_kernel')
    _close(conv.bias.grad.cpu().numpy(), bo.grad.numpy(), 'grad_bias')


K2_CASES = [(shape, cin, cout, lo) for shape in SHAPES + [(8, 12, 34)] for cin, cout in [(8, 16), (16, 16), (32, 64), (12, 40), (24, 7)]
            for lo in (False,)] + [((8, 8, 16), 24, 16, True), ((4, 6, 18), 12, 5, True)]


@pytest.mark.parametrize('act', ['elu', None])
@pytest.mark.parametrize('shape,cin,cout,lo', K2_CASES)
def test_2x2x2_matrix_core_arm_forced(dev, shape, cin, cout, lo, act):
    """variant 6 on every kind of shape it accepts (on and off the 4 x 4 x 16 tile, one to four 16-channel output blocks, a last
    input chunk that is not full, a second up-sampled source): forward and input gradient under the bounds of the direct kernel,
    which runs on the same inputs; both repeat bit for bit"""
    ks, dil = (2, 2, 2), 1
    rng, kern, bias, x = _setup(ks, cin, cout, shape, cin * 7 + cout + shape[2])
    c0 = cin - 8 if lo else cin
    up = (2, 2, 2)
    xo = torch.from_numpy(x).double().requires_grad_()
    ko, bo = torch.from_numpy(kern).double(), torch.from_numpy(bias).double()
    if lo:                                                       # channels [c0, cin) come from a half-resolution tensor
        xlo = rng.standard_normal((B,) + tuple(s // 2 for s in shape) + (cin - c0,)).astype(F)
        lo_o = torch.from_numpy(xlo).double().requires_grad_()
        upl = lo_o
        for d in range(3):
            upl = upl.repeat_interleave(2, dim=1 + d)
        src = torch.cat([xo[..., :c0], upl], -1)
    else:
        src = xo
    yo, _ = _ref_conv(src, ko, bo, ks, dil, 'same', act)
    w = rng.standard_normal(tuple(yo.shape)).astype(F)
    (yo * torch.from_numpy(w).double()).sum().backward()
    with torch.no_grad():
        _, absref = _ref_conv(src.abs(), ko.abs(), bo.abs(), ks, dil, 'same', None)
    bound = 8 * 2.0 ** -24 * absref.numpy() + (3e-6 if act == 'elu' else 0.0) + 1e-30
    conv = M._Conv('c', cin, cout, ks, dilation=dil, padding='same', activation=act).to(dev)
    conv.fold_backward = False
    with torch.no_grad():
        conv.kernel.copy_(torch.from_numpy(kern)); conv.bias.copy_(torch.from_numpy(bias))
    res = {}
    for variant in (1, 6, 6):
        xg = torch.from_numpy(x[..., :c0].copy()).to(dev).requires_grad_()
        lg = torch.from_numpy(xlo).to(dev).requires_grad_() if lo else None
        conv.kernel.grad = None; conv.bias.grad = None
        y = conv(xg, lo=lg, up=up if lo else None, variant=variant)
        (y * torch.from_numpy(w).to(dev)).sum().backward()
        torch.cuda.synchronize()
        err = np.abs(y.detach().cpu().numpy().astype(np.float64) - yo.detach().numpy())
        worst = float((err / bound).max())
        assert worst <= 1.0, 'variant %d: forward error %.2f x the float32 dot-product bound' % (variant, worst)
        _close(xg.grad.cpu().numpy(), xo.grad.numpy()[..., :c0], 'grad_x (variant %d)' % variant)
        if lo:
            _close(lg.grad.cpu().numpy(), lo_o.grad.numpy(), 'grad_lo (variant %d)' % variant)
        res.setdefault(variant, []).append((_bits(y), _bits(xg.grad)))
    (y1, g1), (y2, g2) = res[6]
    assert np.array_equal(y1, y2) and np.array_equal(g1, g2), 'the 2x2x2 arm differs between two calls'


def test_auto_dispatch_takes_the_2x2x2_arm_from_its_measured_size_on(dev):
    """variant 0: 16 -> 16 at 2 x 40 x 40 x 80 (= 4 x 40^3 output voxels, the smallest measured) runs conv3d_mfma_k2, one voxel row
    less runs conv3d_direct -- the bits of the forced arms say which kernel ran"""
    ks = (2, 2, 2)
    for shape, arm in (((40, 40, 80), 6), ((40, 40, 79), 1)):
        rng, kern, bias, x = _setup(ks, 16, 16, shape, 77)
        conv = M._Conv('c', 16, 16, ks, padding='same', activation='elu').to(dev)
        with torch.no_grad():
            conv.kernel.copy_(torch.from_numpy(kern)); conv.bias.copy_(torch.from_numpy(bias))
            xg = torch.from_numpy(x).to(dev)
            auto, direct, k2 = conv(xg, variant=0), conv(xg, variant=1), conv(xg, variant=6)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(direct), _bits(k2))
        assert np.array_equal(_bits(auto), _bits(k2 if arm == 6 else direct)), shape


@pytest.mark.parametrize('same', [True, False])
@pytest.mark.parametrize('cin,cout,shape', [(3, 5, (5, 6, 7)), (16, 16, (8, 8, 16))])
def test_hyperconv_even_kernel_gradients(dev, cin, cout, shape, same):
    """per-entry 2x2x2 kernels (layers.HyperConv*): the input gradient ran the forward kernel with the forward's padding too"""
    ks, dil = (2, 2, 2), 1
    rng = np.random.default_rng(cin + cout)
    kern = (rng.standard_normal((B,) + ks + (cin, cout)) / np.sqrt(8 * cin)).astype(F)
    bias = (rng.standard_normal((B, cout)) * 0.1).astype(F)
    x = rng.standard_normal((B,) + shape + (cin,)).astype(F)
    xo = torch.from_numpy(x).double().requires_grad_()
    ko = torch.from_numpy(kern).double().requires_grad_()
    bo = torch.from_numpy(bias).double().requires_grad_()
    yo = torch.cat([_ref_conv(xo[b:b + 1], ko[b], bo[b], ks, dil, 'same' if same else 'valid', 'elu')[0] for b in range(B)], 0)
    w = rng.standard_normal(tuple(yo.shape)).astype(F)
    (yo * torch.from_numpy(w).double()).sum().backward()
    xg = torch.from_numpy(x).to(dev).requires_grad_()
    kg = torch.from_numpy(kern).to(dev).requires_grad_()
    bg = torch.from_numpy(bias).to(dev).requires_grad_()
    y = L._hyperconv(xg, kg, bg, ks, dil, same, M._act_code('elu'))
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    _close(y.detach().cpu().numpy(), yo.detach().numpy(), 'forward')
    _close(xg.grad.cpu().numpy(), xo.grad.numpy(), 'grad_x')
    _close(kg.grad.cpu().numpy(), ko.grad.numpy(), 'grad_kernel')
    _close(bg.grad.cpu().numpy(), bo.grad.numpy(), 'grad_bias')
