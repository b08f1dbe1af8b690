"""
GPU tests of the hyper-convolution / hyper-dense layers (neurite_amd/layers.py, nrt_hyperconv3d_* in csrc/conv.hip and
csrc/conv_bwd.hip) against torch CPU float64 arithmetic of the same definition, PER BATCH ENTRY: entry b is compared with the
reference of its own kernel and bias.

Criteria (the project's own for this operation class, nothing new):
  forward   tests/test_gpu_unet.py conv_refs / close_conv: element-wise |err| <= 8 * 2^-24 * sum |x_i w_i| and 1e-5 relative on
            well-conditioned outputs ('same' padding, where the C oracle applies); 1e-4 of the output scale for the 'valid' cases
            (tests/test_gpu_conv_backward.py `close`)
  backward  float64 autograd of oracle.torch_unet_oracle.conv3d_same, 2e-4 of the gradient's largest magnitude
            (tests/test_gpu_conv_backward.py).  The per-entry gradient sums over fewer voxels than the batch-summed one that
            tolerance was set for.
The weight and bias gradients are accumulated with float atomics (one per weight and block, as nrt_conv3d_wgrad_f32): they are not
run-to-run bit-identical and are compared by tolerance; the forward and the input gradient use no atomics and are.
"""

import numpy as np
import pytest
import torch

from neurite_amd import _lib
from neurite_amd import layers as L
from neurite_amd import models as M
from oracle import torch_unet_oracle as tuo
from test_gpu_conv_backward import close, TOL
from test_gpu_unet import close_conv, conv_refs

pytestmark = pytest.mark.gpu
F = np.float32
B = 3

SAME_CASES = [                                   # the shape list of test_gpu_conv_backward.test_conv_backward
    (16, 16, 3, 1, 'elu', (9, 10, 17)),
    (16, 16, 3, 1, 'elu', (48, 44, 12)),
    (48, 16, 3, 1, 'elu', (8, 8, 16)),
    (96, 32, 3, 1, 'elu', (8, 4, 8)),
    (32, 64, 3, 1, 'relu', (4, 8, 8)),
    (1, 16, 3, 1, 'elu', (12, 9, 10)),
    (8, 3, 3, 1, None, (7, 8, 9)),
    (20, 24, 3, 2, 'elu', (10, 9, 12)),
    (16, 5, 1, 1, None, (6, 7, 8)),
    (16, 16, (1, 3, 3), 1, 'elu', (1, 12, 13)),
]
VALID_CASES = [                                  # test_conv_backward_valid_padding
    (16, 16, 3, 1, 'elu', (9, 10, 17)), (8, 12, 3, 2, 'relu', (11, 9, 13)), (4, 8, (1, 3, 3), 1, None, (1, 9, 12)),
    (1, 16, 3, 1, 'elu', (8, 9, 10)),
]


def G(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_() if grad else t


def N(t):
    return t.detach().cpu().numpy()


def _case(cin, cout, k, dil, shape, padding, seed):
    rng = np.random.default_rng(seed)
    ks = (k,) * 3 if isinstance(k, int) else tuple(k)
    fan = int(np.prod(ks)) * cin
    kern = (rng.standard_normal((B,) + ks + (cin, cout)) / np.sqrt(fan)).astype(F)        # a DIFFERENT kernel and bias per entry
    bias = (rng.standard_normal((B, cout)) * 0.1).astype(F)
    x = rng.standard_normal((B,) + shape + (cin,)).astype(F)
    oshape = shape if padding == 'same' else tuple(shape[d] - (ks[d] - 1) * dil for d in range(3))
    w = rng.standard_normal((B,) + oshape + (cout,)).astype(F)
    return ks, kern, bias, x, w, oshape


def _reference(x, kern, bias, w, dil, act, padding):
    """float64 autograd, entry by entry with the entry's own kernel: outputs and the three gradients"""
    xo = torch.from_numpy(x).double().requires_grad_()
    ko = torch.from_numpy(kern).double().requires_grad_()
    bo = None if bias is None else torch.from_numpy(bias).double().requires_grad_()
    ys = [tuo.conv3d_same(xo[b:b + 1], ko[b], None if bo is None else bo[b], dil, act, padding=padding) for b in range(x.shape[0])]
    yo = torch.cat(ys, 0)
    (yo * torch.from_numpy(w).double()).sum().backward()
    return yo.detach().numpy(), xo.grad.numpy(), ko.grad.numpy(), None if bo is None else bo.grad.numpy()


def _run_layer(dev, x, kern, bias, w, ks, dil, act, padding):
    layer = L.HyperConv3D(kern.shape[-1], ks, padding=padding, dilation_rate=dil, activation=act, use_bias=bias is not None)
    xg, kg = G(x, dev, True), G(kern, dev, True)
    bg = None if bias is None else G(bias, dev, True)
    y = layer([xg, kg] + ([] if bg is None else [bg]))
    (y * G(w, dev)).sum().backward()
    return y, xg.grad, kg.grad, None if bg is None else bg.grad


def _check_per_entry(y, gx, gk, gb, yo, gxo, gko, gbo):
    for b in range(y.shape[0]):
        close(N(y[b]), yo[b], 'forward[%d]' % b, 1e-4)
        close(N(gk[b]), gko[b], 'grad_kernel[%d]' % b)
        if gbo is not None:
            close(N(gb[b]), gbo[b], 'grad_bias[%d]' % b)
        close(N(gx[b]), gxo[b], 'grad_x[%d]' % b)


@pytest.mark.parametrize('cin,cout,k,dil,act,shape', SAME_CASES)
def test_hyperconv_same(dev, cin, cout, k, dil, act, shape):
    ks, kern, bias, x, w, _ = _case(cin, cout, k, dil, shape, 'same', cin * 100 + cout)
    y, gx, gk, gb = _run_layer(dev, x, kern, bias, w, ks, dil, act, 'same')
    yo, gxo, gko, gbo = _reference(x, kern, bias, w, dil, act, 'same')
    assert tuple(y.shape) == (B,) + shape + (cout,)
    yn = N(y)
    for b in range(B):                           # the forward by the conv criteria, each entry against ITS kernel
        ref, absref = conv_refs(x[b], kern[b], bias[b], dil)
        close_conv(yn[b], ref, absref, act)
    _check_per_entry(y, gx, gk, gb, yo, gxo, gko, gbo)
    # a kernel that ignores the batch stride cannot pass: entry 0 is NOT the convolution with entry 1's kernel
    wrong = tuo.conv3d_same(torch.from_numpy(x[:1]).double(), torch.from_numpy(kern[1]).double(), torch.from_numpy(bias[1]).double(),
                            dil, act).numpy()[0]
    assert float(np.abs(yn[0] - wrong).max()) > 100 * 1e-4 * float(np.abs(wrong).max())
    assert float(np.abs(N(gk[0]) - gko[1]).max()) > 100 * TOL * float(np.abs(gko[1]).max())


@pytest.mark.parametrize('cin,cout,k,dil,act,shape', VALID_CASES)
def test_hyperconv_valid(dev, cin, cout, k, dil, act, shape):
    ks, kern, bias, x, w, oshape = _case(cin, cout, k, dil, shape, 'valid', cin * 10 + cout + dil)
    y, gx, gk, gb = _run_layer(dev, x, kern, bias, w, ks, dil, act, 'valid')
    assert tuple(y.shape) == (B,) + oshape + (cout,)
    yo, gxo, gko, gbo = _reference(x, kern, bias, w, dil, act, 'valid')
    _check_per_entry(y, gx, gk, gb, yo, gxo, gko, gbo)
    wrong = tuo.conv3d_same(torch.from_numpy(x[:1]).double(), torch.from_numpy(kern[1]).double(), torch.from_numpy(bias[1]).double(),
                            dil, act, padding='valid').numpy()[0]
    assert float(np.abs(N(y[0]) - wrong).max()) > 100 * 1e-4 * float(np.abs(wrong).max())


def _abi_forward(dev, x, kern, bias, ks, dil, act_code, variant, shared=False):
    """nrt_hyperconv3d_f32 (or, shared: nrt_conv3d_f32 with kern[0] / bias[0]) straight through the C ABI with an explicit variant"""
    lib = _lib.lib()
    Bn, S, cin, cout = x.shape[0], list(x.shape[1:4]), x.shape[-1], kern.shape[-1]
    xg, kg, bg = G(x, dev), G(kern, dev), G(bias, dev)
    out = torch.empty([Bn] + S + [cout], dtype=torch.float32, device=dev)
    n = int(lib.nrt_conv3d_packed_weight_floats(_lib.ints(ks), cin, cout))
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        if shared:
            packed = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.check(lib.nrt_conv3d_pack_weights_f32(_lib.ptr(kg[0]), _lib.ints(ks), cin, cout, _lib.ptr(packed), st), 'pack')
            rc = lib.nrt_conv3d_f32(_lib.ptr(xg), cin, None, 0, None, _lib.ptr(kg[0]), _lib.ptr(packed), _lib.ptr(bg[0]), _lib.ptr(out),
                                    Bn, _lib.ints(S), _lib.ints(ks), cout, dil, 1, act_code, variant, st)
        else:
            packed = torch.empty(Bn * n, dtype=torch.float32, device=dev)
            _lib.check(lib.nrt_hyperconv3d_pack_weights_f32(_lib.ptr(kg), Bn, _lib.ints(ks), cin, cout, 0, _lib.ptr(packed), st), 'pack')
            rc = lib.nrt_hyperconv3d_f32(_lib.ptr(xg), cin, _lib.ptr(kg), _lib.ptr(packed), _lib.ptr(bg), _lib.ptr(out), Bn, _lib.ints(S),
                                         _lib.ints(ks), cout, dil, 1, act_code, variant, st)
    _lib.check(rc, 'conv variant %d' % variant)
    torch.cuda.synchronize(dev)
    return N(out), (N(packed), n)


@pytest.mark.parametrize('cin,cout,shape', [(16, 16, (9, 10, 17)), (48, 16, (8, 8, 32)), (16, 32, (8, 8, 16)), (32, 48, (5, 8, 16)),
                                            (32, 64, (4, 8, 16))])
def test_persistent_schedule_per_entry(dev, cin, cout, shape):
    """variant 5 (the persistent LDS-DMA schedule, whose blocks walk tiles of several batch entries): every instantiation (1 - 4 output
    blocks; deferred and immediate stores; ragged tiles) picks the weights and the bias of the tile's entry.  The auto choice only
    takes this kernel from two tiles per CU on, so it is asked for by number here; the large case below reaches it through the layer."""
    ks, kern, bias, x, _, _ = _case(cin, cout, 3, 1, shape, 'same', cin + cout)
    y, (packed, n) = _abi_forward(dev, x, kern, bias, ks, 1, 1, 5)
    for b in range(B):
        ref, absref = conv_refs(x[b], kern[b], bias[b], 1)
        close_conv(y[b], ref, absref, 'elu')
    # the batched pack is the shared pack, entry by entry
    lib = _lib.lib()
    for b in range(B):
        one = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.nrt_conv3d_pack_weights_f32(_lib.ptr(G(kern[b], dev)), _lib.ints(ks), cin, cout, _lib.ptr(one),
                                                       _lib.stream_ptr(dev)), 'pack')
        assert np.array_equal(N(one), packed[b * n:(b + 1) * n])
    # same kernel for every entry: bit-identical to the shared-weight entry point, variant by variant
    kern1, bias1 = np.repeat(kern[:1], B, 0), np.repeat(bias[:1], B, 0)
    for variant in (5, 2, 1):
        a, _ = _abi_forward(dev, x, kern1, bias1, ks, 1, 1, variant)
        s, _ = _abi_forward(dev, x, kern1, bias1, ks, 1, 1, variant, shared=True)
        assert np.array_equal(a.view(np.uint32), s.view(np.uint32)), 'variant %d' % variant


@pytest.mark.parametrize('cin,cout', [(16, 16), (16, 32), (32, 48), (32, 64)])
def test_persistent_blocks_cross_batch_entries(dev, cin, cout):
    """3 x 24 x 24 x 64 voxels = 432 tiles on at most 256 persistent blocks: blocks take two tiles, and the tile range of one XCD
    (54 tiles) straddles the entry boundaries at tiles 144 and 288 -- a block's second tile belongs to the NEXT entry, whose weights and
    bias it has to pick up (every output-block count of the kernel)"""
    shape = (24, 24, 64)
    ks, kern, bias, x, _, _ = _case(cin, cout, 3, 1, shape, 'same', cin * 3 + cout)
    y, _ = _abi_forward(dev, x, kern, bias, ks, 1, 1, 5)
    for b in range(B):
        ref, absref = conv_refs(x[b], kern[b], bias[b], 1)
        close_conv(y[b], ref, absref, 'elu')
    y2, _ = _abi_forward(dev, x, kern, bias, ks, 1, 1, 5)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))


def test_transpose_flip_pack(dev):
    """transpose_flip packs, per entry, what models._conv_dgrad builds on the host with flip().transpose().contiguous()"""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    for ks, cin, cout in (((3, 3, 3), 20, 24), ((1, 3, 3), 16, 40), ((1, 1, 1), 64, 8)):
        kern = rng.standard_normal((B,) + ks + (cin, cout)).astype(F)
        kg = G(kern, dev)
        n = int(lib.nrt_conv3d_packed_weight_floats(_lib.ints(ks), cout, cin))
        packed = torch.empty(B * n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.nrt_hyperconv3d_pack_weights_f32(_lib.ptr(kg), B, _lib.ints(ks), cin, cout, 1, _lib.ptr(packed),
                                                            _lib.stream_ptr(dev)), 'pack')
            for b in range(B):
                wt = kg[b].flip(0, 1, 2).transpose(3, 4).contiguous()
                one = torch.empty(n, dtype=torch.float32, device=dev)
                _lib.check(lib.nrt_conv3d_pack_weights_f32(_lib.ptr(wt), _lib.ints(ks), cout, cin, _lib.ptr(one), _lib.stream_ptr(dev)), 'pack')
                assert torch.equal(one, packed[b * n:(b + 1) * n])


def test_auto_choice_reaches_the_persistent_schedule(dev):
    """3 x 32 x 32 x 64 voxels, 16 -> 16 channels: 768 tiles, above two per CU -- the layer's auto choice is the persistent kernel"""
    cin = cout = 16
    shape = (32, 32, 64)
    ks, kern, bias, x, w, _ = _case(cin, cout, 3, 1, shape, 'same', 11)
    y, gx, gk, gb = _run_layer(dev, x, kern, bias, w, ks, 1, 'elu', 'same')
    yn = N(y)
    for b in range(B):
        ref, absref = conv_refs(x[b], kern[b], bias[b], 1)
        close_conv(yn[b], ref, absref, 'elu')
    forced, _ = _abi_forward(dev, x, kern, bias, ks, 1, 1, 5)
    assert np.array_equal(yn.view(np.uint32), forced.view(np.uint32))
    yo, gxo, gko, gbo = _reference(x, kern, bias, w, 1, 'elu', 'same')
    _check_per_entry(y, gx, gk, gb, yo, gxo, gko, gbo)


@pytest.mark.parametrize('cin,cout,k,dil,shape', [(16, 16, 3, 1, (9, 10, 17)), (48, 16, 3, 1, (8, 8, 16)), (1, 16, 3, 1, (12, 9, 10)),
                                                  (20, 24, 3, 2, (10, 9, 12)), (16, 5, 1, 1, (6, 7, 8)), (8, 3, 3, 1, (7, 8, 9))])
def test_per_entry_weight_gradient_sums_to_the_shared_one(dev, cin, cout, k, dil, shape):
    """cross-check of the two code paths: sum_b nrt_hyperconv3d_wgrad_f32[b] == nrt_conv3d_wgrad_f32 on the same tensors (2e-4 of scale),
    and each entry against float64 of that entry alone"""
    lib = _lib.lib()
    rng = np.random.default_rng(cin + cout)
    ks = (k,) * 3
    x = rng.standard_normal((B,) + shape + (cin,)).astype(F)
    dp = rng.standard_normal((B,) + shape + (cout,)).astype(F)
    xg, dg = G(x, dev), G(dp, dev)
    gk = torch.zeros((B,) + ks + (cin, cout), dtype=torch.float32, device=dev)
    gb = torch.zeros(B, cout, dtype=torch.float32, device=dev)
    sk = torch.zeros(ks + (cin, cout), dtype=torch.float32, device=dev)
    sb = torch.zeros(cout, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        _lib.check(lib.nrt_hyperconv3d_wgrad_f32(_lib.ptr(xg), _lib.ptr(dg), _lib.ptr(gk), _lib.ptr(gb), B, _lib.ints(shape), cin, cout,
                                                 _lib.ints(ks), dil, st), 'hyper wgrad')
        _lib.check(lib.nrt_conv3d_wgrad_f32(_lib.ptr(xg), _lib.ptr(dg), _lib.ptr(sk), _lib.ptr(sb), B, _lib.ints(shape), cin, cout,
                                            _lib.ints(ks), dil, st), 'shared wgrad')
    close(N(gk.sum(0)), N(sk), 'sum of the per-entry weight gradients')
    close(N(gb.sum(0)), N(sb), 'sum of the per-entry bias gradients')
    for b in range(B):
        ko = torch.zeros(ks + (cin, cout), dtype=torch.float64, requires_grad=True)
        bo = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        yo = tuo.conv3d_same(torch.from_numpy(x[b:b + 1]).double(), ko, bo, dil, None)
        (yo * torch.from_numpy(dp[b:b + 1]).double()).sum().backward()
        close(N(gk[b]), ko.grad.numpy(), 'grad_kernel[%d]' % b)
        close(N(gb[b]), bo.grad.numpy(), 'grad_bias[%d]' % b)
    # bias gradient may be left out
    gk2 = torch.zeros_like(gk)
    with torch.cuda.device(dev):
        _lib.check(lib.nrt_hyperconv3d_wgrad_f32(_lib.ptr(xg), _lib.ptr(dg), _lib.ptr(gk2), None, B, _lib.ints(shape), cin, cout,
                                                 _lib.ints(ks), dil, _lib.stream_ptr(dev)), 'hyper wgrad')
    close(N(gk2), N(gk), 'without grad_bias')


# shapes where HyperConv3D and models._Conv take the same kernel variant for the same arguments: the plain (single-source) 'same' and
# 'valid' convolutions -- _Conv only differs for the folded decoder / pool / head forms, which have a second source or a second output.
# MFMA (one tile per block) 16/16, 48/16, dilation 2, 1x1x1 with 64 channels; direct kernel 8/3 and 'valid'; single-channel kernels 1/16
@pytest.mark.parametrize('cin,cout,k,dil,act,shape,padding', [
    (16, 16, 3, 1, 'elu', (9, 10, 17), 'same'), (48, 16, 3, 1, 'elu', (8, 8, 16), 'same'), (20, 24, 3, 2, 'relu', (10, 9, 12), 'same'),
    (64, 16, 1, 1, None, (4, 4, 16), 'same'), (8, 3, 3, 1, None, (7, 8, 9), 'same'), (1, 16, 3, 1, 'elu', (12, 9, 10), 'same'),
    (1, 8, 3, 2, 'elu', (12, 9, 10), 'same'), (16, 16, 3, 1, 'tanh', (9, 10, 17), 'valid'),
])
def test_same_kernel_for_every_entry_equals_conv_bit_for_bit(dev, cin, cout, k, dil, act, shape, padding):
    ks, kern, bias, x, _, _ = _case(cin, cout, k, dil, shape, padding, 5)
    conv = M._Conv('c', cin, cout, ks, dilation=dil, padding=padding, activation=act).to(dev)
    with torch.no_grad():
        conv.kernel.copy_(G(kern[0], dev)); conv.bias.copy_(G(bias[0], dev))
        want = conv(G(x, dev))
        layer = L.HyperConv3D(cout, ks, padding=padding, dilation_rate=dil, activation=act)
        got = layer([G(x, dev), G(np.repeat(kern[:1], B, 0), dev), G(np.repeat(bias[:1], B, 0), dev)])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_run_to_run(dev):
    """forward and input gradient: no atomics, bit-identical over two runs; weight / bias gradients: float atomics, by tolerance"""
    for cin, cout, k, dil, act, shape in (SAME_CASES[1], SAME_CASES[5], SAME_CASES[6]):
        ks, kern, bias, x, w, _ = _case(cin, cout, k, dil, shape, 'same', 9)
        a = _run_layer(dev, x, kern, bias, w, ks, dil, act, 'same')
        b = _run_layer(dev, x, kern, bias, w, ks, dil, act, 'same')
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        close(N(a[2]), N(b[2]), 'grad_kernel, two runs')
        close(N(a[3]), N(b[3]), 'grad_bias, two runs')


def _ref_act(t, act):
    return tuo.keras_activation(t, act)


def test_hyperconv2d_tanh_no_bias(dev):
    """rank 2 on the 3-D kernels, a non-fused activation and use_bias=False"""
    rng = np.random.default_rng(21)
    cin, cout, S = 12, 20, (11, 14)
    x = rng.standard_normal((B,) + S + (cin,)).astype(F)
    kern = (rng.standard_normal((B, 3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(F)
    w = rng.standard_normal((B,) + S + (cout,)).astype(F)
    layer = L.HyperConv2D(cout, 3, padding='same', activation='tanh', use_bias=False)
    xg, kg = G(x, dev, True), G(kern, dev, True)
    y = layer([xg, kg])
    assert tuple(y.shape) == (B,) + S + (cout,)
    (y * G(w, dev)).sum().backward()
    yo, gxo, gko, _ = _reference(x[:, None], kern[:, None], None, w[:, None], 1, 'tanh', 'same')
    close(N(y), yo[:, 0], 'forward', 1e-4)
    close(N(xg.grad), gxo[:, 0], 'grad_x')
    for b in range(B):
        close(N(kg.grad[b]), gko[b, 0], 'grad_kernel[%d]' % b)


@pytest.mark.parametrize('lead,cin,units,act,use_bias', [((7, 9), 16, 24, 'relu', True), ((5, 6, 7), 12, 5, 'tanh', True),
                                                         ((33,), 3, 70, None, False), ((), 16, 16, None, True)])
def test_hyperdense(dev, lead, cin, units, act, use_bias):
    rng = np.random.default_rng(cin + units)
    x = rng.standard_normal((B,) + lead + (cin,)).astype(F)
    kern = (rng.standard_normal((B, cin, units)) / np.sqrt(cin)).astype(F)
    bias = (rng.standard_normal((B, units)) * 0.1).astype(F)
    w = rng.standard_normal((B,) + lead + (units,)).astype(F)
    layer = L.HyperDense(units, activation=act, use_bias=use_bias)
    xg, kg, bg = G(x, dev, True), G(kern, dev, True), G(bias, dev, True)
    y = layer([xg, kg, bg] if use_bias else [xg, kg])
    assert tuple(y.shape) == (B,) + lead + (units,)
    (y * G(w, dev)).sum().backward()
    xo, ko, bo = (torch.from_numpy(a).double().requires_grad_() for a in (x, kern, bias))
    pre = torch.einsum('b...i,biu->b...u', xo, ko)
    if use_bias:
        pre = pre + bo.reshape((B,) + (1,) * len(lead) + (units,))
    yo = _ref_act(pre, act)
    (yo * torch.from_numpy(w).double()).sum().backward()
    close(N(y), yo.detach().numpy(), 'forward', 1e-4)
    close(N(xg.grad), xo.grad.numpy(), 'grad_x')
    for b in range(B):
        close(N(kg.grad[b]), ko.grad[b].numpy(), 'grad_kernel[%d]' % b)
        if use_bias:
            close(N(bg.grad[b]), bo.grad[b].numpy(), 'grad_bias[%d]' % b)


def _from_dense_reference(layer, x, hyp, w, conv):
    """float64 autograd through the pseudo-dense maps and the per-entry operation; returns outputs and gradients by name"""
    p = {n: t.detach().cpu().double().requires_grad_() for n, t in layer.named_parameters()}
    xo, ho = torch.from_numpy(x).double().requires_grad_(), torch.from_numpy(hyp).double().requires_grad_()

    def dense(name, act, target):
        out = ho @ p[name + '_kernel']
        if name + '_bias' in p:
            out = out + p[name + '_bias']
        return _ref_act(out, act).reshape((-1,) + tuple(target))
    yo = conv(xo, dense, p)
    (yo * torch.from_numpy(w).double()).sum().backward()
    grads = {n: t.grad.numpy() for n, t in p.items()}
    grads['x'], grads['hyp'] = xo.grad.numpy(), ho.grad.numpy()
    return yo.detach().numpy(), grads


@pytest.mark.parametrize('rank,S,cin,cout,padding,act,use_bias,hk_act', [
    (3, (8, 9, 10), 16, 16, 'same', 'elu', True, None), (3, (7, 8, 9), 4, 6, 'valid', 'tanh', False, 'tanh'),
    (2, (12, 13), 8, 16, 'same', 'relu', True, 'sigmoid'),
])
def test_hyperconv_from_dense(dev, rank, S, cin, cout, padding, act, use_bias, hk_act):
    rng = np.random.default_rng(rank * 10 + cin)
    H = 5
    cls = L.HyperConv3DFromDense if rank == 3 else L.HyperConv2DFromDense
    layer = cls(cout, 3, padding=padding, activation=act, use_bias=use_bias, hyperkernel_activation=hk_act,
                hyperbias_use_bias=False)
    x = rng.standard_normal((B,) + S + (cin,)).astype(F)
    hyp = rng.standard_normal((B, H)).astype(F)
    O = S if padding == 'same' else tuple(s - 2 for s in S)
    w = rng.standard_normal((B,) + O + (cout,)).astype(F)
    xg, hg = G(x, dev, True), G(hyp, dev, True)
    y = layer([xg, hg])
    assert tuple(y.shape) == (B,) + O + (cout,)
    names = sorted(n for n, _ in layer.named_parameters())
    assert names == sorted(['hyperkernel_kernel', 'hyperkernel_bias'] + (['hyperbias_kernel'] if use_bias else []))
    assert all(t.device.type == 'cuda' for t in layer.parameters())
    (y * G(w, dev)).sum().backward()

    def conv(xo, dense, p):
        kern = dense('hyperkernel', hk_act, (3,) * rank + (cin, cout))
        bias = dense('hyperbias', None, (cout,)) if use_bias else None
        x5, k6 = (xo, kern) if rank == 3 else (xo[:, None], kern[:, None])
        ys = [tuo.conv3d_same(x5[b:b + 1], k6[b], None if bias is None else bias[b], 1, act, padding=padding) for b in range(B)]
        yo = torch.cat(ys, 0)
        return yo if rank == 3 else yo[:, 0]
    yo, grads = _from_dense_reference(layer, x, hyp, w, conv)
    close(N(y), yo, 'forward', 1e-4)
    close(N(xg.grad), grads['x'], 'grad_x')
    close(N(hg.grad), grads['hyp'], 'grad_hyp')
    for n, t in layer.named_parameters():
        close(N(t.grad), grads[n], 'grad_' + n)


def test_hyperdense_from_dense(dev):
    rng = np.random.default_rng(8)
    H, cin, units, lead = 4, 16, 12, (6, 10)
    layer = L.HyperDenseFromDense(units, activation='elu', hyperbias_activation='tanh')
    x = rng.standard_normal((B,) + lead + (cin,)).astype(F)
    hyp = rng.standard_normal((B, H)).astype(F)
    w = rng.standard_normal((B,) + lead + (units,)).astype(F)
    xg, hg = G(x, dev, True), G(hyp, dev, True)
    y = layer([xg, hg])
    (y * G(w, dev)).sum().backward()
    assert sorted(n for n, _ in layer.named_parameters()) == ['hyperbias_bias', 'hyperbias_kernel', 'hyperkernel_bias', 'hyperkernel_kernel']

    def dense_op(xo, dense, p):
        kern, bias = dense('hyperkernel', None, (cin, units)), dense('hyperbias', 'tanh', (units,))
        return _ref_act(torch.einsum('b...i,biu->b...u', xo, kern) + bias[:, None, None, :], 'elu')
    yo, grads = _from_dense_reference(layer, x, hyp, w, dense_op)
    close(N(y), yo, 'forward', 1e-4)
    close(N(xg.grad), grads['x'], 'grad_x')
    close(N(hg.grad), grads['hyp'], 'grad_hyp')
    for n, t in layer.named_parameters():
        close(N(t.grad), grads[n], 'grad_' + n)


def test_training_step_under_graph_capture(dev):
    """forward and backward of a HyperConv3D captured as one hipGraph: a replay recomputes from the current contents of its input
    buffers (the layers allocate from torch's allocator and launch on the current stream)"""
    from test_gpu_graph_capture import capture
    cin, cout, shape = 16, 16, (8, 8, 16)
    ks, kern, bias, x, w, _ = _case(cin, cout, 3, 1, shape, 'same', 2)
    layer = L.HyperConv3D(cout, 3, padding='same', activation='elu')
    xg, kg, bg, wg = G(x, dev, True), G(kern, dev, True), G(bias, dev, True), G(w, dev)

    def step():
        y = layer([xg, kg, bg])
        gx, gk, gb = torch.autograd.grad((y * wg).sum(), [xg, kg, bg])
        return y.detach(), gx, gk, gb
    g, outs = capture(step)
    rng = np.random.default_rng(4)
    for _ in range(2):
        with torch.no_grad():
            xg.copy_(G(rng.standard_normal(x.shape).astype(F), dev))
            kg.copy_(G((rng.standard_normal(kern.shape) * 0.05).astype(F), dev))
            bg.copy_(G(rng.standard_normal(bias.shape).astype(F), dev))
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])        # no atomics
        close(N(got[2]), N(want[2]), 'grad_kernel under replay')
        close(N(got[3]), N(want[3]), 'grad_bias under replay')
        yo, gxo, gko, gbo = _reference(N(xg), N(kg), N(bg), w, 1, 'elu', 'same')
        _check_per_entry(got[0], got[1], got[2], got[3], yo, gxo, gko, gbo)


def test_tensors_on_a_device_that_is_not_current():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip('one visible device')
    other = torch.device('cuda:1')
    assert torch.cuda.current_device() == 0
    cin, cout, shape = 16, 16, (8, 8, 16)
    ks, kern, bias, x, w, _ = _case(cin, cout, 3, 1, shape, 'same', 6)
    y, gx, gk, gb = _run_layer(other, x, kern, bias, w, ks, 1, 'elu', 'same')
    assert y.device == other and torch.cuda.current_device() == 0
    yo, gxo, gko, gbo = _reference(x, kern, bias, w, 1, 'elu', 'same')
    _check_per_entry(y, gx, gk, gb, yo, gxo, gko, gbo)
