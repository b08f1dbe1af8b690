"""
GPU tests of the bfloat16 inference path of models.ConvNet (csrc/conv_bf16.hip).

Numerics under test (models.py module docstring): every kernel computes in float32 from the stored bf16 values and rounds its
result to bf16 once, round-to-nearest-even.  A convolution output is therefore checked ELEMENT-WISE against the float64
convolution of the exact bf16 operands (x^, w^, b^):

    |got - act(ref)| <= 2^-8 |act(ref)| + 9 * 2^-24 * S  (+ 3e-6 for ELU, the hardware exponential),   S = sum |x^ w^| + |b^|

2^-8 relative is the half-ulp of round-to-nearest-even to bf16 (a truncating conversion breaks it); the S term is the float32
accumulation.  Whole networks are compared end to end with the oracles evaluated in float64 on the bf16-rounded weights and input
(relative RMS and relative max error, `e2e_errors`); the tolerances E2E_TOL are at most 4x the worst case measured on MI355X.
"""

import contextlib
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import models as nm
from oracle import c_oracle as co
from oracle import keras_graph_oracle as kgo
from oracle import unet_oracle as uo

pytestmark = pytest.mark.gpu
F = np.float32
BF = torch.bfloat16

# end-to-end tolerances (relative RMS, relative max): measured worst cases on MI355X 0.0054 (two_d_pool) and 0.0144 (res_dil_1conv)
E2E_TOL = (0.02, 0.05)


def bfr(a):
    """float32 array of the bf16 values nearest to a (round-to-nearest-even)"""
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(BF).float().numpy()


def GB(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(dev).to(BF)


def N(t):
    return t.detach().float().cpu().numpy()


def act_np(v, act):
    if act == 'elu':
        return uo.elu(v)
    if act == 'relu':
        return np.maximum(v, 0)
    return v


def conv_refs(x, w, b, dil, padding):
    """float64 reference of one batch entry x [X, Y, Z, C] and the sum of absolute terms S; VALID = the SAME output cropped"""
    ref = co.conv3d_same(x, w, b, dilation=dil).astype(np.float64)
    absref = co.conv3d_same(np.abs(x), np.abs(w), np.abs(b), dilation=dil).astype(np.float64)
    if padding == 'valid':
        k = w.shape[:3]
        sl = tuple(slice((kk - 1) * dil // 2, (kk - 1) * dil // 2 + x.shape[d] - (kk - 1) * dil) for d, kk in enumerate(k))
        ref, absref = ref[sl], absref[sl]
    return ref, absref


def check_layer(got, ref, absref, act):
    """the element-wise bound of the module docstring; returns the worst error / bound"""
    want = act_np(ref, act)
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = 2.0 ** -8 * np.abs(want) + 9 * 2.0 ** -24 * absref + (3e-6 if act == 'elu' else 0.0) + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, 'error %.3f x the bf16 bound' % worst
    return worst


def e2e_errors(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = got - ref
    return float(np.sqrt((d ** 2).sum() / max((ref ** 2).sum(), 1e-300))), float(np.abs(d).max() / max(np.abs(ref).max(), 1e-300))


def check_e2e(got, ref, tol=E2E_TOL):
    rms, mx = e2e_errors(got, ref)
    assert rms <= tol[0] and mx <= tol[1], 'end-to-end relative RMS %.3g (tol %.3g), relative max %.3g (tol %.3g)' % (rms, tol[0], mx, tol[1])
    return rms, mx


def set_weights(conv, rng):
    k = conv.kernel.shape
    fan = int(np.prod(k[:-1]))
    w = (rng.standard_normal(k) / np.sqrt(fan)).astype(F)
    b = (rng.standard_normal(k[-1]) * 0.1).astype(F)
    with torch.no_grad():
        conv.kernel.copy_(torch.from_numpy(w))
        conv.bias.copy_(torch.from_numpy(b))


def _randomise(model, rng):
    for name, m in model.layers_by_name.items():
        if isinstance(m, nm._Conv):
            set_weights(m, rng)
        else:
            C = m.gamma.shape[0]
            p = [(1 + 0.1 * rng.standard_normal(C)), 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C), 1 + 0.1 * rng.random(C)]
            with torch.no_grad():
                for t, v in zip((m.gamma, m.beta, m.moving_mean, m.moving_variance), p):
                    t.copy_(torch.from_numpy(v.astype(F)))


def bf16_params(model):
    """({conv: (kernel, bias)}, {bn: (gamma, beta, mean, var)}) as float32 arrays of the model's bf16 values"""
    ws, bns = {}, {}
    for name, m in model.layers_by_name.items():
        if isinstance(m, nm._Conv):
            ws[name] = (N(m.kernel), N(m.bias))
        else:
            bns[name] = [N(m.gamma), N(m.beta), N(m.moving_mean), N(m.moving_variance)]
    return ws, bns


def check_layers(model, xs_dev, expect_convs=None):
    """every convolution of a bf16 model against the float64 convolution of the bf16 tensors the GPU itself produced"""
    names = [op['name'] for op in model.ops]
    with torch.no_grad():
        t = model(xs_dev, return_tensors=names)
    for v in t.values():
        assert v.dtype == BF
    nd = model.ndims
    worst, n = 0.0, 0
    for op in model.ops:
        if op['kind'] not in ('conv', 'likelihood'):
            continue
        m = model.layers_by_name[op['name']]
        src = t[op['merge']] if op.get('lo') else t[op['src']]
        x = N(nm._lift(src, nd))
        got = N(nm._lift(t[op['name']], nd))
        k, b = N(m.kernel), N(m.bias)
        for bi in range(x.shape[0]):
            ref, absref = conv_refs(x[bi], k, b, m.dilation, m.padding)
            worst = max(worst, check_layer(got[bi], ref, absref, m.activation))
        n += 1
    if expect_convs is not None:
        assert n == expect_convs
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# per-layer convolution
# ---------------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # the shapes of test_gpu_unet.py::test_conv3d_mfma_vs_oracle
    (16, 16, (9, 7, 21), (3, 3, 3), 1, 'same', 'elu'), (48, 16, (8, 8, 32), (3, 3, 3), 1, 'same', 'elu'),
    (32, 64, (6, 10, 17), (3, 3, 3), 1, 'same', None), (16, 32, (12, 5, 16), (3, 3, 3), 2, 'same', 'elu'),
    (24, 5, (7, 9, 18), (3, 3, 3), 1, 'same', 'relu'), (16, 40, (5, 6, 19), (1, 3, 3), 1, 'same', 'elu'),
    (64, 16, (4, 4, 16), (1, 1, 1), 1, 'same', None), (8, 16, (10, 10, 10), (3, 3, 3), 1, 'same', 'elu'),
    # Cin = 1 (one k-step), odd Cin, VALID, dilation 2 and 4, a (2, 2, 2) kernel, Cout > 64, a (1, 3, 5) kernel
    (1, 16, (12, 11, 20), (3, 3, 3), 1, 'same', 'elu'), (3, 5, (9, 8, 7), (3, 3, 3), 1, 'valid', 'elu'),
    (12, 8, (9, 10, 11), (3, 3, 3), 2, 'valid', None), (4, 4, (14, 13, 12), (3, 3, 3), 4, 'same', 'elu'),
    (5, 3, (6, 6, 9), (2, 2, 2), 1, 'same', 'elu'), (16, 8, (6, 7, 18), (2, 2, 2), 1, 'valid', 'relu'),
    (2, 70, (6, 7, 8), (3, 3, 3), 1, 'same', 'elu'), (16, 130, (5, 4, 17), (1, 1, 1), 1, 'same', None),
    (8, 6, (1, 12, 20), (1, 3, 5), 1, 'same', 'elu'), (40, 24, (8, 8, 8), (3, 3, 3), 2, 'same', 'elu'),
]


@pytest.mark.parametrize('cin,cout,shape,k,dil,pad,act', CONV_CASES)
def test_conv3d_bf16_vs_oracle(dev, cin, cout, shape, k, dil, pad, act):
    rng = np.random.default_rng(cin * 1000 + cout + dil)
    conv = nm._Conv('c', cin, cout, k, dil, pad, act)
    set_weights(conv, rng)
    conv = conv.to(dev, BF).eval()
    x = bfr(rng.standard_normal((2,) + shape + (cin,)))
    with torch.no_grad():
        y = conv(GB(x, dev))
    assert y.dtype == BF
    y = N(y)
    w, b = N(conv.kernel), N(conv.bias)
    for bi in range(2):
        ref, absref = conv_refs(x[bi], w, b, dil, pad)
        assert y[bi].shape == ref.shape
        check_layer(y[bi], ref, absref, act)


@pytest.mark.parametrize('c0,c1,cout,S,up', [(32, 64, 32, (8, 12, 16), (2, 2, 2)), (16, 32, 16, (10, 6, 18), (2, 2, 2)),
                                             (8, 24, 16, (6, 6, 12), (1, 2, 3)), (4, 12, 7, (6, 6, 6), (2, 2, 2))])
def test_conv3d_bf16_fused_upsample_concat(dev, c0, c1, cout, S, up):
    rng = np.random.default_rng(c0 + 7 * c1)
    conv = nm._Conv('c', c0 + c1, cout, (3, 3, 3), 1, 'same', 'elu')
    set_weights(conv, rng)
    conv = conv.to(dev, BF).eval()
    skip = bfr(rng.standard_normal((2,) + S + (c0,)))
    lo = bfr(rng.standard_normal((2,) + tuple(s // u for s, u in zip(S, up)) + (c1,)))
    with torch.no_grad():
        y = N(conv(GB(skip, dev), lo=GB(lo, dev), up=up))
    w, b = N(conv.kernel), N(conv.bias)
    for bi in range(2):
        xin = np.concatenate([skip[bi], uo.upsample(lo[bi], up)], -1)
        ref, absref = conv_refs(xin, w, b, 1, 'same')
        check_layer(y[bi], ref, absref, 'elu')


def test_conv3d_bf16_rounds_to_nearest_even(dev):
    """1 + 3 * 2^-9 (exact in float32) lies 3/4 of the way from 1 to the next bf16 value 1 + 2^-7: nearest rounding gives
    1 + 2^-7, truncation would give 1"""
    conv = nm._Conv('c', 2, 16, (1, 1, 1), 1, 'same', None).to(dev, BF).eval()
    with torch.no_grad():
        conv.kernel.fill_(1.0)
        conv.bias.zero_()
        x = torch.tensor([1.0, 3 * 2.0 ** -9], device=dev).to(BF).reshape(1, 1, 1, 1, 2).expand(1, 2, 2, 16, 2).contiguous()
        y = N(conv(x))
    assert np.all(y == 1.0 + 2.0 ** -7)


# ---------------------------------------------------------------------------------------------------------------------
# glue kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_glue_kernels_bf16(dev):
    rng = np.random.default_rng(4)
    for C in (5, 16):
        x = bfr(rng.standard_normal((2, 9, 8, 7, C)))
        for pool in ((2, 2, 2), (3, 1, 2), (1, 2, 4)):
            got = N(nm._maxpool(GB(x, dev), pool, 'same'))
            for b in range(2):
                assert np.array_equal(got[b], uo.maxpool_same(x[b], pool))
            gotv = N(nm._maxpool(GB(x, dev), pool, 'valid'))
            ox, oy, oz = [s // p for s, p in zip(x.shape[1:4], pool)]
            ref = x[:, :ox * pool[0], :oy * pool[1], :oz * pool[2]].reshape(2, ox, pool[0], oy, pool[1], oz, pool[2], C).max((2, 4, 6))
            assert np.array_equal(gotv, ref)
    for c0, c1, up in ((16, 32, (2, 2, 2)), (3, 5, (1, 2, 3)), (0, 8, (2, 1, 2))):
        lo = bfr(rng.standard_normal((2, 3, 4, 2, c1)))
        S = [s * u for s, u in zip(lo.shape[1:4], up)]
        skip = bfr(rng.standard_normal([2] + S + [c0])) if c0 else None
        got = N(nm._upsample_concat(GB(skip, dev) if c0 else None, GB(lo, dev), up))
        for b in range(2):
            want = uo.upsample(lo[b], up) if not c0 else np.concatenate([skip[b], uo.upsample(lo[b], up)], -1)
            assert np.array_equal(got[b], want)
    rel = 2.0 ** -8
    for C in (6, 16):
        a, b2 = bfr(rng.standard_normal((2, 4, 4, 4, C))), bfr(rng.standard_normal((2, 4, 4, 4, C)))
        sc, sh = rng.standard_normal(C).astype(F), rng.standard_normal(C).astype(F)
        for got, want in ((nm._elementwise(GB(a, dev), GB(b2, dev), act=1), uo.elu(a.astype(np.float64) + b2)),
                          (nm._elementwise(GB(a, dev), scale=G32(sc, dev), shift=G32(sh, dev)), a.astype(np.float64) * sc + sh),
                          (nm._elementwise(GB(a, dev), act=3), 1 / (1 + np.exp(-a.astype(np.float64)))),
                          (nm._elementwise(GB(a, dev), GB(b2, dev), mul=True), a.astype(np.float64) * b2),
                          (nm._elementwise(GB(a, dev), GB(b2, dev)), a.astype(np.float64) + b2)):
            assert got.dtype == BF
            err = np.abs(N(got) - want)
            assert np.all(err <= rel * np.abs(want) + 4e-7 * (1 + np.abs(want))), float(err.max())
    for C in (33, 16, 8):
        z = bfr(rng.standard_normal((3, 11, 13, C)) * 4)
        e = np.exp(z.astype(np.float64) - z.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        y = N(nm._softmax(GB(z, dev)))
        assert np.all(np.abs(y - p) <= rel * p + 1e-6)
        assert np.all(np.abs(y.astype(np.float64).sum(-1) - 1) <= rel + 1e-6)
    for cin, cout in ((16, 32), (16, 4), (7, 50)):
        k = bfr(rng.standard_normal((1, 1, 1, cin, cout)) / np.sqrt(cin))
        bb = bfr(rng.standard_normal(cout))
        xin = bfr(rng.standard_normal((2, 5, 6, 7, cin)))
        lin = xin.astype(np.float64) @ k.reshape(cin, cout).astype(np.float64) + bb
        S = np.abs(xin.astype(np.float64)) @ np.abs(k.reshape(cin, cout)) + np.abs(bb)
        got = N(nm._conv1x1_softmax(GB(xin, dev), GB(k, dev), GB(bb, dev), False))
        assert np.all(np.abs(got - lin) <= rel * np.abs(lin) + 9 * 2.0 ** -24 * S)
        e = np.exp(lin - lin.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        got = N(nm._conv1x1_softmax(GB(xin, dev), GB(k, dev), GB(bb, dev), True))
        assert np.all(np.abs(got - p) <= rel * p + 1e-6)


def G32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
SMALL = [
    (dict(nb_features=8, nb_levels=3, conv_size=3, nb_labels=6, feat_mult=2), (24, 20, 28, 1), {}),
    (dict(nb_features=8, nb_levels=3, conv_size=3, nb_labels=4, feat_mult=2, nb_conv_per_level=2), (16, 16, 24, 2), {}),
    (dict(nb_features=8, nb_levels=2, conv_size=3, nb_labels=3, feat_mult=2, nb_conv_per_level=2, use_residuals=True,
          batch_norm=-1, conv_dropout=0.2), (12, 16, 20, 2), dict(use_residuals=True)),
    (dict(nb_features=16, nb_levels=3, conv_size=3, nb_labels=5, feat_mult=1, final_pred_activation='linear'), (16, 24, 1), {}),
]


@pytest.mark.parametrize('case', range(len(SMALL)))
def test_unet_small_configs_bf16(dev, case):
    kw, ishape, okw = SMALL[case]
    rng = np.random.default_rng(11 + case)
    model = ne.models.unet(input_shape=ishape, **kw)
    _randomise(model, rng)
    model = model.to(dev, BF)
    x = bfr(rng.standard_normal((2,) + ishape))
    with torch.no_grad():
        y = model(GB(x, dev))
    assert y.dtype == BF and y.shape == (2,) + ishape[:-1] + (kw['nb_labels'],)
    y = N(y)
    weights, bns = bf16_params(model)
    nd = len(ishape) - 1
    for b in range(2):
        xb = x[b].reshape((1,) * (3 - nd) + ishape)
        ref = uo.unet_forward(xb, weights, kw['nb_levels'], kw.get('nb_conv_per_level', 1), pool=(1,) * (3 - nd) + (2,) * nd,
                              bn_params=bns or None, final_pred_activation=kw.get('final_pred_activation', 'softmax'), **okw)
        print('e2e small %d: rms %.3g max %.3g' % ((case,) + e2e_errors(y[b].reshape(ref.shape), ref)))
        check_e2e(y[b].reshape(ref.shape), ref)
    print('layers small %d: worst %.3f of the bound' % (case, check_layers(model, GB(x, dev))))


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unet_graph.json')) as _f:
    REF_GRAPHS = json.load(_f)

GRAPH_TAGS = ['res_dil', 'res_dil_1conv', 'res_same_feats', 'layer_nb_feats', 'list_of_lists', 'bn_dropout_res', 'dropout_plain',
              'prior_logp', 'prior_p', 'multi_input', 'two_d_pool', 'one_d', 'valid_enc', 'enc_default', 'enc_res_dil', 'dec_alone',
              'dec_alone_res', 'dilation_net']


@pytest.mark.parametrize('tag', GRAPH_TAGS)
def test_recorded_graph_bf16(dev, tag):
    case = REF_GRAPHS[tag]
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        warnings.simplefilter('ignore')
        model = getattr(ne.models, case['builder'])(*case['args'], **case['kwargs'])
    rng = np.random.default_rng(sum(map(ord, tag)))
    _randomise(model, rng)
    model = model.to(dev, BF)
    nd = model.ndims
    xs = [rng.standard_normal((2,) + tuple(s)).astype(F) for s in model.input_shapes]
    if tag.startswith('prior'):
        xs[1] = np.log(np.abs(xs[1]) + 0.1).astype(F) if tag == 'prior_logp' else np.abs(xs[1])
    xs = [bfr(x) for x in xs]
    xd = [GB(x, dev) for x in xs] if len(xs) > 1 else GB(xs[0], dev)
    with torch.no_grad():
        y = model(xd)
    assert y.dtype == BF
    y = N(y)
    weights, bns = bf16_params(model)
    wk = {n: (k.reshape(k.shape[3 - nd:]), b) for n, (k, b) in weights.items()}
    for b in range(2):
        ref = kgo.run(case['graph'], [x[b] for x in xs], wk, bns or None)
        assert y[b].shape == ref.shape
        print('e2e %s: rms %.3g max %.3g' % ((tag,) + e2e_errors(y[b], ref)))
        check_e2e(y[b], ref)
    print('layers %s: worst %.3f of the bound' % (tag, check_layers(model, xd)))


def test_unet_cfg3_bf16(dev):
    """config 3 at full size: the layer-wise bound on the five convolutions; the prediction's argmax agrees with the float32 model on
    >= 99 % of the voxels where float32's top-two margin exceeds 0.05"""
    rng = np.random.default_rng(5)
    model = ne.models.unet(16, (160, 160, 160, 1), 3, 3, 32, feat_mult=2)
    _randomise(model, rng)
    model = model.to(dev).eval()
    x = np.random.default_rng(4).standard_normal((1, 160, 160, 160, 1)).astype(F)
    with torch.no_grad():
        p32 = model(G32(x, dev))
        model.bfloat16()
        p16 = model(G32(x, dev))                     # the input op casts to bf16
    assert p16.dtype == BF
    top2 = torch.topk(p32, 2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 0.05
    agree = (p32.argmax(-1) == p16.float().argmax(-1))[sure].float().mean().item()
    print('cfg3 argmax agreement %.5f on %d voxels, max |dp| %.4f' % (agree, int(sure.sum()), float((p16.float() - p32).abs().max())))
    assert agree >= 0.99
    del p32, p16, top2, sure
    convs = ['unet_conv_downarm_0_0', 'unet_conv_downarm_1_0', 'unet_conv_downarm_2_0', 'unet_conv_uparm_3_0', 'unet_conv_uparm_4_0']
    names = convs + ['unet_maxpool_0', 'unet_maxpool_1', 'unet_merge_3', 'unet_merge_4']
    with torch.no_grad():
        t = model(GB(bfr(x), dev), return_tensors=names + ['unet_input'])
    src = {'unet_conv_downarm_0_0': 'unet_input', 'unet_conv_downarm_1_0': 'unet_maxpool_0', 'unet_conv_downarm_2_0': 'unet_maxpool_1',
           'unet_conv_uparm_3_0': 'unet_merge_3', 'unet_conv_uparm_4_0': 'unet_merge_4'}
    for n in convs:
        m = model.layers_by_name[n]
        ref, absref = conv_refs(N(t[src[n]])[0], N(m.kernel), N(m.bias), 1, 'same')
        print('cfg3 %s: worst %.3f of the bound' % (n, check_layer(N(t[n])[0], ref, absref, m.activation)))


# ---------------------------------------------------------------------------------------------------------------------
# contract: float32 unchanged, refusals, cache, determinism, graph capture
# ---------------------------------------------------------------------------------------------------------------------
def _small_unet(dev, dtype=None, seed=3):
    model = ne.models.unet(8, (16, 16, 24, 1), 3, 3, 5, feat_mult=2)
    _randomise(model, np.random.default_rng(seed))
    return model.to(dev) if dtype is None else model.to(dev, dtype)


def test_float32_model_ignores_input_dtype(dev):
    model = _small_unet(dev)
    x = torch.from_numpy(bfr(np.random.default_rng(1).standard_normal((2, 16, 16, 24, 1)))).to(dev)
    with torch.no_grad():
        y32 = model(x)
        y16 = model(x.to(BF))
    assert y32.dtype == torch.float32 and y16.dtype == torch.float32
    assert torch.equal(y32, y16)


def test_refusals_before_launch(dev):
    x = torch.randn(1, 16, 16, 24, 1, device=dev)
    model = _small_unet(dev, BF).train()
    with pytest.raises(NotImplementedError, match='inference'):
        model(x)
    half = _small_unet(dev, torch.float16)
    with pytest.raises(NotImplementedError, match='unet_conv_downarm_0_0'):
        half(x)
    mixed = _small_unet(dev, BF)
    mixed.get_layer('unet_conv_uparm_3_0').float()
    with pytest.raises(NotImplementedError, match='unet_conv_uparm_3_0'):
        mixed(x)
    conv = nm._Conv('c', 4, 8, (3, 3, 3)).to(dev, BF)
    f32, b16 = torch.zeros(8, device=dev), torch.zeros(8, device=dev, dtype=BF)
    with pytest.raises(NotImplementedError):
        nm._elementwise(f32, b16)                                       # a bf16 buffer never reaches an _f32 entry point
    with pytest.raises(NotImplementedError):
        nm._elementwise(b16, f32)                                       # nor a float32 one a _bf16 entry point
    with pytest.raises(NotImplementedError):
        nm._elementwise(b16, scale=b16[:1], shift=b16[:1])              # scale and shift are float32 for both
    with pytest.raises(NotImplementedError):
        nm._elementwise(torch.zeros(8, device=dev, dtype=torch.float16))    # no kernel family takes any other dtype
    with pytest.raises(NotImplementedError):
        conv._run(torch.zeros(1, 4, 4, 4, 4, device=dev))
    torch.cuda.synchronize()


def test_weight_cache_and_determinism(dev):
    model = _small_unet(dev, BF)
    x = GB(bfr(np.random.default_rng(2).standard_normal((2, 16, 16, 24, 1))), dev)
    with torch.no_grad():
        y0 = model(x)
        y1 = model(x)
    assert torch.equal(y0, y1)
    conv = model.get_layer('unet_conv_uparm_3_0')
    with torch.no_grad():
        conv.kernel.copy_(conv.kernel * -1)                       # in place: _version moves
        y2 = model(x)
    assert not torch.equal(y2, y0)
    fresh = _small_unet(dev, BF)
    fresh.get_layer('unet_conv_uparm_3_0').kernel.data.mul_(-1)
    with torch.no_grad():
        assert torch.equal(y2, fresh(x))
    sd = _small_unet(dev, BF, seed=9).state_dict()
    model.load_state_dict(sd)
    other = _small_unet(dev, BF, seed=9)
    with torch.no_grad():
        assert torch.equal(model(x), other(x))


def test_graph_capture_bf16(dev):
    model = _small_unet(dev, BF)
    x = GB(bfr(np.random.default_rng(6).standard_normal((2, 16, 16, 24, 1))), dev)
    with torch.no_grad():
        eager = model(x)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            model(x)                                                  # warm-up: weights packed outside the capture
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = model(x)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)
