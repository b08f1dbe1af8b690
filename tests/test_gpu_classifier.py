"""
models.design_dnn / models.EncoderNet on the device against a float64 torch-CPU restatement of the RECORDED Keras graphs
(tests/golden/classifier_graph.json, evaluated by Keras class in `ref_layer` below), at their recorded sizes.

Inference is compared LAYER BY LAYER: every reference layer is fed the device's own input to that layer, so each layer is held to its
own bound and nothing accumulates (u = 2^-24):
    Conv{1,2,3}D    the criterion of tests/test_gpu_unet.py on the pre-activation: |err| <= 8 u S, S = |b| + sum |x| |w| (+ 3e-6 behind the
                    elu of the epilogue; + 8 u behind a sigmoid: slope <= 1/4, float32 exp, add and divide of a value <= 1)
    Dense           |err| <= (in + 2) u S, the order-free bound of tests/test_gpu_dense.py (+ 8 u behind a sigmoid; behind a softmax
                    twice the row's largest pre-activation bound -- the softmax is 1/2-Lipschitz per logit -- plus the rtol 2e-5 /
                    atol 2e-7 of the softmax kernel's own tests)
    MaxPooling, GlobalMaxPooling3D, the flatten-then-max Lambda, Flatten, Reshape, Dropout (inference)      bit-exact
    Add, RescaleValues     bit-exact against the float32 expression
    Activation      elu: 8 u (1 + |ref|) (float32 exp of a value <= 1, minus 1); softmax: rtol 2e-5, atol 2e-7
    BatchNorm       (inference) |err| <= 8 u (|x scale| + |beta| + |mean scale|): scale and shift are formed in float32 first
Training compares the gradient of a scalar loss with respect to every parameter and the input with float64 autograd through the same
evaluator, the element-wise dropout masks replayed from `net.last_dropout_masks`: 2e-4 of the gradient's largest magnitude per layer,
the criterion of the conv backward tests.  Then ConvNet.apply_constraints (MaxNorm) and the weight files.
"""

import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from neurite_amd import models

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, 'golden', 'classifier_graph.json')) as f:
    GRAPHS = {k: v for k, v in json.load(f).items() if not k.startswith('__') and 'graph' in v}


def _build(tag, **override):
    case = GRAPHS[tag]
    kwargs = dict(case['kwargs'])
    kwargs.update(override)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return getattr(models, case['builder'])(*case['args'], **kwargs)


def _tensor_names(net, ref):
    """{recorded layer name: the network's tensor name}: the same, except the Dropout layers Keras numbered itself"""
    mine = [op['name'] for op in net.ops if op['kind'] == 'dropout_ew' and op.get('auto_name')]
    theirs = [l['name'] for l in ref['layers'] if l['class'] == 'Dropout' and l['name'] not in net.layer_names]
    assert len(mine) == len(theirs)
    out = {l['name']: l['name'] for l in ref['layers']}
    out.update(dict(zip(theirs, mine)))
    return out


def _params(net, grad=False):
    out = {}
    for (name, _, _), a in zip(net._weight_tensors(), net.get_weights()):
        out[name] = torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad and not name.endswith(('moving_mean', 'moving_variance')))
    return out


def _randomise(net, seed):
    rng = np.random.default_rng(seed)
    ws = []
    for (name, _, _), w in zip(net._weight_tensors(), net.get_weights()):
        if name.endswith('moving_variance') or name.endswith('gamma'):
            ws.append(rng.uniform(0.5, 1.5, w.shape).astype(np.float32))
        elif name.endswith('/kernel') and w.ndim >= 2:
            ws.append((rng.standard_normal(w.shape) / np.sqrt(np.prod(w.shape[:-1]))).astype(np.float32))
        else:
            ws.append((0.3 * rng.standard_normal(w.shape)).astype(np.float32))
    net.set_weights(ws)
    return ws


def _act(v, name):
    if name in (None, 'linear'):
        return v
    if name == 'elu':
        return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0)))
    if name == 'relu':
        return torch.clamp(v, min=0)
    if name == 'sigmoid':
        return torch.sigmoid(v)
    raise NotImplementedError(name)


def _conv_pre(x, w, b, cfg):
    """Keras Conv{nd}D, channels last, stride 1, before the activation: 'same' pads (k - 1) d // 2 before, the rest after"""
    nd = len(cfg['kernel_size'])
    xin = x.movedim(-1, 1)
    if cfg['padding'] == 'same':
        pads = []
        for d in reversed(range(nd)):
            tot = (cfg['kernel_size'][d] - 1) * cfg['dilation_rate'][d]
            pads += [tot // 2, tot - tot // 2]
        xin = TF.pad(xin, pads)
    wt = w.permute(nd + 1, nd, *range(nd))
    return getattr(TF, 'conv%dd' % nd)(xin, wt, b, dilation=tuple(cfg['dilation_rate'])).movedim(1, -1)


def ref_layer(layer, t, P, eps, train=False, masks=None):
    """float64 value of a recorded Keras layer from the tensors `t` of the layers before it.  Returns (value, bound info)."""
    cls, name, cfg = layer['class'], layer['name'], layer['config']
    x = t[layer['inputs'][0]]
    if cls.startswith('Conv'):
        assert cfg['strides'] == [1] * len(cfg['strides']) and cfg['use_bias']
        w, b = P[name + '/kernel'], P[name + '/bias']
        pre = _conv_pre(x, w, b, cfg)
        with torch.no_grad():
            S = _conv_pre(x.abs(), w.abs(), b.abs(), cfg)
        extra = {'elu': 3e-6, 'sigmoid': 8 * U}.get(cfg['activation'], 0.0)
        return _act(pre, cfg['activation']), ('abs', 8 * U * S + extra)
    if cls == 'Dense':
        w, b = P[name + '/kernel'], P[name + '/bias']
        pre = x @ w + b
        with torch.no_grad():
            bound = (w.shape[0] + 2) * U * (x.abs() @ w.abs() + b.abs())
        if cfg['activation'] == 'softmax':
            y = torch.softmax(pre, -1)
            return y, ('abs', 2 * bound.max(-1, keepdim=True).values + 2e-5 * y.detach() + 2e-7)
        return _act(pre, cfg['activation']), ('abs', bound + (8 * U if cfg['activation'] == 'sigmoid' else 0.0))
    if cls == 'Dropout':
        if train:
            return x * masks[name].reshape(x.shape), ('none',)
        return x, ('exact',)
    if cls.startswith('MaxPooling'):
        nd = len(cfg['pool_size'])
        assert cfg['strides'] == cfg['pool_size'] and all(s % p == 0 for s, p in zip(x.shape[1:-1], cfg['pool_size']))
        return getattr(TF, 'max_pool%dd' % nd)(x.movedim(-1, 1), tuple(cfg['pool_size'])).movedim(1, -1), ('exact',)
    if cls == 'GlobalMaxPooling3D':
        return torch.amax(x, dim=(1, 2, 3)), ('exact',)
    if cls == 'Lambda':
        assert cfg['function'] == [['batch_flatten'], ['max', 1, True]]
        return torch.amax(x.reshape(x.shape[0], -1), dim=1, keepdim=True), ('exact',)
    if cls == 'Flatten':
        return x.reshape(x.shape[0], -1), ('exact',)
    if cls == 'Reshape':
        return x.reshape((x.shape[0],) + tuple(cfg['target_shape'])), ('exact',)
    if cls == 'RescaleValues':
        return x * cfg['resize'], ('f32', lambda: x.float() * np.float32(cfg['resize']))
    if cls == 'Add':
        a, b = t[layer['inputs'][0]], t[layer['inputs'][1]]
        return a + b, ('f32', lambda: a.float() + b.float())
    if cls == 'Activation':
        if cfg['activation'] == 'softmax':
            return torch.softmax(x, -1), ('softmax',)
        y = _act(x, cfg['activation'])
        return y, ('abs', 8 * U * (1 + y.detach().abs()))
    if cls == 'BatchNormalization':
        assert cfg['axis'] in (-1, x.dim() - 1)
        g, b = P[name + '/gamma'], P[name + '/beta']
        if train:
            axes = tuple(range(x.dim() - 1))
            mean, var = x.mean(axes), x.var(axes, unbiased=False)
        else:
            mean, var = P[name + '/moving_mean'], P[name + '/moving_variance']
        scale = g / torch.sqrt(var + cfg['epsilon'])
        return x * scale + (b - mean * scale), ('abs', 8 * U * ((x * scale).abs() + b.abs() + (mean * scale).abs()))
    raise NotImplementedError(cls)


def _check(name, got, ref, info):
    err = (got.double() - ref).abs()
    how = info[0]
    if how == 'exact':
        assert torch.equal(got, ref.float()), name
    elif how == 'f32':
        assert torch.equal(got, info[1]()), name
    elif how == 'abs':
        worst = float((err / (info[1] + 1e-300)).max())
        print('%-36s %.3f of the bound' % (name, worst))
        assert bool((err <= info[1]).all()), '%s: %.3g x the bound' % (name, worst)
    elif how == 'softmax':
        np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=2e-5, atol=2e-7, err_msg=name)
    else:
        raise AssertionError(how)


def _input(net, batch, seed):
    return torch.randn((batch,) + tuple(net.input_shapes[0]), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('tag', sorted(GRAPHS))
def test_forward_layer_by_layer(dev, tag):
    net, ref = _build(tag), GRAPHS[tag]['graph']
    _randomise(net, 1)
    net.to(dev).eval()
    x = _input(net, 2, 2)
    alias = _tensor_names(net, ref)
    with torch.no_grad():
        out = net(x.to(dev), return_tensors=list(net.layer_names))
    got = {k: out[v].cpu() for k, v in alias.items()}
    P = _params(net)
    classes = set()
    for layer in ref['layers']:
        name = layer['name']
        assert list(got[name].shape[1:]) == layer['output_shape'][1:], name
        if layer['class'] == 'InputLayer':
            assert torch.equal(got[name], x), name
            continue
        t = {k: v.double() for k, v in got.items()}              # the device's own inputs to this layer
        want, info = ref_layer(layer, t, P, None)
        assert tuple(got[name].shape) == tuple(want.shape), (name, got[name].shape, want.shape)
        _check(name, got[name], want, info)
        classes.add(layer['class'])
    final = net(x.to(dev))
    assert torch.equal(final.cpu(), got[ref['outputs'][0]])
    assert classes


TRAIN_TAGS = ['dnn_dense_sigmoid', 'dnn_dropout', 'dnn_dense_softmax', 'dnn_globalmaxpooling', 'dnn_myglobalmaxpooling_bn_last',
              'dnn_unknown_final', 'dnn_maxpool', 'dnn_pool_221', 'dnn_2d_dense_sigmoid', 'enc_dropout', 'enc_rescale',
              'enc_regression', 'enc_residuals', 'enc_batch_norm']


@pytest.mark.parametrize('tag', TRAIN_TAGS)
def test_training_step_gradients(dev, tag):
    net, ref = _build(tag), GRAPHS[tag]['graph']
    _randomise(net, 40)
    net.to(dev).train()
    x = _input(net, 3, 41)
    alias = _tensor_names(net, ref)
    dx = x.to(dev).requires_grad_(True)
    y = net(dx)
    r = torch.randn(y.shape, generator=torch.Generator().manual_seed(42))
    (y * r.to(dev)).sum().backward()
    drops = [l['name'] for l in ref['layers'] if l['class'] == 'Dropout']
    masks = {k: net.last_dropout_masks[alias[k]].cpu().double() for k in drops}
    for k, m in masks.items():                                   # a mask is 0 or 1 / (1 - rate), one draw per element
        rate = next(l for l in ref['layers'] if l['name'] == k)['config']['rate']
        vals = set(np.unique(m.numpy()).tolist())
        assert vals <= {0.0, float(np.float32(1.0) / np.float32(1.0 - rate))} and len(vals) == 2, (k, vals)
    # float64 autograd through the recorded graph
    P = _params(net, grad=True)
    rx = x.double().requires_grad_(True)
    t = {}
    for layer in ref['layers']:
        if layer['class'] == 'InputLayer':
            t[layer['name']] = rx
        else:
            t[layer['name']], _ = ref_layer(layer, t, P, None, train=True, masks=masks)
    yr = t[ref['outputs'][0]]
    np.testing.assert_allclose(y.detach().cpu().double().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-5 * float(yr.abs().max()))
    (yr * r.double()).sum().backward()
    layer_scale = {}                                             # the largest gradient magnitude among a layer's variables
    for name in P:
        if P[name].grad is not None:
            layer = name.rsplit('/', 1)[0]
            layer_scale[layer] = max(layer_scale.get(layer, 0.0), float(P[name].grad.abs().max()))
    checked = 0
    for name, p, _ in net._weight_tensors():
        if name.endswith(('moving_mean', 'moving_variance')):
            continue
        assert p.grad is not None, name
        got, want = p.grad.cpu().double().reshape(P[name].shape), P[name].grad
        scale = layer_scale[name.rsplit('/', 1)[0]]
        assert scale > 0, name
        worst = float((got - want).abs().max()) / scale
        print('%-40s grad error %.2e of scale' % (name, worst))
        assert worst <= 2e-4, '%s: %.3g of the gradient scale' % (name, worst)
        checked += 1
    assert checked >= 4
    scale = float(rx.grad.abs().max())
    assert float((dx.grad.cpu().double() - rx.grad).abs().max()) <= 2e-4 * scale
    # inference draws nothing
    net.eval()
    with torch.no_grad():
        assert torch.equal(net(x.to(dev)), net(x.to(dev)))


def _maxnorm64(w, m, eps=1e-7):
    w = np.asarray(w, np.float64)
    n = np.sqrt((w * w).sum(0, keepdims=True))
    return w * (np.clip(n, 0, m) / (eps + n))


def _constraint_kernel(shape, m, rng):
    """a kernel whose axis-0 norms lie below, at and above m, with one column of zeros.  The norms below m are kept at 1 and 1.5:
    the formula itself moves a column by eps / (eps + n) per application, which is within 4 * 2^-24 only for n >= 0.42 -- a second
    application can be idempotent to that bound for no smaller norm, whatever computes it"""
    w = rng.standard_normal(shape).astype(np.float32)
    flat = w.reshape(shape[0], -1)
    cols = flat.shape[1]
    flat /= np.sqrt((flat.astype(np.float64) ** 2).sum(0, keepdims=True)).astype(np.float32)
    flat[:, 1::4] *= np.float32(16.0)                            # above; columns 0, 4, ... stay at 1 (below)
    flat[:, 2::4] *= np.float32(1.5)
    flat[:, 3::4] *= np.float32(1.5)
    flat[:, 2] = 0.0
    flat[0, 2] = m                                               # exactly at max_value
    flat[:, 3] = 0.0                                             # a zero column
    assert cols >= 8
    return flat.reshape(shape)


def test_apply_constraints_maxnorm(dev):
    m = 2
    net = models.design_dnn(8, (8, 8, 8), 2, 3, 2, conv_maxnorm=m).to(dev).eval()
    ws = _randomise(net, 3)
    rng = np.random.default_rng(4)
    names = [n for n, _, _ in net._weight_tensors()]
    constrained = [n for n, mod in net.layers_by_name.items() if getattr(mod, 'max_norm', None)]
    assert len(constrained) == 6 and all(net.layers_by_name[n].max_norm == m for n in constrained)
    for n in constrained:
        k = names.index(n + '/kernel')
        ws[k] = _constraint_kernel(ws[k].shape, m, rng)
    net.set_weights(ws)
    x = _input(net, 2, 5).to(dev)
    with torch.no_grad():
        before = net(x).clone()                                  # packs the weights of the matrix-core layers
    net.apply_constraints()
    got = net.get_weights()
    for n in names:
        k = names.index(n)
        if n.endswith('/kernel') and n.rsplit('/', 1)[0] in constrained:
            want = _maxnorm64(ws[k], m)
            err = np.abs(got[k].astype(np.float64) - want)
            assert np.all(np.isfinite(got[k]))
            assert np.all(err <= 4 * U * np.abs(want)), (n, float((err / (np.abs(want) + 1e-300)).max()) / U)
            flat = got[k].reshape(got[k].shape[0], -1)
            assert np.all(flat[:, 3] == 0.0)                     # the zero column stays zero
            norms = np.sqrt((flat.astype(np.float64) ** 2).sum(0))
            assert np.all(norms <= m * (1 + 4 * U))
        else:
            assert np.array_equal(got[k], ws[k]), n                # nothing else moves
    with torch.no_grad():
        after = net(x)
    assert not torch.equal(before, after)
    fresh = models.design_dnn(8, (8, 8, 8), 2, 3, 2, conv_maxnorm=m)
    fresh.set_weights(got)
    fresh.to(dev).eval()
    with torch.no_grad():
        assert torch.equal(after, fresh(x)), 'a packed copy of the unconstrained kernel survived apply_constraints'
    # idempotent to within the same bound
    net.apply_constraints()
    again = net.get_weights()
    for a, b in zip(again, got):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 4 * U * np.abs(b))


def test_apply_constraints_in_a_graph_and_without_constraints(dev):
    plain = _build('dnn_dense_sigmoid').to(dev)
    ws = _randomise(plain, 6)
    plain.apply_constraints()
    for a, b in zip(plain.get_weights(), ws):
        assert np.array_equal(a, b)
    net = _build('dnn_maxnorm').to(dev)
    ws = [w * np.float32(6.0) for w in _randomise(net, 7)]
    net.set_weights(ws)
    eager = _build('dnn_maxnorm').to(dev)
    eager.set_weights(ws)
    eager.apply_constraints()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.apply_constraints()
    net.set_weights(ws)                                          # whatever the capture did or did not run: start from the same weights
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(net.get_weights(), eager.get_weights()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('ext', ['npz', 'h5'])
@pytest.mark.parametrize('tag', ['dnn_myglobalmaxpooling_bn_last', 'enc_rescale'])
def test_weight_files_round_trip_bit_for_bit(dev, tag, ext, tmp_path):
    net = _build(tag).to(dev)
    ws = _randomise(net, 70)
    other = _build(tag).to(dev)
    _randomise(other, 71)
    path = str(tmp_path / ('w.' + ext))
    net.save_weights(path)
    x = _input(net, 2, 72).to(dev)
    with torch.no_grad():
        before = other(x).clone()
        other.load_weights(path)
        assert not torch.equal(before, other(x)) and torch.equal(other(x), net(x))
    for a, b in zip(other.get_weights(), ws):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
