"""
models.single_ae / models.ae on the device against a float64 torch-CPU evaluation of the same op list (`ref_op` below).

Inference is compared LAYER BY LAYER: every reference layer is fed the device's own input to that layer, so each layer is held to its
own bound and nothing accumulates:
    Conv           the criterion of tests/test_gpu_unet.py: |err| <= 8 u S (+ 3e-6 behind elu), S = |b| + sum |x| |w|, and 1e-5 relative
                   on outputs with S <= 25 |ref|                                                          (u = 2^-24)
    Dense          |err| <= (in + 2) u S, the order-free bound of tests/test_gpu_dense.py
    LocalBias      bit-exact: x + kernel in float32
    Flatten, Reshape, Lambda(identity), UpSampling, MaxPooling, Add    bit-exact
    Resize         bit-exact against oracle.np_oracle.resize_layer, as tests/test_gpu_interpn.py
    sampling       |err| <= 4 u (|mu| + |exp(lv / 2) noise|), the noise injected
    BatchNorm      (inference) |err| <= 8 u (|x scale| + |beta| + |mean scale|): scale and shift are formed in float32 first
    softmax        rtol 2e-5, atol 2e-7, as the head tests of tests/test_gpu_unet.py
Training compares the gradient of a scalar loss with respect to every parameter and the input with float64 autograd through the same
evaluator (noise fixed): 2e-4 of the gradient's largest magnitude, the criterion of the conv and HyperConv backward tests; the
magnitude is taken over the variables of a layer together, because a bias in front of a training-mode batch norm has a gradient that
is exactly zero and no scale of its own.

`single_ae((2, 2, 2, None), (4, 4, 4, 3), ae_type='conv')` does not exist: with differing spatial sizes the reference takes the
Resize branch and builds Conv3D(filters=None) (neurite/tf/models.py:506-513), which fails; tests/test_ae_abi.py pins that.  The
pass-through branch is reached with equal spatial sizes, (4, 4, 4, None), which is what runs here.  The default batch_norm=True is
axis 1, which is not the last axis of a [B, 4, 4, 4, 3] tensor; the single_ae cases pass batch_norm=None or -1.
"""

import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from neurite_amd import models
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = torch.float64


def _quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*args, **kwargs)


def _params(net, dtype=F64, grad=False):
    """{layer/variable: Keras-shaped tensor}"""
    out = {}
    for (name, _, _), a in zip(net._weight_tensors(), net.get_weights()):
        out[name] = torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad and not name.endswith(('moving_mean', 'moving_variance')))
    return out


def _act(v, name):
    if name in (None, 'linear'):
        return v
    if name == 'elu':
        return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0)))
    if name == 'relu':
        return torch.clamp(v, min=0)
    raise NotImplementedError(name)


def _conv_pre(x, w, b, nd, dilation, padding):
    """Keras Conv{nd}D, channels last, stride 1, before the activation"""
    xin = x.movedim(-1, 1)
    wt = w.permute(nd + 1, nd, *range(nd))
    y = getattr(TF, 'conv%dd' % nd)(xin, wt, b, padding=padding, dilation=dilation)
    return y.movedim(1, -1)


def ref_op(net, op, t, P, train=False, noise=None):
    """float64 value of layer `op` from the tensors `t` of the layers before it (Keras shapes).  Returns (value, bound info)."""
    kind, name, nd = op['kind'], op['name'], net.ndims
    if kind in ('conv', 'likelihood'):
        m = net.layers_by_name[name]
        x = t[op['src']]
        pre = _conv_pre(x, P[name + '/kernel'], P[name + '/bias'], nd, m.dilation, m.padding)
        with torch.no_grad():
            S = _conv_pre(x.abs(), P[name + '/kernel'].abs(), P[name + '/bias'].abs(), nd, m.dilation, m.padding)
        return _act(pre, m.activation), ('conv', pre, S, m.activation)
    if kind == 'dense':
        x, w, b = t[op['src']], P[name + '/kernel'], P[name + '/bias']
        with torch.no_grad():
            S = x.abs() @ w.abs() + b.abs()
        return x @ w + b, ('dense', (w.shape[0] + 2) * U * S)
    if kind in ('identity', 'dropout'):
        return t[op['src']], ('exact',)
    if kind == 'lambda':
        return op['fn'](t[op['src']]), ('ulp', 8)
    if kind == 'flatten':
        return t[op['src']].reshape(t[op['src']].shape[0], -1), ('exact',)
    if kind == 'reshape':
        sp, c = op['shape']
        return t[op['src']].reshape((-1,) + tuple(sp[3 - nd:]) + (c,)), ('exact',)
    if kind == 'maxpool':
        pool = tuple(op['pool'][3 - nd:])
        x = t[op['src']]
        assert all(s % p == 0 for s, p in zip(x.shape[1:-1], pool))
        return getattr(TF, 'max_pool%dd' % nd)(x.movedim(-1, 1), pool).movedim(1, -1), ('exact',)
    if kind == 'upsample':
        x = t[op['src']]
        for d, u in enumerate(op['up'][3 - nd:]):
            x = x.repeat_interleave(int(u), dim=1 + d)
        return x, ('exact',)
    if kind == 'local_bias':
        return t[op['src']] + P[name + '/kernel'], ('f32', lambda: t[op['src']].float() + P[name + '/kernel'].float())
    if kind == 'add':
        return t[op['a']] + t[op['b']], ('f32', lambda: t[op['a']].float() + t[op['b']].float())
    if kind == 'resize':
        x = t[op['src']]
        if train:                                             # differentiable form: align-corners linear interpolation
            mode = {1: 'linear', 2: 'bilinear', 3: 'trilinear'}[nd]
            size = [int(s * z) for s, z in zip(x.shape[1:-1], op['zoom'])]
            return TF.interpolate(x.movedim(-1, 1), size=size, mode=mode, align_corners=True).movedim(1, -1), ('none',)
        zf = [float(z) for z in op['zoom']]
        return torch.from_numpy(npo.resize_layer(x.float().numpy(), zf)).double(), ('exact',)
    if kind == 'sample':
        mu, lv = t[op['a']], t[op['b']]
        p = torch.exp(lv / 2) * noise[name].reshape(mu.shape)
        return mu + p, ('abs', 4 * U * (mu.abs() + p.abs()))
    if kind == 'bn':
        m = net.layers_by_name[name]
        x = t[op['src']]
        g, b = P[name + '/gamma'], P[name + '/beta']
        if train:
            axes = tuple(range(x.dim() - 1))
            mean, var = x.mean(axes), x.var(axes, unbiased=False)
        else:
            mean, var = P[name + '/moving_mean'], P[name + '/moving_variance']
        scale = g / torch.sqrt(var + m.epsilon)
        return x * scale + (b - mean * scale), ('abs', 8 * U * ((x * scale).abs() + b.abs() + (mean * scale).abs()))
    if kind == 'prediction':
        x = t[op['src']]
        if op['activation'] == 'softmax':
            return torch.softmax(x, -1), ('softmax',)
        return _act(x, op['activation']), ('exact',)
    raise NotImplementedError(kind)


def _check(name, got, ref, info):
    got64 = got.double()
    err = (got64 - ref).abs()
    how = info[0]
    if how == 'exact':
        assert torch.equal(got, ref.float()), name
    elif how == 'f32':
        assert torch.equal(got, info[1]()), name
    elif how == 'conv':
        _, pre, S, act = info
        bound = 8 * U * S + (3e-6 if act == 'elu' else 0.0) + 1e-30
        worst = float((err / bound).max())
        print('%-32s conv   %.2f of the bound' % (name, worst))
        assert worst <= 1.0, '%s: %.2f x the float32 dot-product bound' % (name, worst)
        if act in (None, 'linear'):
            well = S <= 25.0 * pre.abs()
            assert bool(well.any()), name
            assert float((err[well] / pre.abs()[well]).max()) <= 1e-5, name
    elif how == 'dense':
        worst = float((err / (info[1] + 1e-300)).max())
        print('%-32s dense  %.3f of the bound' % (name, worst))
        assert bool((err <= info[1]).all()), '%s: %.3g x the bound' % (name, worst)
    elif how == 'abs':
        worst = float((err / (info[1] + 1e-300)).max())
        print('%-32s        %.3f of the bound' % (name, worst))
        assert bool((err <= info[1]).all()), '%s: %.3g x the bound' % (name, worst)
    elif how == 'ulp':
        assert bool((err <= info[1] * U * ref.abs() + 1e-30).all()), name
    elif how == 'softmax':
        np.testing.assert_allclose(got64.numpy(), ref.numpy(), rtol=2e-5, atol=2e-7, err_msg=name)
    else:
        raise AssertionError(how)


def _inputs(net, batch, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((batch,) + tuple(s), generator=g) for s in net.input_shapes]
    for op in net.ops:                                           # a log-prior input: log-probabilities
        if op['kind'] == 'input' and op['name'].endswith('prior-input'):
            xs[op['index']] = torch.log_softmax(xs[op['index']], -1)
    return xs


def _noise(net, batch, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for op in net.ops:
        if op['kind'] == 'sample':
            sp, c = op['shape']
            out[op['name']] = torch.randn((batch,) + tuple(sp) + (c,), generator=g)
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


def _layer_by_layer(net, dev, batch=2, seed=0):
    _randomise(net, seed + 1)
    net.to(dev).eval()
    xs, noise = _inputs(net, batch, seed + 2), _noise(net, batch, seed + 3)
    names = list(net.layer_names)
    with torch.no_grad():
        out = net([x.to(dev) for x in xs], return_tensors=names, _noise={k: v.to(dev) for k, v in noise.items()})
    got = {k: v.cpu() for k, v in out.items()}
    P = _params(net)
    kinds = set()
    for op in net.ops:
        name = op['name']
        if op['kind'] == 'input':
            assert torch.equal(got[name], xs[op['index']]), name
            continue
        t = {k: v.double() for k, v in got.items()}              # the device's own inputs to this layer
        ref, info = ref_op(net, op, t, P, noise={k: v.double() for k, v in noise.items()})
        assert tuple(got[name].shape) == tuple(ref.shape), (name, got[name].shape, ref.shape)
        _check(name, got[name], ref, info)
        kinds.add(op['kind'])
    final = net([x.to(dev) for x in xs], _noise={k: v.to(dev) for k, v in noise.items()})
    # the forward that materialises nothing it does not need ends in the same values
    np.testing.assert_allclose(final.cpu().numpy(), got[net.output_name].numpy(), rtol=1e-5, atol=1e-6)
    return kinds


def test_single_ae_dense_vae_with_shift_layers(dev):
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), do_vae=True, include_mu_shift_layer=True, batch_norm=None)
    kinds = _layer_by_layer(net, dev, batch=3)
    assert {'flatten', 'dense', 'local_bias', 'identity', 'sample', 'reshape'} <= kinds
    for v in (1, 2):                                             # both arms of the forward, through the model
        net.dense_variant = v
        _layer_by_layer(net, dev, batch=3, seed=10 * v)


def test_single_ae_dense_flat_input_default_batch_norm(dev):
    net = _quiet(models.single_ae, [5], (12,), do_vae=True)
    assert 'bn' in _layer_by_layer(net, dev, batch=17)           # a second batch chunk of the dense kernels


@pytest.mark.parametrize('enc_size', [(2, 2, 2, 4), (4, 4, 4, None)], ids=['resize', 'pass_through'])
def test_single_ae_conv(dev, enc_size):
    net = _quiet(models.single_ae, enc_size, (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=None, do_vae=True)
    kinds = _layer_by_layer(net, dev)
    assert ('resize' in kinds) == (enc_size[-1] is not None)


@pytest.mark.parametrize('single', [False, True], ids=['tuple', 'single_model'])
def test_ae_2d_dense(dev, single):
    res = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense', single_model=single)
    if single:
        assert {'conv', 'maxpool', 'flatten', 'dense', 'reshape', 'upsample', 'likelihood', 'prediction'} <= _layer_by_layer(res, dev)
        return
    dec, mid, enc = res
    for k, net in enumerate((enc, mid, dec)):
        _layer_by_layer(net, dev, seed=20 + k)
    # the three stacked give what the chained model gives from the same weights
    one = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense', single_model=True)
    one.set_weights(enc.get_weights() + mid.get_weights() + dec.get_weights())
    one.to(dev)
    x = _inputs(enc, 2, 5)[0].to(dev)
    assert torch.equal(dec(mid(enc(x))), one(x))


def test_ae_3d_vae_with_prior(dev):
    net = _quiet(models.ae, 2, (4, 4, 4, 1), 2, 3, 2, (2, 2, 2, 3), do_vae=True, add_prior_layer=True, single_model=True)
    assert len(net.input_shapes) == 2
    assert {'sample', 'add', 'prediction'} <= _layer_by_layer(net, dev)


def _train_case(net, dev, batch, seed):
    _randomise(net, seed)
    net.to(dev).train()
    xs, noise = _inputs(net, batch, seed + 1), _noise(net, batch, seed + 2)
    dx = [x.to(dev).requires_grad_(True) for x in xs]
    y = net(dx, _noise={k: v.to(dev) for k, v in noise.items()})
    r = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 3))
    (y * r.to(dev)).sum().backward()
    # float64 autograd through the same op list
    P = _params(net, grad=True)
    rx = [x.double().requires_grad_(True) for x in xs]
    t = {}
    for op in net.ops:
        if op['kind'] == 'input':
            t[op['name']] = rx[op['index']]
        else:
            t[op['name']], _ = ref_op(net, op, t, P, train=True, noise={k: v.double() for k, v in noise.items()})
    yr = t[net.output_name]
    np.testing.assert_allclose(y.detach().cpu().double().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-5 * float(yr.abs().max()))
    (yr * r.double()).sum().backward()
    checked = 0
    layer_scale = {}                                             # the largest gradient magnitude among a layer's variables
    for name in P:
        if P[name].grad is not None:
            layer = name.rsplit('/', 1)[0]
            layer_scale[layer] = max(layer_scale.get(layer, 0.0), float(P[name].grad.abs().max()))
    for name, p, _ in net._weight_tensors():
        if name.endswith(('moving_mean', 'moving_variance')):
            continue
        assert p.grad is not None, name
        got, ref = p.grad.cpu().double().reshape(P[name].shape), P[name].grad
        scale = layer_scale[name.rsplit('/', 1)[0]]
        assert scale > 0, name
        worst = float((got - ref).abs().max()) / scale
        print('%-40s grad error %.2e of scale' % (name, worst))
        assert worst <= 2e-4, '%s: %.3g of the gradient scale' % (name, worst)
        checked += 1
    for a, b in zip(dx, rx):
        scale = float(b.grad.abs().max())
        assert float((a.grad.cpu().double() - b.grad).abs().max()) <= 2e-4 * scale
    return checked


def test_training_gradients_dense_vae(dev):
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), do_vae=True, include_mu_shift_layer=True, batch_norm=None)
    assert _train_case(net, dev, batch=5, seed=40) == 8


def test_training_gradients_flat_input_batch_norm(dev):
    """Dense -> BatchNormalization in training mode: the exact gradient of a bias in front of a batch norm is zero (the batch mean is
    subtracted), so a layer's variables share the layer's gradient scale (see _train_case)"""
    net = _quiet(models.single_ae, [5], (12,), do_vae=True)
    assert _train_case(net, dev, batch=17, seed=45) == 12


def test_training_gradients_conv_resize_vae(dev):
    net = _quiet(models.single_ae, (2, 2, 2, 4), (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=None, do_vae=True,
                 activation='elu')
    assert _train_case(net, dev, batch=2, seed=50) == 6


def test_training_gradients_ae_chain(dev):
    net = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense', single_model=True, do_vae=True)
    _train_case(net, dev, batch=3, seed=60)


def test_load_weights_from_h5_changes_the_forward(dev, tmp_path):
    """nothing packed or cached survives load_weights: the forward after it is that of the file's weights"""
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=None, include_mu_shift_layer=True).to(dev)
    other = _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=None, include_mu_shift_layer=True)
    _randomise(net, 70)
    _randomise(other, 71)
    path = str(tmp_path / 'ae_weights.h5')
    other.save_weights(path)
    x = _inputs(net, 2, 72)[0].to(dev)
    before = net(x).clone()
    net.load_weights(path)
    after = net(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, other.to(dev)(x))
    for a, b in zip(net.get_weights(), other.get_weights()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_dense_single_ae_under_graph_capture(dev):
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=None).to(dev)
    _randomise(net, 80)
    x = _inputs(net, 2, 81)[0].to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        net(x)                                                   # workspace growth and lazy allocations: outside the capture
        net(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = net(x)
    x.copy_(_inputs(net, 2, 82)[0])                              # the replay must recompute from the buffer's current contents
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, net(x))
