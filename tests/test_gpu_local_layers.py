"""
GPU tests of the per-voxel parameter layers and the stream layers (csrc/local.hip; neurite/tf/layers.py:746-808, 1535-1607,
1711-1844, 1915-2073).  Every reference is a NumPy restatement of the cited lines written here: float32 in the reference's op order
where the result must agree bit for bit (the affine family, CovStream's first call with one entry), float64 on the same float32
inputs elsewhere, with the project's sum rule as the bound -- a float32 result that is `s` times a sum of n rounded terms lies within

    (n + 5) * 2^-24 * |s| * sum_i |term_i|

of the exact value, whatever the order of summation (n roundings of the sum to first order, + 5 for the few further roundings of
alpha, the scale and the division).  The stream layers are checked call by call: the float64 step starts from the state the layer
held before the call (float32 inputs of that call), the first state being zeros, and `count` must be exact throughout.
"""

import warnings

import numpy as np
import pytest
import torch

import neurite_amd as ne
from conftest import bits_equal

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
F32 = np.float32
SHAPES = [((5, 6, 7), 3), ((9, 10), 1), ((17,), 2), ((33, 17, 9), 4)]       # 630, 90, 34 (no multiple of 4) and 20196 floats per entry


def within(got, exact, bound, what):
    err = np.abs(np.asarray(got, np.float64) - exact)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print('%s: worst error / bound = %.3f' % (what, worst))
    assert np.all(err <= bound), '%s: error up to %.3f of the bound' % (what, worst)


def gpu(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_() if grad else t


def host(t):
    return t.detach().cpu().numpy()


def set_param(p, a):
    with torch.no_grad():
        p.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(p.device))


def pwi(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return ne.layers.LocalParamWithInput(*args, **kwargs)


# ----------------------------------------------------------------------------------------------------------------------------------
# 1 + 2: the affine family
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,C', SHAPES)
@pytest.mark.parametrize('B', [1, 3])
def test_affine_family_forward_is_bit_exact(dev, S, C, B):
    rng = np.random.default_rng(hash((S, C, B)) % (2 ** 31))
    shape = tuple(S) + (C,)
    x = rng.standard_normal((B,) + shape).astype(F32)
    k = rng.standard_normal(shape).astype(F32)
    m = rng.standard_normal(shape).astype(F32)
    xd = gpu(x, dev)
    with torch.no_grad():
        for biasmult in (1.0, 0.37):
            layer = ne.layers.LocalBias(biasmult=biasmult)
            layer(xd)
            assert tuple(layer.kernel.shape) == shape and layer.kernel.is_cuda
            set_param(layer.kernel, k)
            assert bits_equal(host(layer(xd)), x + k * F32(biasmult)), 'LocalBias biasmult %g' % biasmult          # :771
        layer = ne.layers.LocalLinear()
        layer(xd)
        set_param(layer.mult, m)
        set_param(layer.bias, k)
        assert bits_equal(host(layer(xd)), x * m + k), 'LocalLinear'                                               # :805
        for mult in (1.0, 2.5):
            layer = ne.layers.LocalParamLayer(shape, mult=mult, device=dev)
            set_param(layer.kernel, k)
            out = layer()
            assert tuple(out.shape) == (1,) + shape
            assert bits_equal(host(out), k[None] * F32(mult)), 'LocalParamLayer mult %g' % mult                    # :1761
            layer = pwi(shape, mult=mult)
            other = rng.standard_normal((B, 4, 3)).astype(F32)                      # the input only lends its batch size
            layer(gpu(other, dev))
            set_param(layer.kernel, k)

            def want(inp):                                                           # :1837-1841
                b = inp.reshape(B, -1)[:, 0:1] * np.zeros((1,), F32) + np.ones((1,), F32)
                params = (k * F32(mult)).reshape(1, -1)
                return (b * params).reshape((-1,) + shape)                           # K.dot over the single inner element
            out = layer(gpu(other, dev))
            assert tuple(out.shape) == (B,) + shape
            assert bits_equal(host(out), want(other)), 'LocalParamWithInput mult %g' % mult
            view = gpu(np.concatenate([other, other], -1), dev)[..., 3:]             # a view: only the batch stride is used
            assert bits_equal(host(layer(view)), want(other)), 'LocalParamWithInput on a view'
            if B > 1:
                bad = other.copy()
                bad.reshape(B, -1)[1, 0] = np.inf
                with np.errstate(invalid='ignore'):
                    w = want(bad)
                got = host(layer(gpu(bad, dev)))
                assert np.all(np.isnan(got[1])) and bits_equal(got, w)
                assert bits_equal(got[0], want(other)[0]) and bits_equal(got[2], want(other)[2])


@pytest.mark.parametrize('S,C', SHAPES)
@pytest.mark.parametrize('B', [1, 3])
def test_affine_family_backward(dev, S, C, B):
    rng = np.random.default_rng(1000 + hash((S, C, B)) % (2 ** 31))
    shape = tuple(S) + (C,)
    x = rng.standard_normal((B,) + shape).astype(F32)
    k = rng.standard_normal(shape).astype(F32)
    m = rng.standard_normal(shape).astype(F32)
    w = rng.standard_normal((B,) + shape).astype(F32)
    w64 = w.astype(np.float64)
    wd = gpu(w, dev)

    def grads(layer, params, inp):
        out = []
        for _ in range(2):
            for p in params:
                p.grad = None
            xd = None if inp is None else gpu(inp, dev, grad=True)
            y = layer() if inp is None else layer(xd)
            (y * wd[:y.shape[0]]).sum().backward()
            out.append([None if xd is None or xd.grad is None else host(xd.grad)] + [host(p.grad) for p in params])
        for a, b in zip(out[0], out[1]):
            assert (a is None and b is None) or bits_equal(a, b), 'two runs differ'
        return out[0]

    for biasmult in (1.0, 0.37):
        layer = ne.layers.LocalBias(biasmult=biasmult)
        layer(gpu(x, dev))
        set_param(layer.kernel, k)
        gx, gk = grads(layer, [layer.kernel], x)
        assert bits_equal(gx, w)
        within(gk, float(F32(biasmult)) * w64.sum(0), (B + 5) * EPS * abs(float(F32(biasmult))) * np.abs(w64).sum(0),
               'LocalBias d kernel')
    layer = ne.layers.LocalLinear()
    layer(gpu(x, dev))
    set_param(layer.mult, m)
    set_param(layer.bias, k)
    gx, gm, gb = grads(layer, [layer.mult, layer.bias], x)
    assert bits_equal(gx, w * m)                                                     # one multiply
    within(gm, (w64 * x).sum(0), (B + 5) * EPS * np.abs(w64 * x).sum(0), 'LocalLinear d mult')
    within(gb, w64.sum(0), (B + 5) * EPS * np.abs(w64).sum(0), 'LocalLinear d bias')
    # the input gradient alone (frozen parameters), and the parameter gradients alone
    layer.mult.requires_grad_(False)
    layer.bias.requires_grad_(False)
    xd = gpu(x, dev, grad=True)
    (layer(xd) * wd).sum().backward()
    assert bits_equal(host(xd.grad), w * m) and layer.mult.grad is not None
    for mult in (1.0, 2.5):
        layer = ne.layers.LocalParamLayer(shape, mult=mult, device=dev)
        set_param(layer.kernel, k)
        _, gk = grads(layer, [layer.kernel], None)
        within(gk, mult * w64[0], 6 * EPS * mult * np.abs(w64[0]), 'LocalParamLayer d kernel')
        layer = pwi(shape, mult=mult)
        other = rng.standard_normal((B, 5)).astype(F32)
        layer(gpu(other, dev))
        set_param(layer.kernel, k)
        gx, gk = grads(layer, [layer.kernel], other)
        assert gx is None                                                            # the input gets no gradient
        within(gk, mult * w64.sum(0), (B + 5) * EPS * mult * np.abs(w64).sum(0), 'LocalParamWithInput d kernel')


# ----------------------------------------------------------------------------------------------------------------------------------
# 3: LocalCrossLinear
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout', [(1, 1), (1, 5), (3, 4), (5, 3), (8, 8), (16, 32), (33, 2), (64, 64)])
def test_cross_linear_forward_and_gradients(dev, cin, cout):
    rng = np.random.default_rng(100 * cin + cout)
    for S in ((5, 6, 7), (9, 10), (17,)):
        if (cin, cout) == (64, 64) and S != (5, 6, 7):
            continue
        W = rng.normal(1.0 / cin, 0.01, (1,) + S + (cin, cout)).astype(F32)          # the default initializer (:1567-1570)
        bias = rng.normal(1.0 / cin, 0.01, (1,) + S + (cout,)).astype(F32)
        W64, b64 = W.astype(np.float64)[0], bias.astype(np.float64)[0]
        for B in (1, 3, 5):
            x = rng.standard_normal((B,) + S + (cin,)).astype(F32)
            g = rng.standard_normal((B,) + S + (cout,)).astype(F32)
            x64, g64 = x.astype(np.float64), g.astype(np.float64)
            for use_bias in (True, False):
                tag = 'cross linear %d->%d %s B=%d bias=%s' % (cin, cout, S, B, use_bias)
                layer = ne.layers.LocalCrossLinear(cout, use_bias=use_bias)
                with torch.no_grad():
                    layer(gpu(x, dev))
                assert tuple(layer.mult.shape) == W.shape and (layer.bias is None) == (not use_bias)
                set_param(layer.mult, W)
                if use_bias:
                    set_param(layer.bias, bias)
                runs = []
                for _ in range(2):
                    for p in layer.parameters():
                        p.grad = None
                    xd = gpu(x, dev, grad=True)
                    y = layer(xd)
                    (y * gpu(g, dev)).sum().backward()
                    runs.append([host(y), host(xd.grad), host(layer.mult.grad)] + ([host(layer.bias.grad)] if use_bias else []))
                for a, b in zip(runs[0], runs[1]):
                    assert bits_equal(a, b), tag + ': two runs differ'
                y, gx, gW = runs[0][:3]
                want = np.einsum('b...c,...co->b...o', x64, W64)
                mag = np.einsum('b...c,...co->b...o', np.abs(x64), np.abs(W64))
                if use_bias:
                    want, mag = want + b64, mag + np.abs(b64)
                within(y, want, (cin + 1 + 5) * EPS * mag, tag + ' y')
                within(gx, np.einsum('b...o,...co->b...c', g64, W64),
                       (cout + 5) * EPS * np.einsum('b...o,...co->b...c', np.abs(g64), np.abs(W64)), tag + ' gx')
                within(gW[0], np.einsum('b...c,b...o->...co', x64, g64),
                       (B + 5) * EPS * np.einsum('b...c,b...o->...co', np.abs(x64), np.abs(g64)), tag + ' gW')
                if use_bias:
                    within(runs[0][3][0], g64.sum(0), (B + 5) * EPS * np.abs(g64).sum(0), tag + ' gbias')
            with torch.no_grad():                           # the plain launch path gives the numbers of the recorded one
                assert bits_equal(host(layer(gpu(x, dev))), runs[0][0])


def test_cross_linear_equals_locally_connected_1x1x1(dev):
    """the same layer on another kernel: LocallyConnected3D(cout, 1), implementation 1 -- kernel [positions, cin, cout]"""
    rng = np.random.default_rng(77)
    S, cin, cout, B = (5, 6, 7), 3, 4, 3
    W = rng.normal(1.0 / cin, 0.01, (1,) + S + (cin, cout)).astype(F32)
    bias = rng.normal(1.0 / cin, 0.01, (1,) + S + (cout,)).astype(F32)
    x = rng.standard_normal((B,) + S + (cin,)).astype(F32)
    with torch.no_grad():
        cross = ne.layers.LocalCrossLinear(cout)
        cross(gpu(x, dev))
        set_param(cross.mult, W)
        set_param(cross.bias, bias)
        lc = ne.layers.LocallyConnected3D(cout, 1)
        lc(gpu(x, dev))
        set_param(lc.kernel, W.reshape(-1, cin, cout))
        set_param(lc.bias, bias[0])
        a, b = host(cross(gpu(x, dev))), host(lc(gpu(x, dev)))
    mag = np.einsum('b...c,...co->b...o', np.abs(x.astype(np.float64)), np.abs(W.astype(np.float64)[0])) + np.abs(bias.astype(np.float64))
    # each side lies within the sum-rule bound of the exact value
    within(a, b.astype(np.float64), 2 * (cin + 1 + 5) * EPS * mag, 'LocalCrossLinear against LocallyConnected3D')


# ----------------------------------------------------------------------------------------------------------------------------------
# 4: MeanStream
# ----------------------------------------------------------------------------------------------------------------------------------
def mean_step64(mean, count, x, cap):
    """_mean_update (:2059-2073) and the output scale (:1972) in float64; also the terms' magnitudes for the sum rule"""
    B = x.shape[0]
    x64 = x.astype(np.float64)
    new_count = count + B
    alpha = B / min(new_count, cap)
    new_mean = mean * (1 - alpha) + (x64.sum(0) / B) * alpha
    mag = np.abs(mean * (1 - alpha)) + np.abs(x64 * alpha / B).sum(0)
    return new_mean, new_count, alpha, min(1.0, new_count / cap), mag


def check_mean_stream(dev, cap, B, shape, seed):
    rng = np.random.default_rng(seed)
    layer = ne.layers.MeanStream(cap=cap)
    layer.train()
    count = 0
    for call in range(3):
        x = rng.standard_normal((B,) + shape).astype(F32) + F32(0.5)
        before = None if call == 0 else host(layer.mean).astype(np.float64)
        if call == 0:
            before = np.zeros(shape)
        new_mean, new_count, alpha, scale, mag = mean_step64(before, float(count), x, cap)
        if call == 1:                                   # the gradient of the second call
            xd = gpu(x, dev, grad=True)
            y = layer(xd)
            g = rng.standard_normal((B,) + shape).astype(F32)
            (y * gpu(g, dev)).sum().backward()
            g64 = g.astype(np.float64)
            coef = scale * alpha / B
            want = np.broadcast_to(coef * g64.sum(0), g64.shape)
            within(host(xd.grad), want, (B + 1 + 5) * EPS * abs(coef) * np.broadcast_to(np.abs(g64).sum(0), g64.shape),
                   'MeanStream gx (cap %g)' % cap)
        else:
            with torch.no_grad():
                y = layer(gpu(x, dev))
        count += B
        assert float(layer.count) == float(count) and tuple(layer.count.shape) == (1,)
        within(host(layer.mean), new_mean, (B + 1 + 5) * EPS * mag, 'MeanStream mean, call %d (cap %g)' % (call, cap))
        within(host(y), np.broadcast_to(scale * new_mean, y.shape), (B + 1 + 5) * EPS * scale * np.broadcast_to(mag, y.shape),
               'MeanStream y, call %d (cap %g)' % (call, cap))
    return layer, rng, count


def test_mean_stream(dev):
    cap, B, shape = 3, 2, (5, 6, 7, 3)
    layer, rng, count = check_mean_stream(dev, cap, B, shape, 11)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {'mean': shape, 'count': (1,)}
    assert list(layer.parameters()) == []
    # inference: the stored statistics, nothing updated
    mean, cnt = host(layer.mean).copy(), host(layer.count).copy()
    x = rng.standard_normal((B,) + shape).astype(F32)
    layer.eval()
    xd = gpu(x, dev, grad=True)
    y = layer(xd)
    assert not y.requires_grad                          # no gradient in inference mode
    assert bits_equal(host(layer.mean), mean) and bits_equal(host(layer.count), cnt)
    scale = min(1.0, count / cap)
    within(host(y), np.broadcast_to(scale * mean.astype(np.float64), y.shape), 6 * EPS * scale * np.broadcast_to(np.abs(mean), y.shape),
           'MeanStream y, eval')
    # training=False / 0 in train() mode, and a layer that is not trainable, take the inference branch as well
    layer.train()
    for flag in (False, 0):
        assert bits_equal(host(layer(gpu(x, dev), training=flag)), host(y))
    assert bits_equal(host(layer.mean), mean) and bits_equal(host(layer.count), cnt)
    frozen = ne.layers.MeanStream(cap=cap, trainable=False)
    frozen.train()
    out = frozen(gpu(x, dev))
    assert float(frozen.count) == 0.0 and float(out.abs().max()) == 0.0 and float(frozen.mean.abs().max()) == 0.0
    layer.trainable = False                             # set after construction
    layer(gpu(x, dev), training=True)
    assert bits_equal(host(layer.mean), mean) and bits_equal(host(layer.count), cnt)
    layer.trainable = True
    # eval() mode with training=True updates
    layer.eval()
    layer(gpu(x, dev), training=1)
    assert float(layer.count) == count + B
    # a state_dict round trip into a fresh layer reproduces the next output bit for bit
    layer.train()
    fresh = ne.layers.MeanStream(cap=cap)
    fresh.build((B,) + shape)
    fresh.to(dev)
    fresh.load_state_dict(layer.state_dict())
    fresh.train()
    x2 = gpu(rng.standard_normal((B,) + shape).astype(F32), dev)
    with torch.no_grad():
        assert bits_equal(host(fresh(x2)), host(layer(x2)))
    assert bits_equal(host(fresh.mean), host(layer.mean)) and float(fresh.count) == float(layer.count) == count + 2 * B


def test_mean_stream_cap_below_the_batch_size(dev):
    """cap = 1 with two entries: alpha = 2 (:2067), the formula is followed as written"""
    check_mean_stream(dev, 1, 2, (5, 6, 7, 3), 12)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5: CovStream
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feat', [(5, 7), (6, 11, 2)])
@pytest.mark.parametrize('B', [2, 3])
def test_cov_stream(dev, feat, B):
    cap = 4
    rng = np.random.default_rng(int(np.prod(feat)) + B)
    v = int(np.prod(feat))
    layer = ne.layers.CovStream(cap=cap)
    layer.train()
    count = 0
    for call in range(3):
        x = rng.standard_normal((B,) + feat).astype(F32) + F32(0.25)
        mean0 = np.zeros(feat) if call == 0 else host(layer.mean).astype(np.float64)
        cov0 = np.zeros((v, v)) if call == 0 else host(layer.cov).astype(np.float64)
        new_mean, new_count, _, scale, mean_mag = mean_step64(mean0, float(count), x, cap)
        X = x.astype(np.float64).reshape(B, v)                                        # :2036-2045
        prev_cap = min(float(count), cap)
        denom = prev_cap + B - 1
        new_cov = (cov0 * (prev_cap - 1) + np.einsum('br,bc->rc', X, X)) / denom
        mag = np.abs(cov0 * (prev_cap - 1)) + np.einsum('br,bc->rc', np.abs(X), np.abs(X))
        y = layer(gpu(x, dev))
        count += B
        assert tuple(y.shape) == (B, v, v) and float(layer.count) == float(count)
        tag = 'CovStream %s B=%d call %d' % (feat, B, call)
        within(host(layer.cov), new_cov, (B + 1 + 5) * EPS * mag / denom, tag + ' cov')
        within(host(layer.mean), new_mean, (B + 1 + 5) * EPS * mean_mag, tag + ' mean')
        within(host(y), np.broadcast_to(scale * new_cov, y.shape), (B + 1 + 5) * EPS * scale * np.broadcast_to(mag, y.shape) / denom,
               tag + ' y')
        c = host(layer.cov)
        assert bits_equal(c, np.ascontiguousarray(c.T)), tag + ': cov is not symmetric'
    cov, mean, cnt = host(layer.cov).copy(), host(layer.mean).copy(), host(layer.count).copy()
    layer.eval()
    x = rng.standard_normal((B,) + feat).astype(F32)
    y = layer(gpu(x, dev, grad=True))                   # inference mode: no refusal, no gradient, nothing updated
    assert not y.requires_grad
    scale = min(1.0, count / cap)
    within(host(y), np.broadcast_to(scale * cov.astype(np.float64), y.shape), 6 * EPS * scale * np.broadcast_to(np.abs(cov), y.shape),
           'CovStream %s B=%d eval y' % (feat, B))
    assert bits_equal(host(layer.cov), cov) and bits_equal(host(layer.mean), mean) and bits_equal(host(layer.count), cnt)
    layer.train()
    with pytest.raises(NotImplementedError, match='gradient'):
        layer(gpu(x, dev, grad=True))
    assert bits_equal(host(layer.cov), cov) and bits_equal(host(layer.count), cnt)
    with torch.no_grad():
        layer(gpu(x, dev, grad=True))                   # grad mode off: an update like any other
    assert float(layer.count) == count + B


@pytest.mark.parametrize('feat', [(5, 7), (6, 11, 2)])
def test_cov_stream_first_call_with_one_entry_is_plain_ieee(dev, feat):
    """a fresh layer and B = 1: the denominator min(count, cap) + B - 1 is 0 (:2045) -- Inf where the product is not zero, NaN where
    it is; the float32 restatement of :2031-2052 gives the same bits"""
    cap = F32(4)
    rng = np.random.default_rng(5)
    v = int(np.prod(feat))
    x = rng.standard_normal((1,) + feat).astype(F32)
    x.reshape(-1)[0] = 0.0
    x.reshape(-1)[3] = -0.0
    layer = ne.layers.CovStream(cap=4)
    layer.train()
    y = host(layer(gpu(x, dev)))
    with np.errstate(divide='ignore', invalid='ignore'):
        count, mean, cov = np.zeros(1, F32), np.zeros(feat, F32), np.zeros((v, v), F32)
        this_bs = F32(1)
        new_count = count + this_bs
        alpha = this_bs / np.minimum(new_count, cap)
        new_mean = mean * (F32(1) - alpha) + (x.sum(0) / this_bs) * alpha
        X = x.reshape(1, v)
        delta = np.zeros((v, v), F32)
        for b in range(1):
            delta = delta + X[b][:, None] * X[b][None, :]
        prev_cap = np.minimum(count, cap)
        new_cov = (cov * (prev_cap - F32(1)) + delta) / (prev_cap + this_bs - F32(1))
        want = np.minimum(F32(1), new_count / cap) * (np.ones((1, v, v), F32) * new_cov[None])
    assert want.dtype == F32 and np.isnan(want[0, 0]).all() and np.isinf(want[0, 1, 1])
    assert bits_equal(y, want)
    assert bits_equal(host(layer.cov), new_cov) and bits_equal(host(layer.mean), new_mean) and float(layer.count) == 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
# 6: graph capture
# ----------------------------------------------------------------------------------------------------------------------------------
def test_stream_and_local_layers_under_graph_replay(dev):
    """one capture of MeanStream (training) -> LocalLinear; every replay reads the static input anew and advances the statistics on
    the device (tests/test_gpu_graph_capture.py's pattern: warm up on a side stream, capture, replay on changed inputs)"""
    rng = np.random.default_rng(21)
    B, shape, cap = 2, (5, 6, 7, 3), 5
    inputs = [gpu(rng.standard_normal((B,) + shape).astype(F32), dev) for _ in range(5)]
    static = inputs[0].clone()
    nets = []
    for _ in range(2):                                  # the captured pair and its eager twin
        ms, lin = ne.layers.MeanStream(cap=cap), ne.layers.LocalLinear()
        ms.train()
        nets.append((ms, lin))
    (ms, lin), (ms2, lin2) = nets

    def fn():
        with torch.no_grad():
            return lin(ms(static))

    def twin(x):
        with torch.no_grad():
            return lin2(ms2(x))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(2):                              # builds the layers, lazy allocations: outside the capture
            static.copy_(inputs[k])
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2):
        twin(inputs[k])
    lin2.load_state_dict(lin.state_dict())
    assert float(ms.count) == 2 * B
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    torch.cuda.synchronize()
    assert float(ms.count) == 2 * B                     # a capture records, it does not run
    for k in range(2, 5):
        static.copy_(inputs[k])
        g.replay()
        torch.cuda.synchronize()
        want = twin(inputs[k])
        assert float(ms.count) == (k + 1) * B
        assert torch.equal(ms.mean, ms2.mean) and torch.equal(ms.count, ms2.count), 'replay %d' % k
        assert torch.equal(out, want), 'replay %d' % k
    assert float(ms.count) == 2 * B + 3 * B
