"""
csrc/dense.hip through the C ABI against float64 NumPy.

Pass criteria are bounds that hold for ANY summation order of float32 terms each rounded once (u = 2^-24), so they pin no
implementation detail, while an indexing fault breaks them by orders of magnitude:
    forward  |err| <= (in + 2) u (sum_i |x w| + |bias|)        gx  (out + 2) u sum_o |g w|
    gw       (batch + 2) u sum_b |x g|                         gbias  (batch + 1) u sum_b |g|
An activation is 1-Lipschitz here (elu, relu: the set fused into the conv epilogues) and is evaluated once more in float32: the
pre-activation bound plus 4 u max(1, |y|) (expf within 2 ulp of a value <= 1, one subtraction, one rounding of the result).
Shapes are the smallest that cross a slab boundary with a tail, out % 4 != 0, a single column, a second batch chunk (17, 33 > 16) and a
second-stage sum over many partials; each runs under variant 0, 1 and 2, and each call is repeated and must be bit-identical.
"""

import numpy as np
import pytest
import torch

from neurite_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BASE = [(1, 7, 1), (3, 4099, 5), (2, 4096, 64), (17, 1031, 100), (4, 70001, 12), (33, 64, 64)]
SHAPES = BASE + [(b, o, i) for b, i, o in BASE]
ACTS = {0: lambda v: v, 1: lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, 0))), 2: lambda v: np.maximum(v, 0)}
_DATA = {}


def _data(shape):
    """inputs, float64 references and bounds of a shape, computed once and shared by every test of it (never written to)"""
    if shape not in _DATA:
        B, cin, cout = shape
        rng = np.random.default_rng(B * 1000003 + cin * 101 + cout)
        x = rng.standard_normal((B, cin)).astype(np.float32)
        w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
        bias = rng.standard_normal(cout).astype(np.float32)
        g = rng.standard_normal((B, cout)).astype(np.float32)
        x64, w64, g64 = x.astype(np.float64), w.astype(np.float64), g.astype(np.float64)
        d = dict(x=x, w=w, bias=bias, g=g)
        d['pre'] = x64 @ w64
        d['pre_abs'] = np.abs(x64) @ np.abs(w64)
        d['gx'] = g64 @ w64.T
        d['gx_bound'] = (cout + 2) * U * (np.abs(g64) @ np.abs(w64).T)
        d['gw'] = x64.T @ g64
        d['gw_bound'] = (B + 2) * U * (np.abs(x64).T @ np.abs(g64))
        d['gb'] = g64.sum(0)
        d['gb_bound'] = (B + 1) * U * np.abs(g64).sum(0)
        for a in d.values():
            a.setflags(write=False)
        _DATA[shape] = d
    return _DATA[shape]


def _workspace(dev, B, cin, cout, variant):
    n = _lib.lib().nrt_dense_workspace_bytes(B, cin, cout, variant)
    return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)


def _forward(dev, x, w, bias, y, shape, act, variant):
    B, cin, cout = shape
    ws, n = _workspace(dev, B, cin, cout, variant)
    rc = _lib.lib().nrt_dense_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), B, cin, cout, act, variant, _lib.ptr(ws), n,
                                  _lib.stream_ptr(dev))
    _lib.check(rc, 'nrt_dense_f32')
    torch.cuda.synchronize(dev)


def _check_forward(y, d, with_bias, act, cin, what):
    pre = d['pre'] + (d['bias'].astype(np.float64) if with_bias else 0.0)
    bound = (cin + 2) * U * (d['pre_abs'] + (np.abs(d['bias'].astype(np.float64)) if with_bias else 0.0))
    ref = ACTS[act](pre)
    if act:
        bound = bound + 4 * U * np.maximum(1.0, np.abs(ref))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: max |err| / bound = %.3g' % (what, worst))
    assert np.all(err <= bound), '%s: max |err| / bound = %.3g' % (what, worst)


@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'b%d_in%d_out%d' % s)
def test_forward(dev, shape, variant):
    _lib.init_device(dev)
    B, cin, cout = shape
    d = _data(shape)
    x, w, bias = (torch.tensor(d[k]).to(dev) for k in ('x', 'w', 'bias'))
    for with_bias in (True, False):
        for act in (0, 1, 2):
            y = torch.full((B, cout), float('nan'), dtype=torch.float32, device=dev)
            _forward(dev, x, w, bias if with_bias else None, y, shape, act, variant)
            first = y.cpu().numpy()
            _check_forward(first, d, with_bias, act, cin, 'variant %d bias %d act %d' % (variant, with_bias, act))
            y.fill_(float('nan'))
            _forward(dev, x, w, bias if with_bias else None, y, shape, act, variant)
            assert np.array_equal(first.view(np.uint32), y.cpu().numpy().view(np.uint32)), 'not bit-identical run to run'


def _backward(dev, g, x, w, gx, gw, gb, shape, variant):
    B, cin, cout = shape
    ws, n = _workspace(dev, B, cin, cout, variant)
    rc = _lib.lib().nrt_dense_bwd_f32(_lib.ptr(g), _lib.ptr(x), _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), B, cin, cout,
                                      variant, _lib.ptr(ws), n, _lib.stream_ptr(dev))
    _lib.check(rc, 'nrt_dense_bwd_f32')
    torch.cuda.synchronize(dev)


def _within(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: max |err| / bound = %.3g' % (what, worst))
    assert np.all(err <= bound), '%s: max |err| / bound = %.3g' % (what, worst)


@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'b%d_in%d_out%d' % s)
def test_backward(dev, shape, variant):
    _lib.init_device(dev)
    B, cin, cout = shape
    d = _data(shape)
    x, w, g = (torch.tensor(d[k]).to(dev) for k in ('x', 'w', 'g'))
    outs = []
    for _ in range(2):
        gx = torch.full((B, cin), float('nan'), dtype=torch.float32, device=dev)
        gw = torch.full((cin, cout), float('nan'), dtype=torch.float32, device=dev)
        gb = torch.full((cout,), float('nan'), dtype=torch.float32, device=dev)
        _backward(dev, g, x, w, gx, gw, gb, shape, variant)
        outs.append([t.cpu().numpy() for t in (gx, gw, gb)])
    _within(outs[0][0], d['gx'], d['gx_bound'], 'gx variant %d' % variant)
    _within(outs[0][1], d['gw'], d['gw_bound'], 'gw')
    _within(outs[0][2], d['gb'], d['gb_bound'], 'gbias')
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'not bit-identical run to run'


@pytest.mark.parametrize('shape', [(3, 4099, 5), (2, 64, 4096)], ids=lambda s: 'b%d_in%d_out%d' % s)
@pytest.mark.parametrize('want', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)])
def test_backward_leaves_absent_outputs_alone(dev, shape, want):
    """gx / gw / gbias are optional: a NULL one is not computed, and the buffer that WOULD have held it (sitting between guard words,
    right behind the outputs that are written) keeps every byte"""
    _lib.init_device(dev)
    B, cin, cout = shape
    d = _data(shape)
    x, w, g = (torch.tensor(d[k]).to(dev) for k in ('x', 'w', 'g'))
    sizes = [B * cin, cin * cout, cout]
    guard = 64
    pool = torch.full((sum(sizes) + 4 * guard,), -12345.0, dtype=torch.float32, device=dev)
    offs, o = [], guard
    for n in sizes:
        offs.append(o)
        o += n + guard
    views = [pool[a:a + n] for a, n in zip(offs, sizes)]
    gx, gw, gb = [v if k else None for v, k in zip(views, want)]
    _backward(dev, g, x, w, gx, gw, gb, shape, 0)
    host = pool.cpu().numpy()
    refs = [(d['gx'], d['gx_bound']), (d['gw'], d['gw_bound']), (d['gb'], d['gb_bound'])]
    covered = np.zeros(host.shape, bool)
    for a, n, k, (ref, bound), name in zip(offs, sizes, want, refs, ('gx', 'gw', 'gbias')):
        if k:
            _within(host[a:a + n].reshape(ref.shape), ref, bound, name)
            covered[a:a + n] = True
    assert np.all(host[~covered] == -12345.0), 'bytes outside the requested outputs were written'


@pytest.mark.parametrize('variant', [0, 1, 2])
def test_unaligned_base_pointers(dev, variant):
    """x, w and y one float into a larger buffer: 4-byte aligned, not 16-byte aligned; out % 4 == 0, so only the pointers keep the
    call from the 16-byte forms.  The floats around y stay untouched."""
    _lib.init_device(dev)
    shape = (2, 4096, 64)
    B, cin, cout = shape
    d = _data(shape)

    def off1(a):
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
        v = buf[1:1 + a.size]
        v.copy_(torch.from_numpy(a.reshape(-1)))
        assert v.data_ptr() % 16 == 4
        return buf, v
    _, x = off1(d['x'])
    _, w = off1(d['w'])
    ybuf = torch.full((B * cout + 8,), -7.0, dtype=torch.float32, device=dev)
    y = ybuf[1:1 + B * cout]
    bias = torch.from_numpy(d['bias']).to(dev)
    _forward(dev, x, w, bias, y, shape, 0, variant)
    host = ybuf.cpu().numpy()
    _check_forward(host[1:1 + B * cout].reshape(B, cout), d, True, 0, cin, 'unaligned, variant %d' % variant)
    assert host[0] == -7.0 and np.all(host[1 + B * cout:] == -7.0)
    # backward: g, x, w and every output one float in
    _, g = off1(d['g'])
    outs = [torch.full((n + 8,), -7.0, dtype=torch.float32, device=dev) for n in (B * cin, cin * cout, cout)]
    gx, gw, gb = [o[1:-7] for o in outs]
    _backward(dev, g, x, w, gx, gw, gb, shape, variant)
    for o, (ref, bound), name in zip(outs, [(d['gx'], d['gx_bound']), (d['gw'], d['gw_bound']), (d['gb'], d['gb_bound'])],
                                     ('gx', 'gw', 'gbias')):
        host = o.cpu().numpy()
        _within(host[1:-7].reshape(ref.shape), ref, bound, name + ' unaligned')
        assert host[0] == -7.0 and np.all(host[-7:] == -7.0)


def test_a_short_workspace_is_refused(dev):
    _lib.init_device(dev)
    shape = (2, 4096, 64)
    B, cin, cout = shape
    d = _data(shape)
    x, w = (torch.tensor(d[k]).to(dev) for k in ('x', 'w'))
    y = torch.zeros((B, cout), dtype=torch.float32, device=dev)
    small = torch.empty(64, dtype=torch.uint8, device=dev)
    rc = _lib.lib().nrt_dense_f32(_lib.ptr(x), _lib.ptr(w), None, _lib.ptr(y), B, cin, cout, 0, 1, _lib.ptr(small), 64,
                                  _lib.stream_ptr(dev))
    assert rc == _lib.NRT_ERR_WORKSPACE
    torch.cuda.synchronize(dev)
    assert float(y.abs().max()) == 0.0
