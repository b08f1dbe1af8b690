"""
GPU tests of the global max and its gradient (csrc/globalmax.hip; neurite_amd.models._global_max) against torch on the CPU:
  y      bit-exact against torch.amax over the spatial axis (a max is exact, whatever the order);
  count  equal to the exact tie count sum(x == y);
  gx     bit-exact against the float32 expression (1 / count) * g where x == y, 0 elsewhere (tf.reduce_max's gradient), NaN throughout
         a slice whose max is NaN.
B = 2; (V, C) covers one element, the element arm (C = 1, 3, 100 and a 4-byte-offset base pointer), the quad arm (C = 4, 36, 64), the
folded quad arm (C = 1 or 2 with V * C % 4 == 0), more channel units than a block has lanes' worth of rows, and a V at which a batch
entry spans three first-stage blocks (read from nrt_global_max_workspace_bytes, which reports the launcher's grid rule), so that the
second stage merges.  Every call runs twice and its bits are compared; forward + backward are captured into a graph and replayed.
"""

import numpy as np
import pytest
import torch

from neurite_amd import _lib
from neurite_amd import models as M

pytestmark = pytest.mark.gpu
F = np.float32
B = 2


def _blocks(v, c):
    """first-stage blocks per batch entry: workspace = B * blocks * max(C, 4) * 8 bytes (include/neurite_amd.h)"""
    return _lib.lib().nrt_global_max_workspace_bytes(B, v, c) // (B * max(c, 4) * 8)


def _multi_block_v(c=4):
    v = 1
    while _blocks(v, c) < 3:
        v = v * 2 + 1
    lo = v // 2
    while lo + 1 < v:                              # the smallest such V
        mid = (lo + v) // 2
        if _blocks(mid, c) >= 3:
            v = mid
        else:
            lo = mid
    return v


V_MULTI = None
SHAPES = [(1, 1), (7, 1), (4097, 1), (1000, 3), (513, 4), (300, 36), (129, 64), (65, 100), (35937, 2), ('multi', 4), ('multi', 1),
          (1026, 2), (6, 1028), (5, 301)]   # the folded quad arm with two channels; two channel tiles in the quad and the element arm
PATTERNS = ['random', 'quantised', 'max_first', 'max_last', 'all_negative', 'constant', 'ties_straddle', 'all_neg_inf', 'one_pos_inf',
            'one_nan']


def _resolve(v, c):
    global V_MULTI
    if v == 'multi':
        if V_MULTI is None:
            V_MULTI = _multi_block_v(4)
        v = V_MULTI * 4 // c if c < 4 else V_MULTI
        assert _blocks(v, c) >= 3, (v, c)
    return v


def _make(pattern, v, c, rng):
    x = rng.standard_normal((B, v, c)).astype(F)
    if pattern == 'quantised':
        x = rng.integers(-6, 7, (B, v, c)).astype(F)
    elif pattern == 'max_first':
        x[:, 0, :] = 9.0
    elif pattern == 'max_last':
        x[:, -1, :] = 9.0
    elif pattern == 'all_negative':
        x = -np.abs(x) - 1.0
    elif pattern == 'constant':
        x[:] = 0.5
    elif pattern == 'ties_straddle':
        # equal maxima on both sides of every first-stage block boundary (a block owns ceil(V / blocks) rows), and at both ends
        nb = _blocks(v, c)
        per = -(-v // nb)
        for r in {0, v - 1} | {min(v - 1, max(0, k * per + d)) for k in range(1, nb) for d in (-1, 0)}:
            x[:, r, :] = 7.0
    elif pattern == 'all_neg_inf':
        x[:] = -np.inf
    elif pattern == 'one_pos_inf':
        x[0, v // 2, 0] = np.inf
        x[1, v - 1, c - 1] = np.inf
    elif pattern == 'one_nan':
        x[0, v // 3, 0] = np.nan
        x[1, 0, c - 1] = np.nan
    return x


def _reference(x, g):
    xt = torch.from_numpy(x)
    y = torch.amax(xt, dim=1).numpy()
    count = (x == y[:, None, :]).sum(1).astype(np.int32)
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = (F(1.0) / count.astype(F)) * g                      # float32: the reciprocal rounded first
    gx = np.where(x == y[:, None, :], coef[:, None, :], F(0.0)).astype(F)
    gx = np.where(np.isnan(y)[:, None, :], F(np.nan), gx)
    return y, count, gx


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = a.view(np.uint32).copy()
    return a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ': NaN pattern'
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def _run(xg, gg):
    xin = xg.detach().requires_grad_(True)
    y, count = M._global_max(xin, per_channel=True, return_count=True)
    gx, = torch.autograd.grad(y, xin, gg)
    return y.detach(), count, gx


def _check(x, g, dev, xg=None):
    xg = torch.from_numpy(x).to(dev) if xg is None else xg
    gg = torch.from_numpy(g).to(dev)
    y, count, gx = _run(xg, gg)
    y2, count2, gx2 = _run(xg, gg)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(_bits(gx), _bits(gx2))
    assert torch.equal(count, count2)
    wy, wc, wgx = _reference(x, g)
    _same(y.cpu().numpy(), wy, 'y')
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), wc), 'count'
    _same(gx.cpu().numpy(), wgx, 'gx')
    return y, count, gx


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('v,c', SHAPES)
def test_global_max_and_gradient_bit_exact(dev, v, c, pattern):
    v = _resolve(v, c)
    rng = np.random.default_rng(1000 * c + v % 997 + len(pattern))
    x = _make(pattern, v, c, rng)
    g = rng.standard_normal((B, c)).astype(F)
    y, count, _ = _check(x, g, dev)
    if pattern == 'constant':
        assert int(count.min()) == int(count.max()) == v
    if pattern == 'all_neg_inf':
        assert bool(torch.isinf(y).all()) and int(count.min()) == v
    if pattern == 'one_nan':
        assert bool(torch.isnan(y[0, 0])) and int(count[0, 0]) == 0 and int(count[1, c - 1]) == 0


@pytest.mark.parametrize('pattern', ['random', 'ties_straddle', 'one_nan'])
@pytest.mark.parametrize('v', [513, 'multi'])
def test_base_pointer_offset_by_four_bytes_takes_the_element_arm(dev, v, pattern):
    c = 4
    v = _resolve(v, c)
    rng = np.random.default_rng(v)
    x = _make(pattern, v, c, rng)
    g = rng.standard_normal((B, c)).astype(F)
    buf = torch.zeros(B * v * c + 1, dtype=torch.float32, device=dev)
    xg = buf[1:].view(B, v, c)
    xg.copy_(torch.from_numpy(x))
    assert xg.data_ptr() % 16 == 4 and xg.is_contiguous()
    y_off, c_off, gx_off = _check(x, g, dev, xg=xg)
    y, cnt, gx = _check(x, g, dev)                               # the aligned tensor: the quad arm, the same bits
    assert np.array_equal(_bits(y), _bits(y_off)) and torch.equal(cnt, c_off) and np.array_equal(_bits(gx), _bits(gx_off))


def test_flatten_then_max_is_the_single_channel_form(dev):
    """design_dnn's lambda: K.max(K.batch_flatten(x), 1, keepdims=True) on a [B, X, Y, Z, C] tensor"""
    rng = np.random.default_rng(3)
    x = rng.integers(-9, 10, (B, 5, 6, 7, 3)).astype(F)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    y = M._global_max(xg, per_channel=False)
    assert tuple(y.shape) == (B, 1)
    g = rng.standard_normal((B, 1)).astype(F)
    gx, = torch.autograd.grad(y, xg, torch.from_numpy(g).to(dev))
    wy, wc, wgx = _reference(x.reshape(B, -1, 1), g)
    _same(y.detach().cpu().numpy(), wy, 'y')
    _same(gx.cpu().numpy().reshape(B, -1, 1), wgx, 'gx')
    assert int(wc.max()) > 1                                     # the quantised values tie


def test_forward_and_backward_replay_from_a_graph(dev):
    c = 4
    v = _resolve('multi', c)
    rng = np.random.default_rng(11)
    first, second = (torch.from_numpy(_make(p, v, c, rng)).to(dev) for p in ('quantised', 'ties_straddle'))
    gg = torch.from_numpy(rng.standard_normal((B, c)).astype(F)).to(dev)
    x = first.clone()

    def step():
        return _run(x, gg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # workspace growth: outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, c_g, gx_g = step()
    for values in (second, first):
        x.copy_(values)
        graph.replay()
        torch.cuda.synchronize()
        got = (_bits(y_g), c_g.cpu().numpy().copy(), _bits(gx_g))
        y_e, c_e, gx_e = step()
        torch.cuda.synchronize()
        assert np.array_equal(got[0], _bits(y_e)) and np.array_equal(got[1], c_e.cpu().numpy()) and np.array_equal(got[2], _bits(gx_e))
        wy, wc, wgx = _reference(values.cpu().numpy(), gg.cpu().numpy())
        _same(y_e.cpu().numpy(), wy, 'y')
        assert np.array_equal(c_e.cpu().numpy(), wc)
        _same(gx_e.cpu().numpy(), wgx, 'gx')
