"""
utils.separable_conv, layers.GaussianBlur, utils.minmax_norm, utils.subsample_axis and layers.Subsample inside autograd graphs, on
the GPU, against torch float64 autograd on the CPU of the same math written with F.conv1d on explicitly TF-SAME-padded rows, amin /
amax / where, and index_select.

Tolerances, as fractions of the largest oracle gradient of the tensor compared:
  1e-5   one op of this family between the leaf and the loss: the tolerance of the forward row of the README table.
  3e-5   three float32 ops chained (conv -> minmax_norm -> loss, or scale -> blur -> loss): each op's gradient is held to 1e-5 of its
         scale and its float32 inputs carry the error of the op before it, so the errors add.
The gather gradient is a sum of at most a handful of float32 terms: 1e-6.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import augment
from neurite_amd import utils as U

pytestmark = pytest.mark.gpu
F = np.float32


def conv_axis64(x, k, ax, stride=1, dil=1):
    """one TF-SAME pass along axis `ax` of a float64 CPU tensor by F.conv1d on a padded row"""
    n, W = x.shape[ax], k.numel()
    ke = (W - 1) * dil + 1
    o = -(-n // stride)
    total = max((o - 1) * stride + ke - n, 0)
    rows = x.movedim(ax, -1)
    lead = rows.shape[:-1]
    rows = TF.pad(rows.reshape(-1, 1, n), (total // 2, total - total // 2))
    y = TF.conv1d(rows, k.reshape(1, 1, W), stride=stride, dilation=dil)
    return y.reshape(*lead, -1).movedim(-1, ax)


def blur64(x, taps, strides=(1, 1, 1)):
    for ax, (k, s) in enumerate(zip(taps, strides)):
        x = conv_axis64(x, k, ax + 1, s)
    return x


def minmax64(x, axes):
    mn, mx = x.amin(axes, keepdim=True), x.amax(axes, keepdim=True)
    den = mx - mn
    return torch.where(den != 0, (x - mn) / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(x))


def leaf64(a):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=True)


def close(got, want, tol, what):
    got, want = got.detach().cpu().numpy().astype(np.float64), want.detach().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print('%s: error %.3g of the gradient scale' % (what, err / scale))
    assert err <= tol * scale, (what, err, scale)


def test_separable_conv_gradients_wrt_input_and_taps(dev):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 6, 7, 9, 3)).astype(F)
    taps = [rng.standard_normal(w).astype(F) for w in (3, 4, 5)]
    wgt = rng.standard_normal((2, 6, 4, 9, 3)).astype(F)
    strides = (1, 2, 1)
    xd = torch.tensor(x, device=dev, requires_grad=True)
    kd = [torch.tensor(k, device=dev, requires_grad=True) for k in taps]
    y = U.separable_conv(xd, kd, batched=True, strides=strides)
    assert y.grad_fn is not None and tuple(y.shape) == wgt.shape
    (y * torch.tensor(wgt, device=dev)).sum().backward()
    xo, ko = leaf64(x), [leaf64(k) for k in taps]
    yo = blur64(xo, ko, strides)
    (yo * torch.tensor(wgt.astype(np.float64))).sum().backward()
    close(y, yo, 1e-5, 'forward')
    close(xd.grad, xo.grad, 1e-5, 'dx')
    for i in range(3):
        assert kd[i].grad is not None, 'the graph of tap tensor %d was cut' % i
        close(kd[i].grad, ko[i].grad, 1e-5, 'dk[%d]' % i)


def test_device_taps_are_used_in_place_and_x_is_saved_only_for_tap_gradients(dev):
    x = torch.randn(1, 5, 6, 2, device=dev, requires_grad=True)
    k = torch.randn(3, device=dev)
    y = U.separable_conv(x, k, batched=True, axis=0)
    saved = y.grad_fn.saved_tensors
    assert saved[0] is None and saved[1].data_ptr() == k.data_ptr()            # the taps where they lie; x not kept
    k.requires_grad_(True)
    y = U.separable_conv(x.detach(), k, batched=True, axis=0)
    saved = y.grad_fn.saved_tensors
    assert saved[0] is not None and saved[1] is None


@pytest.mark.parametrize('mode', ['sigma1.5', 'random-isotropic'])
def test_gaussian_blur_inside_a_graph(dev, mode):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 9, 8, 10, 2)).astype(F)
    scale = rng.standard_normal((2,)).astype(F)
    if mode == 'sigma1.5':
        layer = ne.layers.GaussianBlur(sigma=1.5)
        taps = U.gaussian_kernel(sigma=[1.5] * 3, separate=True)
    else:
        layer = ne.layers.GaussianBlur(sigma=2.0, random=True, min_sigma=0.5, isotropic=True, seed=4)
        taps = [U.gaussian_kernel(sigma=[2.0], random=True, min_sigma=[0.5], separate=True, seed=4)] * 3
    xd = torch.tensor(x, device=dev, requires_grad=True)
    sd = torch.tensor(scale, device=dev, requires_grad=True)
    y = layer(xd * sd)
    assert y.grad_fn is not None
    (y ** 2).mean().backward()
    xo, so = leaf64(x), leaf64(scale)
    yo = blur64(xo * so, [t.to(torch.float64) for t in taps])
    (yo ** 2).mean().backward()
    close(y, yo, 1e-5, 'forward')
    close(xd.grad, xo.grad, 3e-5, 'dx')
    close(sd.grad, so.grad, 3e-5, 'dscale')


def test_minmax_norm_of_a_conv_output(dev):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 7, 6, 9, 3)).astype(F)
    taps = [rng.standard_normal(w).astype(F) for w in (3, 3, 2)]
    wgt = rng.standard_normal(x.shape).astype(F)
    xd = torch.tensor(x, device=dev, requires_grad=True)
    kd = [torch.tensor(k, device=dev, requires_grad=True) for k in taps]
    y = U.minmax_norm(U.separable_conv(xd, kd, batched=True), axis=[1, 2, 3])
    assert y.grad_fn is not None
    (y * torch.tensor(wgt, device=dev)).sum().backward()
    xo, ko = leaf64(x), [leaf64(k) for k in taps]
    yo = minmax64(blur64(xo, ko), (1, 2, 3))
    (yo * torch.tensor(wgt.astype(np.float64))).sum().backward()
    close(y, yo, 1e-5, 'forward')
    close(xd.grad, xo.grad, 3e-5, 'dx')
    for i in range(3):
        close(kd[i].grad, ko[i].grad, 3e-5, 'dk[%d]' % i)


@pytest.mark.parametrize('upsample', [True, False])
def test_subsample_axis_with_recorded_draws(dev, upsample):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 12, 10, 3)).astype(F)
    draws = [0.4, 0.55]                                         # the axis draw, the thickness draw
    ax_i, thick = U._subsample_draws(2, 2, 4, 1, None, draws)
    ax = (1, 2)[ax_i]
    down, up = U.subsample_axis_indices(x.shape[ax], thick)
    index = down[up] if upsample else down
    assert upsample or index.size < x.shape[ax]
    wgt = rng.standard_normal(x.shape[:ax] + (index.size,) + x.shape[ax + 1:]).astype(F)
    xd = torch.tensor(x, device=dev, requires_grad=True)
    y = U.subsample_axis(xd, stride_min=2, stride_max=4, axes=(1, 2), upsample=upsample, _draws=draws)
    assert y.grad_fn is not None
    (y * torch.tensor(wgt, device=dev)).sum().backward()
    xo = leaf64(x)
    yo = xo.index_select(ax, torch.tensor(index, dtype=torch.long))
    (yo * torch.tensor(wgt.astype(np.float64))).sum().backward()
    assert (y.detach().cpu().numpy() == yo.detach().numpy().astype(F)).all()
    close(xd.grad, xo.grad, 1e-6, 'dx')


def test_subsample_layer(dev):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 12, 10, 3)).astype(F)
    layer = ne.layers.Subsample(stride_min=2, stride_max=4, seed=3)
    xd = torch.tensor(x, device=dev, requires_grad=True)
    y = layer(xd)
    assert y.grad_fn is not None
    seed = int(np.random.default_rng(3).integers(2 ** 31 - 1))                 # the layer's first draw of a seed
    ax_i, thick = U._subsample_draws(len(layer.axes), 2, 4, 1, seed)
    ax = list(layer.axes)[ax_i]
    down, up = U.subsample_axis_indices(x.shape[ax], thick)
    wgt = rng.standard_normal(x.shape).astype(F)
    (y * torch.tensor(wgt, device=dev)).sum().backward()
    xo = leaf64(x)
    (xo.index_select(ax, torch.tensor(down[up], dtype=torch.long)) * torch.tensor(wgt.astype(np.float64))).sum().backward()
    close(xd.grad, xo.grad, 1e-6, 'dx')


def test_untracked_path_is_the_forward_only_op(dev):
    """requires_grad False, or no_grad: the same launches as before the family was differentiable -- the outputs equal those of the
    C ABI called directly, bit for bit, and carry no grad_fn; the tracked path returns the same bits"""
    rng = np.random.default_rng(5)
    x = torch.tensor(rng.standard_normal((2, 9, 8, 10, 3)).astype(F), device=dev)
    taps = [torch.tensor(rng.standard_normal(w).astype(F), device=dev) for w in (3, 4, 5)]

    def direct(x):
        for ax, k in enumerate(taps):
            n, W = x.shape[ax + 1], k.numel()
            o = -(-n // 1)
            before = max((o - 1) + W - n, 0) // 2
            y = torch.empty_like(x)
            _lib.call(dev, 'nrt_conv1d_axis_f32', _lib.ptr(x), _lib.ptr(k), _lib.ptr(y), int(np.prod(x.shape[:ax + 1])), n,
                      int(np.prod(x.shape[ax + 2:])), o, W, 1, 1, before)
            x = y
        z = torch.empty_like(x)
        nws = _lib.lib().nrt_minmax_workspace_bytes(2, 3)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        _lib.call(dev, 'nrt_minmax_norm_f32', _lib.ptr(x), _lib.ptr(z), 2, 9 * 8 * 10, 3, _lib.ptr(ws), nws)
        return x, z

    want_blur, want_norm = direct(x)
    outs = []
    a = U.separable_conv(x, taps, batched=True)
    outs.append((a, U.minmax_norm(a, axis=[1, 2, 3])))
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        a = U.separable_conv(xg, taps, batched=True)
        outs.append((a, U.minmax_norm(a, axis=[1, 2, 3])))
        s = U.subsample_axis(xg, _draws=[0.3, 0.5])
    assert s.grad_fn is None and not s.requires_grad
    for a, b in outs:
        assert a.grad_fn is None and b.grad_fn is None and not a.requires_grad and not b.requires_grad
        assert torch.equal(a.view(torch.int32), want_blur.view(torch.int32))
        assert torch.equal(b.view(torch.int32), want_norm.view(torch.int32))
    a = U.separable_conv(xg, taps, batched=True)
    b = U.minmax_norm(a, axis=[1, 2, 3])
    assert a.grad_fn is not None and b.grad_fn is not None
    assert torch.equal(a.detach().view(torch.int32), want_blur.view(torch.int32))
    assert torch.equal(b.detach().view(torch.int32), want_norm.view(torch.int32))


def test_forward_only_ops_raise_on_backward(dev):
    x = torch.randn(8, 9, 10, 1, device=dev, requires_grad=True)
    y, _ = augment.random_blur_rescale(x, std_min=0.5, std_max=1.5, seed=1, reduce='max')      # 'max': a deterministic statistic
    assert y.requires_grad and y.grad_fn is not None            # tracked as a whole, not half of it
    with pytest.raises(NotImplementedError, match='backward'):
        y.sum().backward()
    with torch.no_grad():
        z, _ = augment.random_blur_rescale(x, std_min=0.5, std_max=1.5, seed=1, reduce='max')
    assert z.grad_fn is None and torch.equal(z, y.detach())


def test_forward_and_backward_capture_into_one_graph(dev):
    """blur -> minmax_norm -> weighted sum and its gradient in one torch.cuda.graph: no host synchronisation, no pageable copy.  The
    input changes between replays; every replay's gradient equals the eager one bit for bit, and replaying twice changes nothing."""
    rng = np.random.default_rng(6)
    shape = (2, 12, 11, 10, 2)
    data = [torch.tensor(rng.standard_normal(shape).astype(F), device=dev) for _ in range(2)]
    wgt = torch.tensor(rng.standard_normal(shape).astype(F), device=dev)
    layer = ne.layers.GaussianBlur(sigma=1.0)
    x = data[0].clone().requires_grad_(True)

    def step():
        y = U.minmax_norm(layer(x), axis=[1, 2, 3])
        return torch.autograd.grad((y * wgt).sum(), x)[0]

    eager = []
    for d in data:
        with torch.no_grad():
            x.copy_(d)
        eager.append(step().clone())
    assert not torch.equal(eager[0], eager[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx = step()
    for d, want in list(zip(data, eager)) + [(data[0], eager[0])]:
        with torch.no_grad():
            x.copy_(d)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gx.view(torch.int32), want.view(torch.int32))
