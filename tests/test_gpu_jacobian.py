"""
utils.jacobian_determinant / metrics.JacobianDeterminant / losses.NegJacobian (csrc/jacobian.hip) on the GPU against the float64
restatement of tests/jacobian_restatement.py (np.gradient's stencil, the VoxelMorph expansion).  Every forward call is made twice and
the two results are compared bit for bit.

The kernels are gathers with one thread per voxel: a block of 256 threads owns a run of at least 2048 voxels of one batch entry, a
batch entry has at most 2048 runs (above 2048 * 2048 voxels the runs grow), and a second launch adds the runs' partials.  Shapes
[*S]; every case runs with batch 3, some with batch 1 as well:
    2x2x2, 3x2x5, 2x3         every voxel at a border; extent 2 (both voxels use the same difference), extent 3 (one interior voxel)
    5x6x7                     210 voxels: one run, not every thread has a voxel
    9x33x34                   10098 voxels: 5 runs of 2020, seams in the middle of lines and planes
    2|3|4|6 x9x10             outer extents 2, 3, 4 and 6
    23x89, 32x64, 3x683       2047, 2048, 2049 voxels: one run short of, at, and one voxel past the run length (2-D)
    17x241, 17x65             4097 voxels: three runs; 1105: one
    2049x2050                 4200450 voxels > 2048 * 2048: 2048 runs of 2051 voxels (batch 1, integer field only)
Fields: even integers in -6 .. 6 (every determinant, cofactor and short sum exact in float32: bit-for-bit cases) and
amp * standard normal at amplitudes 0.3 and 1.5, seed 3: at that seed no voxel of any case has |det64| within the float32 bound of
zero, which the count and loss-gradient tests assert before they compare (the cap on excluded voxels is zero).

Measured on MI355X (every test prints its ratio): the map of float fields at most 0.38 of the derived bound; the two sums at most
1.6e-10 of the order-free bound (threads add in float64); gradients, through the map and through the loss, at most 1.7e-7 of the largest
magnitude (criterion 2e-4).
"""

import numpy as np
import pytest
import torch

import jacobian_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 3
SHAPES = [(2, 2, 2), (3, 2, 5), (5, 6, 7), (9, 33, 34), (2, 9, 10), (3, 9, 10), (4, 9, 10), (6, 9, 10), (2, 3), (17, 65), (23, 89), (32, 64),
          (3, 683), (17, 241)]
CASES = [(s, 3) for s in SHAPES] + [(s, 1) for s in [(2, 2, 2), (5, 6, 7), (9, 33, 34), (17, 65)]]
IDS = ['%s_b%d' % ('x'.join(map(str, s)), b) for s, b in CASES]
_CACHE = {}


def _ne():
    import neurite_amd as ne
    return ne


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy()


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), 'not bit-identical run to run'
    return a


def _field(shape, batch, kind):
    """float32 CPU tensor [batch, *shape, D], made once; kind 'int' or the amplitude of a normal field"""
    key = (shape, batch, kind)
    if key not in _CACHE:
        rng = np.random.default_rng(SEED)
        full = (batch,) + tuple(shape) + (len(shape),)
        f = R.even_integer_field(full, rng) if kind == 'int' else (kind * rng.standard_normal(full)).astype(np.float32)
        _CACHE[key] = torch.tensor(f)
    return _CACHE[key]


def _ref(shape, batch, kind):
    """(det64 [B, *S], bound [B, *S]) of a field, made once: the float64 restatement and 12 * 2^-24 * scale"""
    key = (shape, batch, kind, 'ref')
    if key not in _CACHE:
        f = _field(shape, batch, kind).double()
        _CACHE[key] = (R.det_torch(f), 12 * U * R.error_scale(f))
    return _CACHE[key]


def _assert_no_voxel_near_zero(shape, batch, kind):
    det64, bound = _ref(shape, batch, kind)
    near = int((det64.abs() <= bound).sum())
    assert near == 0, '%d voxels have |det64| within the float32 bound of zero: choose another seed' % near


def _rows(dev, f):
    """the raw stats rows of the kernel: count [B] int64 and [B, 4] float64 (min, max, sum det, sum det^2)"""
    ne = _ne()
    disp, _ = ne.utils._jacdet_checked(f.to(dev), 'test')
    _, rows, _ = _twice(lambda: ne.utils._jacdet_launch(disp, want_stats=True))
    rows = rows.cpu()
    return rows[:, 0].contiguous().view(torch.int64).numpy(), rows[:, 1:].numpy()


# ---- 1. even-integer fields: bit for bit ----------------------------------------------------------------------------------------------
def _check_integer_field(dev, shape, batch):
    ne = _ne()
    f = _field(shape, batch, 'int')
    det64, _ = _ref(shape, batch, 'int')
    want = det64.numpy()
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = _twice(lambda: ne.utils.jacobian_determinant(f.to(dev)))
    assert got.shape == tuple(f.shape[:-1]) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want), 'stencil, border or run-seam error: %d voxels differ' % int(
        (got.cpu().numpy() != want).sum())
    flat = want.reshape(batch, -1)
    V = flat.shape[1]
    count, rows = _rows(dev, f)
    assert np.array_equal(count, (flat <= 0).sum(1))
    assert np.array_equal(rows[:, 0], flat.min(1)) and np.array_equal(rows[:, 1], flat.max(1))
    assert np.array_equal(rows[:, 2], flat.sum(1)) and np.array_equal(rows[:, 3], (flat * flat).sum(1))     # multiples of 1/8, 1/64: exact
    st = _twice(lambda: tuple(ne.metrics.JacobianDeterminant().stats(f.to(dev))))
    assert np.array_equal(st[0].cpu().numpy(), count) and st[0].dtype == torch.int64
    assert np.array_equal(st[1].cpu().numpy(), count / float(V))
    assert np.array_equal(st[4].cpu().numpy(), flat.sum(1) / float(V))
    assert np.allclose(st[5].cpu().numpy(), flat.std(1), rtol=1e-12, atol=0)
    # the loss, as float32(sum64 / V), and its gradient: float64 rounded once
    y = f.to(dev).requires_grad_(True)
    loss = _twice(lambda: ne.losses.NegJacobian().loss(None, y))
    want_loss = (np.maximum(0.0, -flat).sum(1) / float(V)).astype(np.float32)
    assert loss.shape == (batch,) and np.array_equal(_bits(loss), want_loss.view(np.int32))
    w = torch.tensor(np.random.default_rng(4).random(batch).astype(np.float32) + 0.5)
    gy, = torch.autograd.grad((loss * w.to(dev)).sum(), (y,))
    # (the gradient of the SUM of max(0, -det) is a short sum of cofactors, multiples of 1/2: exact in any order; then float64 scales it
    # by w / V, two float64 roundings whatever the machine, and float32 rounds once)
    y64 = f.double().requires_grad_(True)
    gsum, = torch.autograd.grad(torch.relu(-R.det_torch(y64)).sum(), (y64,))
    assert np.array_equal(gsum.numpy() * 2, np.round(gsum.numpy() * 2))
    wy = gsum * (w.double() / float(V)).reshape((batch,) + (1,) * (f.dim() - 1))
    assert float(wy.abs().max()) > 0
    want_gy = wy.to(torch.float32).numpy()                               # (compared as values: a zero may carry either sign)
    assert np.array_equal(gy.cpu().numpy(), want_gy), '%d elements differ' % int((gy.cpu().numpy() != want_gy).sum())


@pytest.mark.parametrize('shape,batch', CASES, ids=IDS)
def test_even_integer_fields_are_exact(dev, shape, batch):
    _check_integer_field(dev, shape, batch)


def test_more_than_2048_runs_worth_of_voxels(dev):
    """above 2048 * 2048 voxels the runs grow past 2048 voxels instead of becoming more"""
    _check_integer_field(dev, (2049, 2050), 1)


# ---- 2. float fields: the map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp', [0.3, 1.5])
@pytest.mark.parametrize('shape,batch', CASES, ids=IDS)
def test_map_of_float_fields_within_the_derived_bound(dev, shape, batch, amp):
    ne = _ne()
    f = _field(shape, batch, amp)
    det64, bound = _ref(shape, batch, amp)
    if det64.numel() >= 200:
        assert bool((det64 < 0).any()) and bool((det64 > 0).any()), 'the field must fold somewhere and not everywhere'
    got = _twice(lambda: ne.utils.jacobian_determinant(f.to(dev)))
    err = (got.cpu().double() - det64).abs()
    ratio = float((err / bound).max())
    print('%s b%d amp %g: det, worst |err| / bound = %.3g' % (shape, batch, amp, ratio))
    assert bool((err <= bound).all()), ratio
    # an unbatched field gives the first entry's bits; the metric class gives the map's
    one = ne.utils.jacobian_determinant(f[0].to(dev))
    assert one.shape == tuple(shape) and np.array_equal(_bits(one), _bits(got[0]))
    assert np.array_equal(_bits(ne.metrics.JacobianDeterminant().det(f.to(dev))), _bits(got))


# ---- 3. float fields: the stats -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp', [0.3, 1.5])
@pytest.mark.parametrize('shape,batch', CASES, ids=IDS)
def test_stats_of_float_fields(dev, shape, batch, amp):
    ne = _ne()
    f = _field(shape, batch, amp)
    own = ne.utils.jacobian_determinant(f.to(dev)).cpu().numpy().reshape(batch, -1)          # the kernel's own map
    V = own.shape[1]
    count, rows = _rows(dev, f)
    assert np.array_equal(count, (own <= 0).sum(1))
    assert np.array_equal(rows[:, 0], own.min(1).astype(np.float64)) and np.array_equal(rows[:, 1], own.max(1).astype(np.float64))
    own64 = own.astype(np.float64)
    for k, terms in ((2, own64), (3, own64 * own64)):
        err = np.abs(rows[:, k] - terms.sum(1))
        bound = V * U * np.abs(terms).sum(1)                                                 # the order-free bound
        print('%s b%d amp %g: sum %d, worst |err| / bound = %.3g' % (shape, batch, amp, k, float((err / bound).max())))
        assert np.all(err <= bound)
    st = ne.metrics.JacobianDeterminant().stats(f.to(dev))
    assert all(t.shape == (batch,) for t in st) and st.folded_voxels.dtype == torch.int64
    mean = rows[:, 2] / V
    assert np.array_equal(st.folded_voxels.cpu().numpy(), count) and np.array_equal(st.folded_fraction.cpu().numpy(), count / float(V))
    assert np.array_equal(st.min.cpu().numpy(), rows[:, 0]) and np.array_equal(st.max.cpu().numpy(), rows[:, 1])
    assert np.array_equal(st.mean.cpu().numpy(), mean)
    assert np.allclose(st.std.cpu().numpy(), np.sqrt(np.maximum(rows[:, 3] / V - mean * mean, 0.0)), rtol=1e-12, atol=0)
    assert np.abs(st.mean.cpu().numpy() - own64.mean(1)).max() <= U * np.abs(own64).sum(1).max()
    assert np.array_equal(_bits(ne.metrics.JacobianDeterminant().folded(f.to(dev))), _bits(st.folded_fraction))
    # the float64 count, where no voxel is within the bound of zero: every case at this seed
    _assert_no_voxel_near_zero(shape, batch, amp)
    det64, _ = _ref(shape, batch, amp)
    assert np.array_equal(count, (det64 <= 0).reshape(batch, -1).sum(1).numpy())


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.detach().cpu().double() - want).abs().max())
    print('%s: largest |err| / largest magnitude = %.3g' % (what, err / scale if scale > 0 else float('nan')))
    assert scale > 0 and err <= 2e-4 * scale, (what, err, scale)


@pytest.mark.parametrize('shape,batch', CASES, ids=IDS)
def test_gradients_against_float64_autograd(dev, shape, batch):
    ne = _ne()
    amp = 1.5
    f = _field(shape, batch, amp)
    y64 = f.double().requires_grad_(True)
    y = f.to(dev).requires_grad_(True)
    g = torch.Generator().manual_seed(4)
    up = torch.randn(f.shape[:-1], generator=g, dtype=torch.float64)
    w = torch.rand(batch, generator=g, dtype=torch.float64) + 0.5
    what = '%s b%d' % (shape, batch)
    # through the map, under a random upstream gradient
    wy, = torch.autograd.grad((R.det_torch(y64) * up).sum(), (y64,))
    gy, = torch.autograd.grad((ne.utils.jacobian_determinant(y) * up.float().to(dev)).sum(), (y,))
    _close(gy, wy, what + ' map gdisp')
    gy2, = torch.autograd.grad((ne.utils.jacobian_determinant(y) * up.float().to(dev)).sum(), (y,))
    assert np.array_equal(_bits(gy), _bits(gy2)), 'not bit-identical run to run'
    # through the loss: the indicator must not flip, so no voxel may be within the bound of zero
    _assert_no_voxel_near_zero(shape, batch, amp)
    for mult in (None, 2.5):
        want = R.neg_loss(y64) * (1.0 if mult is None else mult)
        got = _twice(lambda: ne.losses.NegJacobian(mult).loss(None, y))
        det64, bound = _ref(shape, batch, amp)
        assert float((got.detach().cpu().double() - want.detach()).abs().max()) <= 1.01 * float(bound.reshape(batch, -1).mean(1).max()) * (
            1.0 if mult is None else mult) + 2 * U * float(want.detach().abs().max())
        wy, = torch.autograd.grad((want * w).sum(), (y64,))
        gy, = torch.autograd.grad((got * w.float().to(dev)).sum(), (y,))
        _close(gy, wy, what + ' loss gdisp, mult %s' % mult)


def test_both_upstream_gradients_in_one_call(dev):
    """gdet and gloss together: the sum of what each gives alone"""
    ne = _ne()
    L = ne._lib
    shape, batch = (9, 33, 34), 3
    disp = _field(shape, batch, 1.5).to(dev).contiguous()
    g = torch.Generator().manual_seed(5)
    gdet = torch.randn(disp.shape[:-1], generator=g).to(dev)
    gloss = (torch.rand(batch, generator=g) + 0.5).to(dev)
    outs = []
    for a, b in ((gdet, None), (None, gloss), (gdet, gloss)):
        o = torch.full_like(disp, float('nan'))
        L.call(dev, 'nrt_jacdet_bwd_f32', L.ptr(disp), L.ptr(a), L.ptr(b), batch, L.ints(shape), 3, L.ptr(o))
        outs.append(o)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[2]).all()) and float(outs[1].abs().max()) > 0
    assert np.array_equal(_bits(outs[2]), _bits(outs[0] + outs[1]))


def test_from_an_unaligned_base_pointer(dev):
    """a voxel is 12 bytes (8 in 2-D): nothing may assume more than 4-byte alignment of the field, the map or the gradient"""
    ne = _ne()
    for shape in ((9, 33, 34), (17, 65)):
        y = _field(shape, 3, 1.5).to(dev)
        buf = torch.zeros(y.numel() + 1, device=dev)
        off = buf[1:].view(y.shape)
        off.copy_(y)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert np.array_equal(_bits(ne.utils.jacobian_determinant(y)), _bits(ne.utils.jacobian_determinant(off)))
        a, b = ne.metrics.JacobianDeterminant().stats(y), ne.metrics.JacobianDeterminant().stats(off)
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        yl, ol = y.clone().requires_grad_(True), off.detach().requires_grad_(True)
        la, lb = ne.losses.NegJacobian().loss(None, yl), ne.losses.NegJacobian().loss(None, ol)
        assert np.array_equal(_bits(la), _bits(lb))
        ga, = torch.autograd.grad(la.sum(), (yl,))
        gb, = torch.autograd.grad(lb.sum(), (ol,))
        assert np.array_equal(_bits(ga), _bits(gb))
        up = torch.randn(y.shape[:-1], generator=torch.Generator().manual_seed(6)).to(dev)
        ga, = torch.autograd.grad((ne.utils.jacobian_determinant(yl) * up).sum(), (yl,))
        gb, = torch.autograd.grad((ne.utils.jacobian_determinant(ol) * up).sum(), (ol,))
        assert np.array_equal(_bits(ga), _bits(gb))


def test_a_non_contiguous_field_is_made_contiguous(dev):
    ne = _ne()
    y = _field((5, 6, 7), 3, 1.5).to(dev)
    strided = y.permute(0, 3, 2, 1, 4).contiguous().permute(0, 3, 2, 1, 4)
    assert not strided.is_contiguous() and torch.equal(strided, y)
    assert np.array_equal(_bits(ne.utils.jacobian_determinant(strided)), _bits(ne.utils.jacobian_determinant(y)))
    assert np.array_equal(_bits(ne.losses.NegJacobian().loss(None, strided)), _bits(ne.losses.NegJacobian().loss(None, y)))


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_multiple_losses_decorator_backward_to_the_flow_of_a_warp(dev):
    """NCC + Grad + NegJacobian of one y_pred (three channels, so that it can stand for a field), back through the warp that made it"""
    ne = _ne()
    rng = np.random.default_rng(13)
    moving = torch.tensor((2.0 * rng.standard_normal((2, 10, 11, 12, 3))).astype(np.float32)).to(dev)
    fixed = torch.tensor(rng.random((2, 10, 11, 12, 3), dtype=np.float32)).to(dev)
    flow = torch.tensor((0.5 * rng.standard_normal((2, 10, 11, 12, 3))).astype(np.float32)).to(dev).requires_grad_(True)
    three = ne.losses.multiple_losses_decorator([ne.losses.NCC(win=5).loss, ne.losses.Grad('l2').loss, ne.losses.NegJacobian(2.0).loss],
                                                [1, 0.01, 0.5])
    warped = ne.layers.SpatialTransformer()([moving, flow])
    total = three(fixed, warped)
    assert total.shape == (2,)
    g_flow, = torch.autograd.grad(total.sum(), (flow,), retain_graph=True)
    assert bool(torch.isfinite(g_flow).all()) and float(g_flow.abs().max()) > 0
    # the same in two steps: the losses' gradient at the warped tensor, then the warp's own backward
    leaf = warped.detach().requires_grad_(True)
    g_leaf, = torch.autograd.grad(three(fixed, leaf).sum(), (leaf,))
    g_two, = torch.autograd.grad(warped, (flow,), g_leaf)
    assert np.array_equal(_bits(g_flow), _bits(g_two))
    # the Jacobian term alone against float64
    w64 = warped.detach().cpu().double().requires_grad_(True)
    want = 2.0 * R.neg_loss(w64)
    assert float(want.detach().min()) > 0
    got = ne.losses.NegJacobian(2.0).loss(None, leaf)
    bound = 12 * U * R.error_scale(w64.detach())
    assert int((R.det_torch(w64.detach()).abs() <= bound).sum()) == 0, 'a voxel within the float32 bound of zero: the indicator may flip'
    assert float((got.detach().cpu().double() - want.detach()).abs().max()) <= 2.0 * 1.01 * float(bound.reshape(2, -1).mean(1).max()) + 2 * U * float(
        want.detach().abs().max())
    g64, = torch.autograd.grad(want.sum(), (w64,))
    gj, = torch.autograd.grad(got.sum(), (leaf,))
    _close(gj, g64, 'NegJacobian gradient at the warped tensor')
    # a deferred warp as y_pred is looked at like any tensor; it has 4 .. 256 channels on three axes, so its shape is refused: five axes
    # with four channels read as an unbatched 4-D field, eight channels as three axes with the wrong channel count
    for extra, error in ((1, NotImplementedError), (5, ValueError)):
        with ne.deferred.scope(True):
            lazy = ne.layers.SpatialTransformer()([torch.cat([moving] + [moving[..., :1]] * extra, -1), flow.detach()])
        assert isinstance(lazy, ne.deferred.DeferredWarp) and lazy.pending
        with pytest.raises(error):
            ne.losses.NegJacobian(2.0).loss(None, lazy)


def test_forward_and_backward_capture_into_one_graph(dev):
    ne = _ne()
    rng = np.random.default_rng(14)
    shape = (2, 9, 33, 34, 3)
    first, second = ([torch.tensor((1.5 * rng.standard_normal(s)).astype(np.float32)).to(dev) for s in (shape, shape[:-1], (2,))]
                     for _ in range(2))
    F, UP, W = (t.clone() for t in first)
    neg, metric = ne.losses.NegJacobian(0.5), ne.metrics.JacobianDeterminant()

    def step():
        f = F.detach().requires_grad_(True)                              # a leaf of this step's own stream
        det = ne.utils.jacobian_determinant(f)
        loss = neg.loss(None, f)
        g, = torch.autograd.grad((det * UP).sum() + (loss * W).sum(), (f,))
        st = metric.stats(f)
        return det.detach(), loss.detach(), g, st.folded_voxels, st.mean, st.std

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                           # workspace growth: outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    for values in (second, first, second):
        for dst, src in zip((F, UP, W), values):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        got = [_bits(t) for t in captured]
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert np.array_equal(a, _bits(b))
