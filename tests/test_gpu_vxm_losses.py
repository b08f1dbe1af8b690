"""
losses.NCC / losses.Grad (csrc/vxmloss.hip) on the GPU against the restatement of tests/vxm_loss_restatement.py: the window sums through
the C ABI, the cc map, the loss, the gradients, and the plumbing (deferred warps, multiple_losses_decorator, graph capture).  Every
forward call is made twice and the two results are compared bit for bit.

The box-sum kernel owns a tile of 8 (y) x 32 (z) outputs per plane and marches through chunks of 32 planes (x); shapes are
[B, x, y, z, C].  Which case reaches which arm:
    big      [2,21,35,70,1]  win 9        y: 5 tiles, the last of 3 rows; z: 3 tiles, the last of 6 columns; one x chunk; one channel
    chunks   [1,37,9,33,1]   win (5,3,7)  x: TWO chunks (32 + 5 planes); y: 2 tiles (8 + 1); z: 2 tiles (32 + 1); mixed odd windows
    even     [1,37,9,33,1]   win (4,9,2)  the same seams with EVEN windows (1 / 0 zeros in front; the backward mirrors them: 2 / 1)
    small    [1,5,7,6,2]     win 9        every extent below the window; two channels (the channel-loop load path)
    one      [1,5,7,6,2]     win 1        the window of one voxel: n = 2, nothing but the channel sum
    2d       [2,33,40,1]     win 9        rank 2: leading extent 1 and window 1, a march of one plane; y: 5 tiles (8 x 4 + 1)
    1d       [3,50,1]        win 9        rank 1: z only, 2 tiles (32 + 18)
    c3_w3    [2,17,12,19,3]  win 3        three channels, the smallest odd window
    c3_w15   [2,17,12,19,3]  win 15       the largest window (111 KB of LDS: the opt-in above 64 KB), wider than y; ring of 15 planes
The second kernel of `loss` adds 1 .. 15 block partials per batch entry in these cases.
Grad (rows = lines along z with their channels; a block runs 256 / lanes rows at a time):
    [2,9,10,11,3]   33-element rows on 64 lanes, per element, 23 blocks     [2,6,7,8,4]    channels % 4 == 0: 16-byte accesses
    [1,20,21,130,2] 260-element rows: a second trip along the row, 210 blocks of 2 rows
    [2,33,40,2]     rank 2                                                   [3,50,1]       rank 1, one row per batch entry
    [2,6,7,8,4] from a base pointer that is only 4-byte aligned: per element

Measured on MI355X (every test prints its ratio): sums of float images at most 0.44 of the order-free bound (the window of one voxel),
0.25 in 1-D, below 0.04 in 2-D and 3-D; the cc map at most 0.015 of its bound (1-D; 0.004 and below in 2-D and 3-D), largest |err|
4.9e-6; the loss at most 0.0081 of its bound; NCC gradients 6e-7 .. 8.1e-6 of the largest magnitude, Grad gradients at most 1.2e-7.
"""

import numpy as np
import pytest
import torch

import vxm_loss_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
CASES = {
    'big': ((2, 21, 35, 70, 1), 9),
    'chunks': ((1, 37, 9, 33, 1), (5, 3, 7)),
    'even': ((1, 37, 9, 33, 1), (4, 9, 2)),
    'small': ((1, 5, 7, 6, 2), 9),
    'one': ((1, 5, 7, 6, 2), 1),
    '2d': ((2, 33, 40, 1), 9),
    '1d': ((3, 50, 1), 9),
    'c3_w3': ((2, 17, 12, 19, 3), 3),
    'c3_w15': ((2, 17, 12, 19, 3), 15),
}
# a window of one voxel has (near) zero variance: the cc bound does not apply there, and the gradient is dominated by voxels at the clamp
FLOAT_CC_CASES = sorted(c for c in CASES if c != 'one')
GRAD_SHAPES = {'3d_c3': (2, 9, 10, 11, 3), '3d_c4': (2, 6, 7, 8, 4), '3d_long': (1, 20, 21, 130, 2), '2d': (2, 33, 40, 2), '1d': (3, 50, 1)}
_CACHE = {}


def _ne():
    import neurite_amd as ne
    return ne


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _images(tag, kind):
    """(I, J) float64 CPU tensors of a case, made once; kind 'float': uniform [0, 1) and J = 0.7 I + 0.3 noise, 'int': integers 0 .. 7"""
    key = (tag, kind)
    if key not in _CACHE:
        shape = CASES[tag][0]
        rng = np.random.default_rng(sorted(CASES).index(tag) + (100 if kind == 'int' else 0))
        if kind == 'int':
            I, J = rng.integers(0, 8, shape).astype(np.float32), rng.integers(0, 8, shape).astype(np.float32)
        else:
            I = rng.random(shape, dtype=np.float32)
            J = (np.float32(0.7) * I + np.float32(0.3) * rng.random(shape, dtype=np.float32)).astype(np.float32)
        _CACHE[key] = (torch.tensor(I, dtype=torch.float64), torch.tensor(J, dtype=torch.float64))
    return _CACHE[key]


def _ref(tag, kind):
    """float64 sums [B, *S, 5], the sums of the magnitudes of their terms, and n"""
    key = (tag, kind, 'ref')
    if key not in _CACHE:
        I, J = _images(tag, kind)
        shape, win = CASES[tag]
        n = float(np.prod(R.window_of(win, len(shape) - 2)) * shape[-1])
        _CACHE[key] = (R.ncc_sums(I, J, win).numpy(), R.ncc_sums(I, J, win, absolute=True).numpy(), n)
    return _CACHE[key]


def _abi_forward(dev, tag, kind, want_loss=True):
    """nrt_ncc_f32 with all three outputs, called twice: sums [B, *S, 5], cc [B, *S], loss [B] as numpy"""
    ne = _ne()
    L = ne._lib
    L.require_device(torch.zeros(1, device=dev))
    shape, win = CASES[tag]
    nd = len(shape) - 2
    I, J = (t.to(torch.float32).to(dev).contiguous() for t in _images(tag, kind))
    shape3 = [1] * (3 - nd) + list(shape[1:-1])
    win3 = [1] * (3 - nd) + R.window_of(win, nd)
    cs, cw = L.ints(shape3), L.ints(win3)
    nws = int(L.lib().nrt_ncc_workspace_bytes(shape[0], cs, shape[-1], cw))
    assert nws > 0
    outs = []
    for _ in range(2):
        sums = torch.full(tuple(shape[:-1]) + (5,), float('nan'), device=dev)
        cc = torch.full(tuple(shape[:-1]), float('nan'), device=dev)
        loss = torch.full((shape[0],), float('nan'), device=dev)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = L.lib().nrt_ncc_f32(L.ptr(I), L.ptr(J), shape[0], cs, shape[-1], cw, EPS, L.ptr(sums), L.ptr(cc),
                                     L.ptr(loss) if want_loss else None, L.ptr(ws) if want_loss else None, nws if want_loss else 0,
                                     L.stream_ptr(dev))
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append((sums, cc, loss))
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b)), 'not bit-identical run to run'
    return tuple(t.cpu().numpy() for t in outs[0])


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a), _bits(b)), 'not bit-identical run to run'
    return a


# ---- 1. the window sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(CASES))
def test_sums_of_integer_images_are_exact(dev, tag):
    sums, cc, _ = _abi_forward(dev, tag, 'int')
    S64, _, n = _ref(tag, 'int')
    assert S64.max() < 2 ** 24
    assert np.array_equal(sums.astype(np.float64), S64), 'window, border or tile-seam error: %d sums differ' % int((sums != S64).sum())
    # and the map is the float32 epilogue of the exact sums, bit for bit
    want = R.ncc_epilogue32(S64, n, EPS)
    assert np.array_equal(cc.view(np.int32), want.view(np.int32)), 'largest difference %g' % float(np.abs(cc - want).max())


@pytest.mark.parametrize('tag', sorted(CASES))
def test_sums_of_float_images_within_the_order_free_bound(dev, tag):
    sums, _, _ = _abi_forward(dev, tag, 'float', want_loss=False)
    S64, A64, n = _ref(tag, 'float')
    bound = (n + 2) * U * A64
    err = np.abs(sums.astype(np.float64) - S64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: sums, worst |err| / bound = %.3g' % (tag, ratio))
    assert np.all(err <= bound), ratio


# ---- 2. the cc map --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', FLOAT_CC_CASES)
def test_cc_of_float_images_within_the_derived_bound(dev, tag):
    """|cc - cc64| <= 8 (n + 4) 2^-24 (S_II / Ivar + S_JJ / Jvar) (1 + cc64): every term of cross is at most sqrt(S_II S_JJ) in size and
    |cross| <= sqrt(Ivar Jvar).  Measured on MI355X, worst |err| / bound per case: 1d 0.0147, 2d 0.0032, big 0.00045, c3_w15 0.00003,
    c3_w3 0.0035, chunks 0.0026, even 0.0039, small 0.00009 (the float32 CPU evaluation of the same expression: at most 14 / 5864)."""
    _, cc, _ = _abi_forward(dev, tag, 'float', want_loss=False)
    S64, _, n = _ref(tag, 'float')
    cc64, (c0, vI0, vJ0), (cross, Ivar, Jvar), _ = R.ncc_from_sums(torch.tensor(S64), n, EPS)
    assert bool((vI0 > EPS).all()) and bool((vJ0 > EPS).all()), 'the bound applies where both variances exceed eps: every voxel here'
    cc64 = cc64.numpy()
    bound = 8 * (n + 4) * U * (S64[..., 2] / Ivar.numpy() + S64[..., 3] / Jvar.numpy()) * (1 + cc64)
    err = np.abs(cc.astype(np.float64) - cc64)
    ratio = float((err / bound).max())
    print('%s: cc, worst |err| / bound = %.3g (largest |err| %.3g)' % (tag, ratio, float(err.max())))
    assert np.all(err <= bound), ratio
    # the class returns the same bits, with a channel axis
    ne = _ne()
    I, J = (t.to(torch.float32).to(dev) for t in _images(tag, 'float'))
    m = _twice(lambda: ne.losses.NCC(win=CASES[tag][1]).ncc(I, J))
    assert m.shape == tuple(I.shape[:-1]) + (1,)
    assert np.array_equal(_bits(m)[..., 0], cc.view(np.int32))


def test_zero_background_gives_one_and_no_gradient(dev):
    """windows that lie wholly in an exactly-zero block: every sum is 0, the three maxima clamp to eps, cc = (eps / eps) (eps / eps) = 1
    exactly, and nothing flows back"""
    ne = _ne()
    rng = np.random.default_rng(8)
    shape = (1, 24, 10, 34, 1)
    I, J = (torch.tensor(rng.random(shape, dtype=np.float32)) for _ in range(2))
    I[:, :16] = 0.0
    J[:, :16] = 0.0
    I, J = I.to(dev).requires_grad_(True), J.to(dev).requires_grad_(True)
    ncc = ne.losses.NCC(win=5)
    cc = _twice(lambda: ncc.ncc(I, J))
    assert bool((cc[:, :14] == 1.0).all())                               # windows of planes 0 .. 13 end at plane 15
    assert not bool((cc[:, 14:] == 1.0).all())
    gI, gJ = torch.autograd.grad(ncc.loss(I, J).sum(), (I, J))
    assert bool((gI[:, :12] == 0).all()) and bool((gJ[:, :12] == 0).all())    # every window that holds planes 0 .. 11 is all zero
    assert float(gI[:, 14:].abs().max()) > 0 and float(gJ[:, 14:].abs().max()) > 0
    assert bool(torch.isfinite(gI).all()) and bool(torch.isfinite(gJ).all())


# ---- 3. the loss ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(CASES))
def test_loss_is_minus_the_mean_of_the_kernels_own_map(dev, tag):
    _, cc, loss = _abi_forward(dev, tag, 'float')
    B = cc.shape[0]
    flat = cc.reshape(B, -1).astype(np.float64)
    V = flat.shape[1]
    want = -flat.mean(1)
    bound = (V + 2) * U * np.abs(flat).mean(1)
    err = np.abs(loss.astype(np.float64) - want)
    print('%s: loss, worst |err| / bound = %.3g' % (tag, float((err / bound).max())))
    assert np.all(err <= bound)
    # both reduce modes of the class
    ne = _ne()
    I, J = (t.to(torch.float32).to(dev) for t in _images(tag, 'float'))
    ncc = ne.losses.NCC(win=CASES[tag][1])
    got = _twice(lambda: ncc.loss(I, J))
    assert got.shape == (B,) and np.array_equal(_bits(got), loss.view(np.int32))
    neg = _twice(lambda: ncc.loss(I, J, reduce=None))
    assert neg.shape == tuple(I.shape[:-1]) + (1,) and np.array_equal(_bits(neg)[..., 0], (-cc).view(np.int32))


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.detach().cpu().double() - want).abs().max())
    print('%s: largest |err| / largest magnitude = %.3g' % (what, err / scale))
    assert scale > 0 and err <= 2e-4 * scale, (what, err, scale)


@pytest.mark.parametrize('tag', FLOAT_CC_CASES)
def test_ncc_gradients_against_float64_autograd(dev, tag):
    ne = _ne()
    shape, win = CASES[tag]
    I64, J64 = (t.clone().requires_grad_(True) for t in _images(tag, 'float'))
    I, J = (t.detach().to(torch.float32).to(dev).requires_grad_(True) for t in (I64, J64))
    g = torch.Generator().manual_seed(4)
    w = torch.randn(shape[0], generator=g, dtype=torch.float64)
    up = torch.randn(shape[:-1] + (1,), generator=g, dtype=torch.float64)
    ncc = ne.losses.NCC(win=win)
    # through loss
    wI, wJ = torch.autograd.grad((R.ncc_loss(I64, J64, win, EPS) * w).sum(), (I64, J64))
    gI, gJ = torch.autograd.grad((ncc.loss(I, J) * w.float().to(dev)).sum(), (I, J))
    _close(gI, wI, tag + ' loss gI')
    _close(gJ, wJ, tag + ' loss gJ')
    # through the map, with a random upstream gradient; and through -map (reduce=None)
    wI, wJ = torch.autograd.grad((R.ncc_map(I64, J64, win, EPS) * up).sum(), (I64, J64))
    gI, gJ = torch.autograd.grad((ncc.ncc(I, J) * up.float().to(dev)).sum(), (I, J))
    _close(gI, wI, tag + ' map gI')
    _close(gJ, wJ, tag + ' map gJ')
    nI, = torch.autograd.grad((ncc.loss(I, J, reduce=None) * up.float().to(dev)).sum(), (I,))
    assert np.array_equal(_bits(nI), _bits(-gI))
    # one image only
    oJ, = torch.autograd.grad((ncc.ncc(I.detach(), J) * up.float().to(dev)).sum(), (J,))
    assert np.array_equal(_bits(oJ), _bits(gJ))


def _field(tag, kind):
    shape = GRAD_SHAPES[tag]
    rng = np.random.default_rng(sorted(GRAD_SHAPES).index(tag) + 40)
    if kind == 'int':
        return torch.tensor(rng.integers(-4, 5, shape).astype(np.float32))
    return torch.tensor(rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize('penalty', ['l1', 'l2'])
@pytest.mark.parametrize('tag', sorted(GRAD_SHAPES))
def test_grad_loss_on_integer_fields_is_exact(dev, tag, penalty):
    ne = _ne()
    y = _field(tag, 'int')
    for mult in (None, 0.375):
        got = _twice(lambda: ne.losses.Grad(penalty, loss_mult=mult).loss(None, y.to(dev)))
        want = R.grad_loss32(y, penalty, mult)
        assert got.shape == (y.shape[0],)
        assert np.array_equal(_bits(got), want.view(np.int32)), (got.cpu().numpy(), want)


@pytest.mark.parametrize('penalty', ['l1', 'l2'])
@pytest.mark.parametrize('tag', sorted(GRAD_SHAPES))
def test_grad_loss_and_gradient_against_float64(dev, tag, penalty):
    ne = _ne()
    y32 = _field(tag, 'float')
    y64 = y32.double().requires_grad_(True)
    y = y32.to(dev).requires_grad_(True)
    w = torch.randn(y32.shape[0], generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for mult in (None, 2.5):
        want = R.grad_loss(y64, penalty, mult)
        got = _twice(lambda: ne.losses.Grad(penalty, loss_mult=mult).loss(None, y))
        # a mean of N terms plus a handful of operations: the order-free bound on the mean of the magnitudes (the terms are >= 0)
        n_terms = y32[0].numel()
        assert float((got.detach().cpu().double() - want.detach()).abs().max()) <= (n_terms + 8) * U * float(want.detach().abs().max())
        wy, = torch.autograd.grad((want * w).sum(), (y64,))
        gy, = torch.autograd.grad((got * w.float().to(dev)).sum(), (y,))
        _close(gy, wy, '%s %s mult %s gy' % (tag, penalty, mult))


def test_grad_l1_with_exact_ties_has_sign_zero(dev):
    """equal neighbours: d = 0, |d| passes no gradient (sign(0) = 0), exactly as torch.abs does"""
    ne = _ne()
    y32 = _field('3d_c3', 'int')
    y32[:, 2:5] = 1.0                                                    # a slab of ties along every axis
    y64 = y32.double().requires_grad_(True)
    y = y32.to(dev).requires_grad_(True)
    wy, = torch.autograd.grad(R.grad_loss(y64, 'l1').sum(), (y64,))
    gy, = torch.autograd.grad(ne.losses.Grad('l1').loss(None, y).sum(), (y,))
    assert bool((gy[:, 3] == 0).all()) and bool((wy[:, 3] == 0).all())   # the middle of the slab: six tied neighbours
    _close(gy, wy, 'ties gy')


def test_grad_from_an_unaligned_base_pointer(dev):
    """channels % 4 == 0 but a base that is only 4-byte aligned: the per-element arm, the same values"""
    ne = _ne()
    y = _field('3d_c4', 'int').to(dev)
    buf = torch.zeros(y.numel() + 1, device=dev)
    off = buf[1:].view(y.shape)
    off.copy_(y)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    for penalty in ('l1', 'l2'):
        a = ne.losses.Grad(penalty).loss(None, y)
        b = ne.losses.Grad(penalty).loss(None, off)
        assert np.array_equal(_bits(a), _bits(b))
    yl = y.clone().requires_grad_(True)
    ol = off.detach().requires_grad_(True)
    ga, = torch.autograd.grad(ne.losses.Grad('l2').loss(None, yl).sum(), (yl,))
    gb, = torch.autograd.grad(ne.losses.Grad('l2').loss(None, ol).sum(), (ol,))
    assert np.array_equal(_bits(ga), _bits(gb))


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_a_deferred_warp_as_y_pred(dev):
    ne = _ne()
    rng = np.random.default_rng(12)
    moving = torch.tensor(rng.random((1, 12, 12, 12, 4), dtype=np.float32)).to(dev)
    fixed = torch.tensor(rng.random((1, 12, 12, 12, 4), dtype=np.float32)).to(dev)
    flow = torch.tensor(rng.standard_normal((1, 12, 12, 12, 3)).astype(np.float32)).to(dev)
    with ne.deferred.scope(True):
        warped = ne.layers.SpatialTransformer()([moving, flow])
    assert isinstance(warped, ne.deferred.DeferredWarp) and warped.pending
    got = ne.losses.NCC(win=5).loss(fixed, warped)
    with ne.deferred.scope(False):
        eager = ne.layers.SpatialTransformer()([moving, flow])
    assert not isinstance(eager, ne.deferred.DeferredWarp)
    assert np.array_equal(_bits(got), _bits(ne.losses.NCC(win=5).loss(fixed, eager)))
    with ne.deferred.scope(True):
        warped = ne.layers.SpatialTransformer()([moving, flow])
    assert np.array_equal(_bits(ne.losses.Grad('l2').loss(None, warped)), _bits(ne.losses.Grad('l2').loss(None, eager)))


def test_multiple_losses_decorator_backward_to_the_flow_of_a_warp(dev):
    ne = _ne()
    rng = np.random.default_rng(13)
    moving = torch.tensor(rng.random((2, 10, 11, 12, 1), dtype=np.float32)).to(dev)
    fixed = torch.tensor(rng.random((2, 10, 11, 12, 1), dtype=np.float32)).to(dev)
    flow = torch.tensor((0.5 * rng.standard_normal((2, 10, 11, 12, 3))).astype(np.float32)).to(dev).requires_grad_(True)
    both = ne.losses.multiple_losses_decorator([ne.losses.NCC(win=5).loss, ne.losses.Grad('l2').loss], [1, 0.01])
    warped = ne.layers.SpatialTransformer()([moving, flow])
    total = both(fixed, warped)
    assert total.shape == (2,)
    g_flow, = torch.autograd.grad(total.sum(), (flow,), retain_graph=True)
    assert bool(torch.isfinite(g_flow).all()) and float(g_flow.abs().max()) > 0
    # the same in two steps: the losses' gradient at the warped image, then the warp's own backward
    leaf = warped.detach().requires_grad_(True)
    g_leaf, = torch.autograd.grad(both(fixed, leaf).sum(), (leaf,))
    g_two, = torch.autograd.grad(warped, (flow,), g_leaf)
    assert np.array_equal(_bits(g_flow), _bits(g_two))
    w64 = warped.detach().cpu().double().requires_grad_(True)
    want = R.ncc_loss(fixed.cpu().double(), w64, 5, EPS) + 0.01 * R.grad_loss(w64, 'l2')
    assert float((total.detach().cpu().double() - want.detach()).abs().max()) <= 1e-5 * float(want.detach().abs().max())
    g64, = torch.autograd.grad(want.sum(), (w64,))
    _close(g_leaf, g64, 'decorator gradient at the warped image')


@pytest.mark.parametrize('win', [(4, 9, 2), 9], ids=['even', 'w9'])      # 41 KB and 69 KB of LDS: the second opts in above 64 KB, in the capture too
def test_forward_and_backward_capture_into_one_graph(dev, win):
    ne = _ne()
    rng = np.random.default_rng(14)
    shape = (1, 37, 9, 33, 1)
    first, second = ([torch.tensor(rng.random(s, dtype=np.float32)).to(dev) for s in (shape, shape, shape[:-1] + (3,))] for _ in range(2))
    I, J, F = (t.clone() for t in first)
    ncc, grad = ne.losses.NCC(win=win), ne.losses.Grad('l1', loss_mult=0.5)

    def step():
        i, j, f = (t.detach().requires_grad_(True) for t in (I, J, F))   # leaves of this step's own stream
        loss = ncc.loss(i, j) + grad.loss(None, f)
        return (loss.detach(),) + torch.autograd.grad(loss.sum(), (i, j, f))

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
        for dst, src in zip((I, J, F), values):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        got = [_bits(t) for t in captured]
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert np.array_equal(a, _bits(b))
