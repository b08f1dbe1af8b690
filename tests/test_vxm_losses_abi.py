"""
CPU tests of losses.NCC / losses.Grad (no kernel is launched): the five entry points of csrc/vxmloss.hip are declared, typed and exported
and refuse bad arguments before any launch; the classes are public, validate their arguments on the host and refuse CPU tensors; and
the restatement the GPU tests compare against (tests/vxm_loss_restatement.py) agrees with itself: the backward's analytic formula
against float64 autograd, exactly representable window sums on the integer images the bit-for-bit tests use, the closed form of Grad on
a linear ramp.
"""

import numpy as np
import pytest
import torch

import vxm_loss_restatement as R

ENTRY_POINTS = ['nrt_ncc_workspace_bytes', 'nrt_ncc_f32', 'nrt_ncc_bwd_f32', 'nrt_grad_loss_f32', 'nrt_grad_loss_bwd_f32']
D = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
BIG = 1 << 40


def _L():
    from neurite_amd import _lib
    return _lib


def _ncc(I=D, J=D, batch=2, shape=(5, 6, 7), channels=1, win=(3, 3, 3), eps=1e-5, sums=D, cc=D, loss=D, ws=D, nws=BIG,
         shape_null=False, win_null=False):
    L = _L()
    return L.lib().nrt_ncc_f32(I, J, batch, None if shape_null else L.ints(shape), channels, None if win_null else L.ints(win), eps, sums,
                               cc, loss, ws, nws, None)


def _ncc_bwd(I=D, J=D, gcc=D, gloss=D, batch=2, shape=(5, 6, 7), channels=1, win=(3, 3, 3), eps=1e-5, gI=D, gJ=D, ws=D, nws=BIG,
             shape_null=False, win_null=False):
    L = _L()
    return L.lib().nrt_ncc_bwd_f32(I, J, gcc, gloss, batch, None if shape_null else L.ints(shape), channels,
                                   None if win_null else L.ints(win), eps, gI, gJ, ws, nws, None)


def _ncc_bytes(batch=2, shape=(5, 6, 7), channels=1, win=(3, 3, 3)):
    L = _L()
    return L.lib().nrt_ncc_workspace_bytes(batch, L.ints(shape), channels, L.ints(win))


def _grad(y=D, batch=2, shape=(5, 6, 7), nd=3, channels=3, penalty=1, mult=1.0, loss=D, ws=D, nws=BIG, shape_null=False):
    L = _L()
    return L.lib().nrt_grad_loss_f32(y, batch, None if shape_null else L.ints(shape), nd, channels, penalty, mult, loss, ws, nws, None)


def _grad_bwd(y=D, gloss=D, batch=2, shape=(5, 6, 7), nd=3, channels=3, penalty=1, mult=1.0, gy=D, shape_null=False):
    L = _L()
    return L.lib().nrt_grad_loss_bwd_f32(y, gloss, batch, None if shape_null else L.ints(shape), nd, channels, penalty, mult, gy, None)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_null_pointers_and_non_positive_sizes_are_invalid_arguments():
    inv = _L().NRT_ERR_INVALID_ARG
    for kw in ({'I': None}, {'J': None}, {'shape_null': True}, {'win_null': True}, {'sums': None, 'cc': None, 'loss': None},
               {'batch': 0}, {'batch': -1}, {'shape': (5, 0, 7)}, {'shape': (-5, 6, 7)}, {'eps': -1.0}, {'eps': float('nan')}):
        assert _ncc(**kw) == inv, kw
    for kw in ({'I': None}, {'J': None}, {'shape_null': True}, {'win_null': True}, {'gcc': None, 'gloss': None}, {'gI': None, 'gJ': None},
               {'batch': 0}, {'shape': (5, 6, 0)}):
        assert _ncc_bwd(**kw) == inv, kw
    for kw in ({'batch': 0}, {'shape': (0, 6, 7)}):
        assert _ncc_bytes(**kw) == 0, kw
    for kw in ({'y': None}, {'loss': None}, {'shape_null': True}, {'batch': 0}, {'channels': 0}, {'shape': (5, 6, 0)}, {'nd': 0}, {'nd': 4},
               {'penalty': 0}, {'penalty': 3}, {'nd': 2}, {'nd': 1, 'shape': (1, 6, 7)}):          # nd < 3 needs leading extents of 1
        assert _grad(**kw) == inv, kw
    for kw in ({'y': None}, {'gloss': None}, {'gy': None}, {'shape_null': True}, {'batch': -3}, {'channels': 0}, {'nd': 4}, {'penalty': 0},
               {'nd': 2}):
        assert _grad_bwd(**kw) == inv, kw
    # each single optional tensor may be missing
    ok_or_ws = (_L().NRT_ERR_WORKSPACE,)
    assert _ncc(loss=D, sums=None, cc=None, ws=None, nws=0) in ok_or_ws
    assert _ncc_bwd(gcc=None, ws=None, nws=0) in ok_or_ws and _ncc_bwd(gloss=None, gJ=None, ws=None, nws=0) in ok_or_ws


def test_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    for kw in ({'win': (0, 3, 3)}, {'win': (3, 3, 16)}, {'win': (3, 16, 3)}, {'win': (-1, 3, 3)}, {'channels': 0}, {'channels': 17},
               {'batch': 1, 'shape': (1 << 10, 1 << 10, 1 << 11)},                       # 2^31 voxels
               {'batch': 2, 'shape': (1 << 10, 1 << 10, 1 << 10)},
               {'batch': 1, 'shape': (1 << 10, 1 << 10, 1 << 9), 'channels': 4},          # 2^31 elements
               {'batch': 1, 'shape': (1 << 30, 1 << 30, 1 << 30)}):
        assert _ncc(**kw) == unsup, kw
        assert _ncc_bwd(**kw) == unsup, kw
        kb = {k: v for k, v in kw.items()}
        assert _ncc_bytes(**kb) == 0, kw
    for kw in ({'batch': 1, 'shape': (1 << 10, 1 << 10, 1 << 10), 'channels': 2}, {'batch': 4, 'shape': (1 << 10, 1 << 10, 1 << 9), 'channels': 1},
               {'batch': 1, 'shape': (1 << 20, 1 << 20, 1 << 20), 'channels': 1}):
        assert _grad(**kw) == unsup, kw
        assert _grad_bwd(**kw) == unsup, kw
    # just inside: windows 1 and 15, 16 channels, 2^31 - 2^21 elements
    assert _ncc_bytes(win=(1, 15, 1), channels=16) > 0
    assert _ncc_bytes(batch=1, shape=(1 << 10, 1 << 10, (1 << 11) - 2), channels=1) > 0


def test_missing_or_short_workspace_is_refused():
    ws = _L().NRT_ERR_WORKSPACE
    need = _ncc_bytes()
    assert need >= 2 * 5 * 6 * 7 * 5 * 4                                # the backward's five coefficient fields per voxel
    assert _ncc(ws=None, nws=0) == ws and _ncc(ws=None, nws=BIG) == ws and _ncc(ws=256, nws=4) == ws
    assert _ncc_bwd(ws=None, nws=0) == ws and _ncc_bwd(ws=256, nws=need - 1) == ws
    assert _grad(ws=None, nws=0) == ws and _grad(ws=256, nws=2 * 6144 - 1) == ws


def test_classes_are_public():
    import neurite_amd as ne
    assert 'NCC' in ne.losses.__all__ and 'Grad' in ne.losses.__all__
    n = ne.losses.NCC()
    assert n.win is None and n.eps == 1e-5
    g = ne.losses.Grad()
    assert g.penalty == 'l1' and g.loss_mult is None


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    a, b = torch.rand(2, 5, 6, 7, 1), torch.rand(2, 5, 6, 7, 1)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.NCC().loss(a, b)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.NCC(win=3).ncc(a, b)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.NCC().loss(a, b, reduce=None)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.Grad('l2').loss(None, torch.rand(2, 5, 6, 7, 3))
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.multiple_losses_decorator([ne.losses.NCC().loss, ne.losses.Grad('l2').loss], [1, 0.01])(a, b)


def test_host_side_argument_errors():
    import neurite_amd as ne
    NCC, Grad = ne.losses.NCC, ne.losses.Grad
    a = torch.rand(2, 5, 6, 7, 1)
    for win in (0, -3, (3, 0, 3), 2.5, (3, 3.0, 3), 'nine', (), True):
        with pytest.raises(ValueError):
            NCC(win=win)
    for win in (16, (3, 3, 99)):
        with pytest.raises(NotImplementedError):
            NCC(win=win)
    with pytest.raises(ValueError):
        NCC(eps=-1.0)
    with pytest.raises(ValueError):
        NCC().loss(a, a, reduce='sum')
    with pytest.raises(ValueError):
        NCC(win=(3, 3)).loss(a, a)                                      # two windows, three spatial axes
    with pytest.raises(ValueError):
        NCC().loss(a, torch.rand(2, 5, 6, 8, 1))                        # shapes differ
    with pytest.raises(ValueError):
        NCC().loss(torch.rand(2, 5), torch.rand(2, 5))                  # no spatial axis
    with pytest.raises(ValueError):
        NCC().loss(torch.rand(2, 3, 4, 5, 6, 1), torch.rand(2, 3, 4, 5, 6, 1))
    with pytest.raises(TypeError):
        NCC().loss(a.numpy(), a)
    for dtype in (torch.float64, torch.bfloat16, torch.float16, torch.int32):
        with pytest.raises(NotImplementedError):                        # before any launch, whatever the device
            NCC().loss(a.to(dtype), a.to(dtype))
        with pytest.raises(NotImplementedError):
            Grad().loss(None, torch.zeros(2, 5, 6, 7, 3).to(dtype))
    for penalty in ('l3', 'L1', None, 1):
        with pytest.raises(ValueError):
            Grad(penalty)
    with pytest.raises(NotImplementedError):
        Grad('l1', vox_weight=torch.ones(5, 6, 7))
    with pytest.raises(ValueError):
        Grad().loss(None, torch.rand(2, 5))


# ---- the restatement against itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,win', [((2, 7, 9, 8, 1), 5), ((1, 6, 7, 5, 2), (4, 3, 2)), ((2, 11, 13, 1), (4, 5)), ((3, 17, 3), 9),
                                       ((1, 4, 5, 6, 1), 9)],
                         ids=['3d_w5', '3d_even_c2', '2d_even', '1d_c3', 'below_win'])
def test_analytic_gradient_equals_float64_autograd(shape, win):
    g = torch.Generator().manual_seed(11)
    I = torch.rand(shape, generator=g, dtype=torch.float64)
    J = (0.7 * I + 0.3 * torch.rand(shape, generator=g, dtype=torch.float64))
    I[0, :3] = 0.0                                                      # a stretch where the maxima clamp
    J[0, :3] = 0.0
    I.requires_grad_(True)
    J.requires_grad_(True)
    up = torch.randn(shape[:-1], generator=g, dtype=torch.float64)
    cc = R.ncc_map(I, J, win)
    gI, gJ = torch.autograd.grad((cc[..., 0] * up).sum(), (I, J))
    aI, aJ = R.ncc_grad_analytic(I.detach(), J.detach(), up, win)
    scale = max(float(gI.abs().max()), float(gJ.abs().max()))
    assert scale > 0
    assert float((gI - aI).abs().max()) <= 1e-12 * scale and float((gJ - aJ).abs().max()) <= 1e-12 * scale
    # through the loss: the upstream gradient of cc is -gloss[b] / V
    w = torch.randn(shape[0], generator=g, dtype=torch.float64)
    lI, lJ = torch.autograd.grad((R.ncc_loss(I, J, win) * w).sum(), (I, J))
    V = int(np.prod(shape[1:-1]))
    up = (-w / V).reshape((-1,) + (1,) * (len(shape) - 2)).expand(shape[:-1])
    aI, aJ = R.ncc_grad_analytic(I.detach(), J.detach(), up, win)
    scale = max(float(lI.abs().max()), float(lJ.abs().max()))
    assert float((lI - aI).abs().max()) <= 1e-12 * scale and float((lJ - aJ).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize('shape,win', [((1, 12, 11, 13, 1), 9), ((1, 16, 17, 18, 3), 15), ((2, 9, 8, 7, 3), 9), ((1, 9, 10, 2), (4, 9))],
                         ids=['w9', 'w15_c3', 'w9_c3', '2d_even'])
def test_integer_images_give_exactly_representable_sums(shape, win):
    rng = np.random.default_rng(5)
    I = torch.tensor(rng.integers(0, 8, shape).astype(np.float64))
    J = torch.tensor(rng.integers(0, 8, shape).astype(np.float64))
    S = R.ncc_sums(I, J, win).numpy()
    assert S.max() < 2 ** 24 and S.min() >= 0
    assert np.array_equal(S, np.round(S)) and np.array_equal(S.astype(np.float32).astype(np.float64), S)
    # and the float32 epilogue of exact sums is the float64 one up to rounding
    n = float(np.prod(R.window_of(win, len(shape) - 2)) * shape[-1])
    cc32 = R.ncc_epilogue32(S, n, 1e-5)
    cc64 = R.ncc_map(I, J, win)[..., 0].numpy()
    assert cc32.shape == cc64.shape and np.all(np.isfinite(cc32))
    ok = R.ncc_from_sums(torch.tensor(S), n, 1e-5)[1]
    well = ((ok[1] > 1.0) & (ok[2] > 1.0)).numpy()                      # away from the clamp the two agree closely
    assert well.any() and np.abs(cc32 - cc64)[well].max() <= 1e-3 * (1 + np.abs(cc64[well]).max())


def test_zero_windows_give_one():
    z = torch.zeros(1, 6, 6, 6, 1, dtype=torch.float64)
    assert torch.equal(R.ncc_map(z, z, 3), torch.ones(1, 6, 6, 6, 1, dtype=torch.float64))
    assert np.array_equal(R.ncc_epilogue32(np.zeros((4, 5), np.float32), 27.0, 1e-5), np.ones(4, np.float32))


@pytest.mark.parametrize('penalty', ['l1', 'l2'])
def test_grad_on_a_linear_ramp_has_the_closed_form(penalty):
    # y[b, i, j, k, c] = a_c i + b_c j + c_c k: every difference along an axis is that axis' slope
    slopes = torch.tensor([[1.0, -2.0, 0.5], [3.0, 0.25, -1.0], [-4.0, 2.0, 8.0]], dtype=torch.float64)   # [axis, channel]
    shape = (5, 6, 7)
    grids = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing='ij')
    y = sum(g.unsqueeze(-1) * slopes[a] for a, g in enumerate(grids)).unsqueeze(0).repeat(2, 1, 1, 1, 1)
    per_axis = slopes.abs().mean(1) if penalty == 'l1' else (slopes ** 2).mean(1)
    want = float(per_axis.sum() / 3)
    got = R.grad_loss(y, penalty)
    assert got.shape == (2,) and torch.allclose(got, torch.full((2,), want, dtype=torch.float64), rtol=1e-14, atol=0)
    assert torch.allclose(R.grad_loss(y, penalty, loss_mult=2.5), torch.full((2,), 2.5 * want, dtype=torch.float64), rtol=1e-14, atol=0)
    got32 = R.grad_loss32(y, penalty, loss_mult=2.5)
    assert got32.dtype == np.float32 and np.allclose(got32, 2.5 * want, rtol=1e-6, atol=0)
    # lower ranks: 2-D and 1-D ramps
    y2 = y[:, 0, :, :, :2] - y[:, 0, :1, :1, :2]
    per2 = slopes[1:, :2].abs().mean(1) if penalty == 'l1' else (slopes[1:, :2] ** 2).mean(1)
    assert torch.allclose(R.grad_loss(y2, penalty), torch.full((2,), float(per2.sum() / 2), dtype=torch.float64), rtol=1e-14, atol=0)
    y1 = y[:, 0, 0, :, :]
    per1 = slopes[2].abs().mean() if penalty == 'l1' else (slopes[2] ** 2).mean()
    assert torch.allclose(R.grad_loss(y1, penalty), torch.full((2,), float(per1), dtype=torch.float64), rtol=1e-14, atol=0)
