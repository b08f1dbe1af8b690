"""
CPU tests of utils.jacobian_determinant / metrics.JacobianDeterminant / losses.NegJacobian (no kernel is launched): the three entry
points of csrc/jacobian.hip are declared, typed and exported and refuse bad arguments before any launch; the Python entry points
validate on the host and refuse CPU tensors; and the restatement the GPU tests compare against (tests/jacobian_restatement.py) agrees
with itself: the torch form against the NumPy form on np.gradient (difference 0 in float64), the gather formula of the backward
against float64 autograd, and even-integer fields give determinants that float32 holds exactly.
"""

import numpy as np
import pytest
import torch

import jacobian_restatement as R

ENTRY_POINTS = ['nrt_jacdet_workspace_bytes', 'nrt_jacdet_f32', 'nrt_jacdet_bwd_f32']
D = 16                                             # a non-NULL, 8-byte aligned "pointer"; nothing is launched on an argument error
BIG = 1 << 40
SHAPES = [(2, 2, 2), (3, 2, 5), (5, 6, 7), (9, 33, 34), (2, 3), (17, 65)]


def _L():
    from neurite_amd import _lib
    return _lib


def _fwd(disp=D, batch=2, shape=(5, 6, 7), nd=None, det=D, stats=D, loss=D, ws=D, nws=BIG, shape_null=False):
    L = _L()
    return L.lib().nrt_jacdet_f32(disp, batch, None if shape_null else L.ints(shape), len(shape) if nd is None else nd, det, stats, loss,
                                  ws, nws, None)


def _bwd(disp=D, gdet=D, gloss=D, batch=2, shape=(5, 6, 7), nd=None, gdisp=D, shape_null=False):
    L = _L()
    return L.lib().nrt_jacdet_bwd_f32(disp, gdet, gloss, batch, None if shape_null else L.ints(shape), len(shape) if nd is None else nd,
                                      gdisp, None)


def _bytes(batch=2, shape=(5, 6, 7), nd=None):
    L = _L()
    return L.lib().nrt_jacdet_workspace_bytes(batch, L.ints(shape), len(shape) if nd is None else nd)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_invalid_arguments_are_refused_before_any_launch():
    inv = _L().NRT_ERR_INVALID_ARG
    for kw in ({'disp': None}, {'shape_null': True}, {'det': None, 'stats': None, 'loss': None}, {'batch': 0}, {'batch': -2},
               {'shape': (5, 1, 7)}, {'shape': (1, 6, 7)}, {'shape': (5, 6, 1)}, {'shape': (1, 6)}, {'shape': (5, 0, 7)},
               {'shape': (5, -6, 7)}, {'stats': 20}):                                       # a stats row holds 8-byte values
        assert _fwd(**kw) == inv, kw
    for kw in ({'disp': None}, {'shape_null': True}, {'gdet': None, 'gloss': None}, {'gdisp': None}, {'batch': 0}, {'shape': (5, 1, 7)},
               {'shape': (6, 1)}):
        assert _bwd(**kw) == inv, kw
    for kw in ({'batch': 0}, {'shape': (5, 1, 7)}, {'shape': (2, 1)}):
        assert _bytes(**kw) == 0, kw
    # each single output may be missing; one upstream gradient is enough (the workspace check comes last: nothing was launched)
    ws = _L().NRT_ERR_WORKSPACE
    assert _fwd(det=None, loss=None, ws=None, nws=0) == ws and _fwd(det=None, stats=None, ws=None, nws=0) == ws


def test_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    for kw in ({'shape': (7,), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 4}, {'shape': (5, 6, 7), 'nd': 0},
               {'batch': 65536, 'shape': (2, 2)},
               {'batch': 1, 'shape': (1 << 10, 1 << 10, 1 << 11)},                        # 2^31 voxels
               {'batch': 1, 'shape': (1 << 10, 1 << 10, 1 << 10)},                        # 2^30 voxels, 3 * 2^30 elements
               {'batch': 1, 'shape': (1 << 15, 1 << 15)},                                 # 2^30 voxels, 2^31 elements
               {'batch': 4, 'shape': (1 << 10, 1 << 10, 1 << 8)},                         # 2^30 voxels in the batch
               {'batch': 1, 'shape': (1 << 30, 1 << 30, 1 << 30)}):
        assert _fwd(**kw) == unsup, kw
        assert _bwd(**kw) == unsup, kw
        assert _bytes(**kw) == 0, kw
    # just inside: 65535 batch entries; 2^31 - 2^16 elements
    assert _bytes(batch=65535, shape=(2, 2)) > 0
    assert _bytes(batch=1, shape=(1 << 15, (1 << 15) - 1)) > 0


def test_missing_or_short_workspace_is_refused():
    ws = _L().NRT_ERR_WORKSPACE
    need = _bytes()
    assert need > 0
    assert _fwd(ws=None, nws=0) == ws and _fwd(ws=None, nws=BIG) == ws and _fwd(ws=256, nws=need - 1) == ws
    assert _bytes(batch=3, shape=(9, 33, 34)) >= 3 * _bytes(batch=1, shape=(9, 33, 34)) > 0


def test_python_entry_points_are_public():
    import neurite_amd as ne
    assert 'jacobian_determinant' in ne.utils.__all__
    assert 'JacobianDeterminant' in ne.metrics.__all__ and 'NegJacobian' in ne.losses.__all__
    assert ne.losses.NegJacobian().loss_mult is None and ne.losses.NegJacobian(0.5).loss_mult == 0.5
    assert ne.metrics.JacobianStats._fields == ('folded_voxels', 'folded_fraction', 'min', 'max', 'mean', 'std')


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    f3, f2, f3u = torch.rand(2, 5, 6, 7, 3), torch.rand(2, 5, 6, 2), torch.rand(5, 6, 7, 3)
    M = ne.metrics.JacobianDeterminant()
    for f in (f3, f2, f3u):
        for fn in (ne.utils.jacobian_determinant, M.det, M.stats, M.folded, lambda t: ne.losses.NegJacobian().loss(None, t)):
            with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                fn(f)
    both = ne.losses.multiple_losses_decorator([ne.losses.Grad('l2').loss, ne.losses.NegJacobian(2.0).loss], [1, 0.1])
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        both(None, f3)


def test_host_side_argument_errors():
    import neurite_amd as ne
    M = ne.metrics.JacobianDeterminant()
    fns = (ne.utils.jacobian_determinant, M.det, M.stats, M.folded, lambda t: ne.losses.NegJacobian().loss(None, t))
    for fn in fns:
        for dtype in (torch.float64, torch.bfloat16, torch.float16, torch.int32):         # before any launch, whatever the device
            with pytest.raises(NotImplementedError):
                fn(torch.zeros(2, 5, 6, 7, 3).to(dtype))
        for shape in ((2, 5, 6, 7, 2), (2, 5, 6, 7, 1), (5, 6, 7, 4)):                     # channels != spatial axes
            with pytest.raises(ValueError):
                fn(torch.zeros(shape))
        for shape in ((2, 5, 1, 7, 3), (1, 6, 7, 3), (2, 1, 6, 2), (5, 1, 2)):             # an extent of 1, as np.gradient refuses it
            with pytest.raises(ValueError):
                fn(torch.zeros(shape))
        for shape in ((2, 9, 1), (9, 1), (2, 3, 4, 5, 6, 4), (3, 4, 5, 6, 4)):             # 1-D and 4-D
            with pytest.raises(NotImplementedError):
                fn(torch.zeros(shape))
        with pytest.raises(ValueError):
            fn(torch.zeros(3))
        with pytest.raises(TypeError):
            fn(np.zeros((5, 6, 7, 3), np.float32))
    with pytest.raises(ValueError):
        R.det_numpy(np.zeros((5, 1, 7, 3)))                                                # the oracle refuses the same


# ---- the restatement against itself --------------------------------------------------------------------------------------------------
def _field64(shape, amp, seed, batch=2):
    """float32 values held in float64, as VoxelMorph sees a float32 field after the integer grid has promoted it: there disp + grid
    and every difference are exact, which is what makes G + identity the same numbers as np.gradient(disp + grid)"""
    rng = np.random.default_rng(seed)
    return torch.tensor((amp * rng.standard_normal((batch,) + tuple(shape) + (len(shape),))).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize('shape', SHAPES + [(40, 40, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_torch_form_equals_the_numpy_form(shape):
    for amp in (0.05, 1.5, 20.0):
        f = _field64(shape, amp, 3)
        got = R.det_torch(f).numpy()
        for b in range(f.shape[0]):
            want = R.det_numpy(f[b].numpy())
            assert want.dtype == np.float64 and float(np.abs(got[b] - want).max()) == 0.0
        # float32 input: VoxelMorph's own result is float64 (the integer grid promotes)
        assert R.det_numpy(f[0].numpy().astype(np.float32)).dtype == np.float64


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gather_formula_equals_float64_autograd(shape):
    f = _field64(shape, 1.5, 5).requires_grad_(True)
    g = torch.Generator().manual_seed(6)
    up = torch.randn(f.shape[:-1], generator=g, dtype=torch.float64)
    want, = torch.autograd.grad((R.det_torch(f) * up).sum(), (f,))
    got = R.grad_analytic(f.detach(), up)
    scale = float(want.abs().max())
    assert scale > 0 and float((got - want).abs().max()) <= 1e-12 * scale
    # through the loss: w[p] = -gloss[b] / V [det[p] < 0]
    wl = torch.randn(f.shape[0], generator=g, dtype=torch.float64)
    want, = torch.autograd.grad((R.neg_loss(f) * wl).sum(), (f,))
    det = R.det_torch(f.detach())
    assert bool((det < 0).any()) and bool((det > 0).any())
    V = det[0].numel()
    w = (-wl / V).reshape((-1,) + (1,) * len(shape)) * (det < 0)
    got = R.grad_analytic(f.detach(), w)
    scale = float(want.abs().max())
    assert scale > 0 and float((got - want).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_even_integer_fields_give_determinants_exact_in_float32(shape):
    rng = np.random.default_rng(7)
    f = R.even_integer_field((3,) + tuple(shape) + (len(shape),), rng)
    det = R.det_torch(torch.tensor(f, dtype=torch.float64)).numpy()
    assert np.array_equal(det * 8, np.round(det * 8)), 'multiples of 1/8'
    assert np.array_equal(det.astype(np.float32).astype(np.float64), det)
    if det.size >= 100:
        folded = float((det <= 0).mean())
        assert 0.3 < folded < 0.6, folded
    # the float32 evaluation of the same operation order gives the same numbers
    det32 = R.det_torch(torch.tensor(f)).numpy()
    assert det32.dtype == np.float32 and np.array_equal(det32.astype(np.float64), det)
    # and so do the cofactors and what the backward adds up
    f64 = torch.tensor(f, dtype=torch.float64)
    g = R.grad_analytic(f64, (torch.tensor(det) < 0).to(torch.float64)).numpy()
    assert np.array_equal(g * 2, np.round(g * 2)) and float(np.abs(g).max()) < 2 ** 20


def test_float32_error_stays_under_the_derived_bound():
    """the float32 evaluation (one subtraction, an exact * 0.5, one + 1, then the expansion) against float64: at most
    12 * 2^-24 * error_scale; a scale built on |J| instead of |G| + delta would fail"""
    for shape in SHAPES:
        for amp in (0.05, 0.3, 1.5, 20.0):
            f32 = _field64(shape, amp, 9).to(torch.float32)
            d32 = R.det_torch(f32).double()
            d64 = R.det_torch(f32.double())
            bound = 12 * 2.0 ** -24 * R.error_scale(f32.double())
            assert bool(((d32 - d64).abs() <= bound).all()), (shape, amp, float(((d32 - d64).abs() / bound).max()))
