"""
GPU tests of the affine warp (csrc/affine_warp.hip, fused.affine_warp, SpatialTransformer on an affine input).

Forward: bit for bit the two-kernel path -- utils.affine_to_dense_shift, then SpatialTransformer on the dense field -- for every shape,
channel count and matrix of tests/affine_warp_cases.py, both methods, with and without a fill value, shift_center and single_transform.
Matrix gradient: against float64 at the device's own float32 sampling locations (affine_warp_cases.matrix_gradient_f64), at the
criterion of tests/test_gpu_backward.py: max error below 1e-4 of the gradient's largest magnitude.  Then determinism, the volume
gradient against the dense-field path, and graph capture.  Every test first asserts that recipe (c) sends 5 % to 50 % of the output
voxels out of bounds, so that the clamp and the fill arm both run.
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import deferred, fused, utils

import affine_warp_cases as AW

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _dense_path(vol, M, O, method, fill, shift_center, single):
    """the parent path: the materialised field, then the warp kernels"""
    nb = 1 if single else M.shape[0]
    with torch.no_grad(), deferred.scope(False):
        shift = utils.affine_to_dense_shift(M[:nb], list(O), shift_center=shift_center)
        return ne.layers.SpatialTransformer(interp_method=method, fill_value=fill, single_transform=single)([vol, shift])


def _case(dev, name, C, seed=7):
    S, O, B, _ = AW.SHAPES[name]
    AW.assert_recipe_c_crosses_the_border(S, O, B)
    vol = torch.tensor(AW.volume(S, B, C, seed), device=dev)
    mats = {k: torch.tensor(v, device=dev) for k, v in AW.matrices(len(S), B).items()}
    return S, O, B, vol, mats


@pytest.mark.parametrize('name,C', AW.SHAPE_CHANNELS)
def test_forward_is_the_two_kernel_path_bit_for_bit(dev, name, C):
    S, O, B, vol, mats = _case(dev, name, C)
    shape = None if O == S else O
    for mname, M in mats.items():
        for method in ('linear', 'nearest'):
            for fill in (None, 0.5):
                for shift_center in (True, False):
                    for single in (False, True):
                        got = fused.affine_warp(vol, M, shape=shape, interp_method=method, fill_value=fill, shift_center=shift_center,
                                                single_transform=single)
                        want = _dense_path(vol, M, O, method, fill, shift_center, single)
                        assert got.shape == want.shape and torch.equal(got, want), (mname, method, fill, shift_center, single)
    # the identity on the volume's own grid returns the volume
    assert torch.equal(fused.affine_warp(vol, mats['identity']), vol)
    assert torch.equal(fused.affine_warp(vol, mats['identity'], interp_method='nearest', fill_value=0.5, shift_center=False), vol)


@pytest.mark.parametrize('name', ['3d_shape', '2d'])
def test_four_channels_off_the_16_byte_grid(dev, name):
    # a volume that starts 4 bytes past a 16-byte boundary: the one-channel items, the same bits and the same gradient
    S, O, B, vol, mats = _case(dev, name, 4)
    shape = None if O == S else O
    flat = torch.empty(vol.numel() + 1, device=dev)
    off = flat[1:].view(vol.shape)
    off.copy_(vol)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    w = torch.tensor(np.random.default_rng(15).standard_normal((B,) + tuple(O) + (4,)).astype(np.float32), device=dev)
    for method in ('linear', 'nearest'):
        got = fused.affine_warp(off, mats['c'], shape=shape, interp_method=method, fill_value=0.5)
        assert torch.equal(got, fused.affine_warp(vol, mats['c'], shape=shape, interp_method=method, fill_value=0.5))
        assert torch.equal(got, _dense_path(vol, mats['c'], O, method, 0.5, True, False))
    a, b = _gpu_matrix_grad(off, mats['c'], w, shape, 0.5, True, False), _gpu_matrix_grad(vol, mats['c'], w, shape, 0.5, True, False)
    scale = float(b.abs().max())
    assert scale > 0 and float((a - b).abs().max()) <= TOL * scale


@pytest.mark.parametrize('name,C', [('3d', 1), ('3d_shape', 32), ('2d', 3), ('2d_shape', 4)])
def test_spatial_transformer_sends_affines_to_the_kernel(dev, name, C):
    S, O, B, vol, mats = _case(dev, name, C)
    for mname in ('c', 'c_square', 'translation'):
        for fill, single in ((None, False), (0.5, True)):
            st = ne.layers.SpatialTransformer(fill_value=fill, single_transform=single, shape=None if O == S else O)
            want = _dense_path(vol, mats[mname], O, 'linear', fill, True, single)
            with deferred.scope(False):
                plain = st([vol, mats[mname]])
                M = mats[mname].clone().requires_grad_()
                tracked = st([vol, M])
            assert torch.equal(plain, want) and torch.equal(tracked.detach(), want), (mname, fill, single)
            assert plain.grad_fn is None and type(tracked.grad_fn).__name__.startswith('_AffineWarpFn'), type(tracked.grad_fn).__name__
            tracked.sum().backward()
            assert M.grad is not None and M.grad.shape == M.shape
            if single:
                assert float(M.grad[1:].abs().max()) == 0.0               # only the first matrix warps
            if mname == 'c_square':
                assert float(M.grad[:, -1].abs().max()) == 0.0            # the last row of the square form is not read


def test_which_affine_inputs_take_the_single_kernel(dev, monkeypatch):
    # every route gives the same bits, so the route itself is observed: calls of fused.affine_warp
    calls = []
    real = fused.affine_warp
    monkeypatch.setattr(fused, 'affine_warp', lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def taken(vol, M, **kw):
        del calls[:]
        with deferred.scope(False):
            out = ne.layers.SpatialTransformer(**kw)([vol, M])
        assert torch.equal(out.detach(), _dense_path(vol, M.detach(), vol.shape[1:-1], kw.get('interp_method', 'linear'),
                                                     kw.get('fill_value'), True, False)) or kw.get('indexing') == 'xy'
        return len(calls) == 1

    for C in (1, 3, 4, 16, 256):
        S, O, B, vol, mats = _case(dev, '3d', C)
        assert taken(vol, mats['c']) and taken(vol, mats['c'], interp_method='nearest', fill_value=0.5)
    for C in (32, 64, 128):                                # the linear forward loses to the wave-cache and tile kernels there
        S, O, B, vol, mats = _case(dev, '3d', C)
        assert not taken(vol, mats['c']) and taken(vol, mats['c'], interp_method='nearest')
        assert taken(vol, mats['c'].clone().requires_grad_())
        with torch.no_grad():
            assert not taken(vol, mats['c'].clone().requires_grad_())
    S, O, B, vol, mats = _case(dev, '2d', 32)
    assert taken(vol, mats['c'])                           # 2-D: no wave-cache kernel
    square = vol[:, :11].contiguous()                      # ('xy' grids need equal leading extents)
    assert taken(square, mats['c']) and not taken(square, mats['c'], indexing='xy')        # cartesian matrices keep the torch form
    S, O, B, vol, mats = _case(dev, '3d', 1)
    assert not taken(vol.to(torch.float64), mats['c'])     # other volume dtypes keep the dense field
    assert taken(vol, mats['c'].to(torch.float64))         # the matrix is cast, as before


def test_deferred_warp_keeps_the_dense_field(dev):
    # SpatialTransformer -> Dice on an affine: the warp is deferred for the fused Dice kernel, which consumes the field
    S, O, B, vol, mats = _case(dev, '3d', 32)
    with deferred.scope(True):
        out = ne.layers.SpatialTransformer()([vol, mats['c']])
        assert isinstance(out, deferred.DeferredWarp)
        assert torch.equal(deferred.materialize(out), _dense_path(vol, mats['c'], O, 'linear', None, True, False))


def _gpu_matrix_grad(vol, M, w, shape, fill, shift_center, single, method='linear'):
    M = M.clone().requires_grad_()
    out = fused.affine_warp(vol, M, shape=shape, interp_method=method, fill_value=fill, shift_center=shift_center, single_transform=single)
    (out * w).sum().backward()
    return M.grad


GRAD_CASES = [('3d', 1), ('3d', 2), ('3d', 3), ('3d', 4), ('3d', 5), ('3d', 32), ('3d_shape', 1), ('3d_shape', 32), ('2d', 1), ('2d', 3),
              ('2d', 4), ('2d', 32), ('2d_shape', 2), ('2d_shape', 3), ('2d_shape', 4), ('2d_shape', 5), ('3d_blocks', 1)]


@pytest.mark.parametrize('name,C', GRAD_CASES)
def test_matrix_gradient_against_float64(dev, name, C):
    S, O, B, vol, mats = _case(dev, name, C)
    D = len(S)
    shape = None if O == S else O
    w = torch.tensor(np.random.default_rng(11).standard_normal((B,) + tuple(O) + (C,)).astype(np.float32), device=dev)
    combos = [('c', None, True, False), ('c', 0.5, True, False), ('c', 0.5, False, True), ('c_square', None, True, True),
              ('identity', None, True, False), ('translation', 0.5, True, False), ('translation', None, False, False),
              ('c_half', None, True, False), ('c_double', 0.5, True, False)]
    for mname, fill, shift_center, single in combos:
        M = mats[mname]
        got = _gpu_matrix_grad(vol, M, w, shape, fill, shift_center, single)
        assert got.shape == M.shape and got.dtype == torch.float32
        nb = 1 if single else B
        shift32 = utils.affine_to_dense_shift(M[:nb], list(O), shift_center=shift_center).cpu().numpy()
        want = AW.matrix_gradient_f64(vol.cpu().numpy(), shift32, w.cpu().numpy(), fill, shift_center, single)
        scale = float(np.abs(want).max())
        assert scale > 0, (mname, fill, shift_center, single)
        g = got.cpu().numpy().astype(np.float64)
        err = float(np.abs(g[:nb, :D] - want).max()) / scale
        print('%s C=%d %s fill=%s centre=%s single=%s: max err / scale = %.3g' % (name, C, mname, fill, shift_center, single, err))
        assert err < TOL, '%s: max err / scale = %.3g' % ((mname, fill, shift_center, single), err)
        assert float(np.abs(g[nb:]).max(initial=0.0)) == 0.0 and float(np.abs(g[:, D:]).max(initial=0.0)) == 0.0


def test_matrix_gradient_where_the_block_count_is_capped(dev):
    # 64 batch entries of 33 x 20 x 17 x 13: 145860 one-channel items per entry ask for 72 blocks, the cap is max(64, 4096 / 64) = 64, so
    # the grid stride is shorter than the items need; with single_transform the second kernel adds 4096 rows
    S, O, B0, _ = AW.SHAPES['3d_blocks']
    AW.assert_recipe_c_crosses_the_border(S, O, 2)
    B, C = 64, 13
    assert -(-(int(np.prod(O)) * C) // 2048) > max(64, 4096 // B)
    vol_np = AW.volume(S, B, C, seed=8)
    w_np = np.random.default_rng(16).standard_normal((B,) + tuple(O) + (C,)).astype(np.float32)
    vol, w = torch.tensor(vol_np, device=dev), torch.tensor(w_np, device=dev)
    M = torch.tensor(np.stack([AW.recipe_c(3, b % 2) for b in range(B)], 0), device=dev)
    for single in (False, True):
        got = _gpu_matrix_grad(vol, M, w, None, 0.5, True, single)
        nb = 1 if single else B
        shift32 = utils.affine_to_dense_shift(M[:nb], list(O), shift_center=True).cpu().numpy()
        want = AW.matrix_gradient_f64(vol_np, shift32, w_np, 0.5, True, single)
        scale = float(np.abs(want).max())
        err = float(np.abs(got.cpu().numpy().astype(np.float64)[:nb] - want).max()) / scale
        print('capped grid, single=%s: max err / scale = %.3g' % (single, err))
        assert scale > 0 and err < TOL, err
        assert torch.equal(got, _gpu_matrix_grad(vol, M, w, None, 0.5, True, single))


def test_nearest_has_a_zero_matrix_gradient(dev):
    for name, C in (('3d', 3), ('2d_shape', 4)):
        S, O, B, vol, mats = _case(dev, name, C)
        w = torch.ones((B,) + tuple(O) + (C,), device=dev)
        for single in (False, True):
            got = _gpu_matrix_grad(vol, mats['c'], w, None if O == S else O, 0.5, True, single, method='nearest')
            assert got.shape == mats['c'].shape and torch.equal(got, torch.zeros_like(got))


@pytest.mark.parametrize('name,C', [('3d_blocks', 1), ('3d', 32), ('2d_shape', 3)])
def test_matrix_gradient_is_deterministic(dev, name, C):
    S, O, B, vol, mats = _case(dev, name, C)
    w = torch.tensor(np.random.default_rng(12).standard_normal((B,) + tuple(O) + (C,)).astype(np.float32), device=dev)
    for single in (False, True):
        a = _gpu_matrix_grad(vol, mats['c'], w, None if O == S else O, 0.5, True, single)
        junk = torch.full((1 << 20,), float('nan'), device=dev)               # the workspace holds no state between calls
        del junk
        b = _gpu_matrix_grad(vol, mats['c'], w, None if O == S else O, 0.5, True, single)
        assert float(a.abs().max()) > 0 and torch.equal(a, b)


@pytest.mark.parametrize('name,C', [('3d', 3), ('3d_shape', 32), ('2d_shape', 4)])
def test_volume_gradient_is_the_dense_field_paths(dev, name, C):
    S, O, B, vol, mats = _case(dev, name, C)
    shape = None if O == S else O
    w = torch.tensor(np.random.default_rng(13).standard_normal((B,) + tuple(O) + (C,)).astype(np.float32), device=dev)
    for method, fill, single in (('linear', None, False), ('linear', 0.5, True), ('nearest', 0.5, False)):
        alone = _gpu_matrix_grad(vol, mats['c'], w, shape, fill, True, single, method=method)
        v = vol.clone().requires_grad_()
        M = mats['c'].clone().requires_grad_()
        out = fused.affine_warp(v, M, shape=shape, interp_method=method, fill_value=fill, single_transform=single)
        (out * w).sum().backward()
        assert torch.equal(M.grad, alone)                                     # unchanged by asking for the volume gradient
        v2 = vol.clone().requires_grad_()
        with deferred.scope(False):
            shift = utils.affine_to_dense_shift(mats['c'][:1 if single else B], list(O), shift_center=True)
            ref = ne.layers.SpatialTransformer(interp_method=method, fill_value=fill, single_transform=single)([v2, shift])
        (ref * w).sum().backward()
        scale = float(v2.grad.abs().max())
        assert scale > 0 and float((v.grad - v2.grad).abs().max()) <= TOL * scale, (method, fill, single)
        # the volume gradient alone
        v3 = vol.clone().requires_grad_()
        (fused.affine_warp(v3, mats['c'], shape=shape, interp_method=method, fill_value=fill, single_transform=single) * w).sum().backward()
        assert float((v3.grad - v2.grad).abs().max()) <= TOL * scale


def test_forward_and_backward_under_graph_replay(dev):
    # as tests/test_gpu_graph_capture.py: the inputs change between replays, and a replay equals the eager call bit for bit
    S, O, B, vol, mats = _case(dev, '3d_shape', 4)
    M = mats['c'].clone()
    w = torch.tensor(np.random.default_rng(14).standard_normal((B,) + tuple(O) + (4,)).astype(np.float32), device=dev)
    vols = [vol.clone(), torch.roll(vol, 2, dims=1).contiguous()]
    Ms = [M.clone(), mats['c_half'].clone()]

    def fn():
        m = M.detach().requires_grad_()
        out = fused.affine_warp(vol, m, shape=O, fill_value=0.5)
        g, = torch.autograd.grad((out * w).sum(), m)
        return out.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                               # workspace growth and lazy allocations: outside the capture
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
    for k in (0, 1, 0):
        vol.copy_(vols[k])
        M.copy_(Ms[k])
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = fn()
        assert float(want[1].abs().max()) > 0
        for a, b in zip(got, want):
            assert torch.equal(a, b), k
