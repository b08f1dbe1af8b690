"""
CPU tests of the affine warp (no kernel is launched): the three entry points of csrc/affine_warp.hip are declared, typed and exported and
refuse bad arguments before any launch; fused.affine_warp is public and, like SpatialTransformer on an affine input, validates its
arguments on the host and refuses CPU tensors; and the matrices the GPU tests use (tests/affine_warp_cases.py) send between 5 % and
50 % of the output voxels out of bounds on every shape, so that the clamp and the fill arm both run there.
"""

import pytest
import torch

import affine_warp_cases as AW

ENTRY_POINTS = ['nrt_affine_warp_workspace_bytes', 'nrt_affine_warp_f32', 'nrt_affine_warp_bwd_f32']
P = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
BIG = 1 << 40


def _L():
    from neurite_amd import _lib
    return _lib


def _fwd(vol=P, matrix=P, out=P, ndim=3, vol_shape=(5, 6, 7), out_shape=(5, 6, 7), channels=1, batch=2, mbatch=None, shift_center=1,
         method=0, has_fill=0, fill=0.0, vol_shape_null=False, out_shape_null=False):
    L = _L()
    return L.lib().nrt_affine_warp_f32(vol, matrix, out, ndim, None if vol_shape_null else L.ints(vol_shape),
                                       None if out_shape_null else L.ints(out_shape), channels, batch, batch if mbatch is None else mbatch,
                                       shift_center, method, has_fill, fill, None)


def _bwd(vol=P, matrix=P, gout=P, gm=P, ndim=3, vol_shape=(5, 6, 7), out_shape=(5, 6, 7), channels=1, batch=2, mbatch=None, shift_center=1,
         method=0, has_fill=0, ws=P, nws=BIG, vol_shape_null=False, out_shape_null=False):
    L = _L()
    return L.lib().nrt_affine_warp_bwd_f32(vol, matrix, gout, gm, ndim, None if vol_shape_null else L.ints(vol_shape),
                                           None if out_shape_null else L.ints(out_shape), channels, batch,
                                           batch if mbatch is None else mbatch, shift_center, method, has_fill, ws, nws, None)


def _bytes(ndim=3, out_shape=(5, 6, 7), channels=1, batch=2):
    L = _L()
    return L.lib().nrt_affine_warp_workspace_bytes(ndim, L.ints(out_shape), channels, batch)


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
    common = ({'vol': None}, {'matrix': None}, {'vol_shape_null': True}, {'out_shape_null': True}, {'batch': 0}, {'batch': -1},
              {'channels': 0}, {'channels': -4}, {'vol_shape': (5, 0, 7)}, {'vol_shape': (-5, 6, 7)}, {'out_shape': (5, 6, 0)},
              {'out_shape': (5, -6, 7)}, {'ndim': 2, 'vol_shape': (0, 6), 'out_shape': (5, 6)}, {'mbatch': 3}, {'mbatch': 0},
              {'method': 2}, {'method': -1})
    for kw in common + ({'out': None},):
        assert _fwd(**kw) == inv, kw
    for kw in common + ({'gout': None}, {'gm': None}):
        assert _bwd(**kw) == inv, kw
    for kw in ({'batch': 0}, {'channels': 0}, {'out_shape': (0, 6, 7)}, {'out_shape': (5, 6, -7)}):
        assert _bytes(**kw) == 0, kw


def test_ranks_and_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    for kw in ({'ndim': 1}, {'ndim': 4}, {'ndim': 0}, {'batch': 65536},
               {'batch': 1, 'out_shape': (1 << 10, 1 << 10, 1 << 11)},                                 # 2^31 output voxels
               {'batch': 2, 'out_shape': (1 << 10, 1 << 10, 1 << 10)},
               {'batch': 1, 'out_shape': (1 << 10, 1 << 10, 1 << 9), 'channels': 4},                  # 2^31 elements
               {'batch': 1, 'vol_shape': (1 << 10, 1 << 10, 1 << 11)},                                 # the volume counts too
               {'batch': 1, 'vol_shape': (1 << 30, 1 << 30, 1 << 30)},
               {'batch': 1, 'ndim': 2, 'vol_shape': (1 << 16, 1 << 15), 'out_shape': (4, 4)}):
        assert _fwd(**kw) == unsup, kw
        assert _bwd(**kw) == unsup, kw
    for kw in ({'ndim': 1}, {'ndim': 4}, {'batch': 65536}, {'batch': 1, 'out_shape': (1 << 10, 1 << 10, 1 << 11)},
               {'batch': 2, 'out_shape': (1 << 10, 1 << 10, 1 << 9), 'channels': 2}):
        assert _bytes(**kw) == 0, kw
    # just inside: 2^31 - 2^21 elements, the largest batch
    assert _bytes(batch=1, out_shape=(1 << 10, 1 << 10, (1 << 11) - 2)) > 0
    assert _bytes(batch=65535, out_shape=(2, 2, 2), channels=3) > 0
    assert _bytes(ndim=2, batch=1, out_shape=(1 << 15, (1 << 16) - 1, 99)) > 0                                 # (the third extent is not read)


def test_missing_or_short_workspace_is_refused():
    ws = _L().NRT_ERR_WORKSPACE
    need = _bytes()
    assert need >= 2 * 12 * 4                                           # one row of D (D + 1) floats per batch entry at the least
    assert _bwd(ws=None, nws=0) == ws and _bwd(ws=None, nws=BIG) == ws and _bwd(ws=256, nws=need - 1) == ws
    assert _bwd(ws=256, nws=0, method=1) == ws                          # nearest writes zeros, after the same checks
    assert _bytes(ndim=2, out_shape=(13, 11), channels=3) >= 2 * 6 * 4
    assert _bwd(ndim=2, vol_shape=(13, 11), out_shape=(13, 11), channels=3, ws=256, nws=_bytes(ndim=2, out_shape=(13, 11), channels=3) - 1) == ws
    # a pure function of the shapes, growing with the voxels
    assert _bytes() == need and _bytes(out_shape=(160, 160, 160)) > need


def test_affine_warp_is_public():
    import neurite_amd as ne
    assert 'affine_warp' in ne.fused.__all__ and callable(ne.fused.affine_warp)


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    vol, M = torch.rand(2, 5, 6, 7, 1), torch.eye(3, 4).repeat(2, 1, 1)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.affine_warp(vol, M)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.affine_warp(vol[:, 0], torch.eye(3).repeat(2, 1, 1), shape=(4, 4), interp_method='nearest', fill_value=0.0)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.layers.SpatialTransformer()([vol, M])
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.layers.SpatialTransformer(single_transform=True, fill_value=0.0)([vol, torch.eye(4).repeat(2, 1, 1).requires_grad_()])


def test_host_side_argument_errors():
    import neurite_amd as ne
    aw = ne.fused.affine_warp
    vol, M = torch.rand(2, 5, 6, 7, 1), torch.eye(3, 4).repeat(2, 1, 1)
    for dtype in (torch.float64, torch.bfloat16, torch.float16, torch.int32):
        with pytest.raises(NotImplementedError):                        # before any launch, whatever the device
            aw(vol.to(dtype), M)
        with pytest.raises(NotImplementedError):
            aw(vol, M.to(dtype))
    with pytest.raises(TypeError):
        aw(vol.numpy(), M)
    for bad in (torch.rand(2, 5, 1), torch.rand(2, 3, 4, 5, 6, 1)):     # 1-D and 4-D volumes
        with pytest.raises(NotImplementedError):
            aw(bad, M)
    for bad in (torch.eye(3, 4), torch.rand(2, 4, 3), torch.rand(2, 2, 3), torch.rand(2, 3, 5), torch.rand(2, 1, 3, 4),
                torch.rand(3, 3, 4), torch.rand(0, 3, 4)):
        with pytest.raises(ValueError):
            aw(vol, bad)
    with pytest.raises(ValueError):
        aw(vol, M[:1])                                                  # one matrix for two volumes needs single_transform
    with pytest.raises(ValueError):
        aw(vol, M, shape=(5, 6))
    with pytest.raises(ValueError):
        aw(vol, M, interp_method='cubic')
    # accepted on the host: what is left is the device check
    with pytest.raises(_L().NeuriteAmdError, match='no CPU fallback'):
        aw(vol, M[:1], single_transform=True)


@pytest.mark.parametrize('name', list(AW.SHAPES))
def test_recipe_c_sends_5_to_50_percent_out_of_bounds(name):
    S, O, B, _ = AW.SHAPES[name]
    AW.assert_recipe_c_crosses_the_border(S, O, B)
    mats = AW.matrices(len(S), B)
    assert set(mats) == {'identity', 'translation', 'c', 'c_half', 'c_double', 'c_square'}
    assert mats['c_square'].shape == (B, len(S) + 1, len(S) + 1) and AW.oob_fraction(mats['identity'][0], S, S) == 0.0
