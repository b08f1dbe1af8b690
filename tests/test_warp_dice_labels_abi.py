"""
CPU tests of ne.fused.warp_dice_labels (no kernel is launched): the three entry points of csrc/warp_labels.hip are declared, typed and
exported and refuse bad arguments, a short workspace and over-limit sizes before any launch; the Python wrapper validates its arguments
on the host and refuses CPU tensors.
"""

import pytest
import torch

ENTRY_POINTS = ['nrt_warp_dice_labels_workspace_bytes', 'nrt_warp_dice_labels_f32', 'nrt_warp_dice_labels_bwd_f32']
D = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
BIG = 1 << 40
SHIFT, ABSOLUTE, LINSPACE = 1, 0, 2


def _L():
    from neurite_amd import _lib
    return _lib


def _fwd(moving=D, loc=D, fixed=D, warped=None, vol=(5, 6, 7), out=(4, 5, 6), L=5, batch=2, loc_bs=360, mode=SHIFT, has_fill=0, fill=0.0,
         eps=0.0, sums=D, dice=D, ws=D, nws=BIG, vol_null=False, out_null=False):
    lib = _L()
    return lib.lib().nrt_warp_dice_labels_f32(moving, loc, fixed, warped, None if vol_null else lib.ints(vol), None if out_null else lib.ints(out),
                                              L, batch, loc_bs, mode, has_fill, fill, eps, sums, dice, ws, nws, None)


def _bwd(moving=D, loc=D, fixed=D, sums=D, gdice=D, gloc=D, vol=(5, 6, 7), out=(4, 5, 6), L=5, batch=2, loc_bs=360, mode=SHIFT, has_fill=0,
         eps=0.0, vol_null=False, out_null=False):
    lib = _L()
    return lib.lib().nrt_warp_dice_labels_bwd_f32(moving, loc, fixed, sums, gdice, gloc, None if vol_null else lib.ints(vol),
                                                  None if out_null else lib.ints(out), L, batch, loc_bs, mode, has_fill, eps, None)


def _bytes(out=(4, 5, 6), L=5, batch=2):
    lib = _L()
    return lib.lib().nrt_warp_dice_labels_workspace_bytes(lib.ints(out), L, batch)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_bad_arguments_are_refused_before_any_launch():
    inv = _L().NRT_ERR_INVALID_ARG
    for kw in ({'moving': None}, {'loc': None}, {'fixed': None}, {'sums': None}, {'dice': None}, {'vol_null': True}, {'out_null': True},
               {'L': 0}, {'L': -4}, {'L': 257}, {'batch': 0}, {'batch': -1}, {'vol': (5, 0, 7)}, {'out': (4, -5, 6)}, {'out': (4, 0, 6)},
               {'has_fill': 1, 'fill': 1.0}, {'has_fill': 1, 'fill': -0.5}, {'has_fill': 1, 'fill': float('nan')},
               {'mode': LINSPACE}, {'mode': LINSPACE, 'loc': None}, {'mode': 3}, {'mode': -1}, {'loc_bs': -1}):
        assert _fwd(**kw) == inv, kw
    for kw in ({'moving': None}, {'loc': None}, {'fixed': None}, {'sums': None}, {'gdice': None}, {'gloc': None}, {'vol_null': True},
               {'out_null': True}, {'L': 0}, {'L': 257}, {'batch': 0}, {'vol': (5, 6, 0)}, {'out': (-4, 5, 6)}, {'mode': LINSPACE}, {'mode': 3}):
        assert _bwd(**kw) == inv, kw
    for kw in ({'L': 0}, {'L': 257}, {'batch': 0}, {'out': (4, 0, 6)}, {'out': (4, 5, -6)}):
        assert _bytes(**kw) == 0, kw
    # a zero fill is the supported one (the call then gets as far as the workspace check); so is fill_value without has_fill
    ws = _L().NRT_ERR_WORKSPACE
    assert _fwd(has_fill=1, fill=0.0, ws=None, nws=0) == ws and _fwd(has_fill=1, fill=-0.0, ws=None, nws=0) == ws
    assert _fwd(has_fill=0, fill=3.0, ws=None, nws=0) == ws
    assert _fwd(mode=ABSOLUTE, loc_bs=0, L=1, ws=None, nws=0) == ws and _fwd(L=256, warped=D, ws=None, nws=0) == ws


def test_missing_or_short_workspace_is_refused():
    ws = _L().NRT_ERR_WORKSPACE
    need = _bytes()
    assert need >= 2 * 3 * 5 * 4                                        # at least one row of partial sums per batch entry
    assert _fwd(ws=None, nws=0) == ws and _fwd(ws=None, nws=BIG) == ws and _fwd(ws=256, nws=need - 1) == ws and _fwd(ws=256, nws=4) == ws
    # the need grows with the labels, the batch and (up to the block cap) the output
    assert _bytes(L=10) > need and _bytes(batch=4) > need and _bytes(out=(40, 50, 60)) > need
    assert _bytes(out=(400, 500, 600)) == _bytes(out=(800, 500, 600))
    assert _fwd(out=(40, 50, 60), loc_bs=360000, ws=256, nws=need) == ws


def test_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    for kw in ({'vol': (1 << 10, 1 << 10, 1 << 11)},                    # 2^31 voxels in the volume
               {'vol': (1 << 20, 1 << 20, 1 << 20)},
               {'out': (1 << 10, 1 << 10, 1 << 11)},                    # 2^31 output voxels
               {'out': (1 << 20, 1 << 20, 1 << 20)},
               {'batch': 65536}):
        assert _fwd(**kw) == unsup, kw
        assert _bwd(**kw) == unsup, kw
    assert _bytes(out=(1 << 10, 1 << 10, 1 << 11)) == 0 and _bytes(batch=65536) == 0
    # the warped output: one batch entry below 4 GiB, as nrt_warp_dice_soft_f32 limits it
    assert _fwd(out=(1 << 10, 1 << 10, 1 << 5), L=32, warped=D) == unsup
    # just inside (refused only for the workspace it was not given)
    ws = _L().NRT_ERR_WORKSPACE
    assert _fwd(vol=(1 << 10, 1 << 10, (1 << 11) - 1), ws=None, nws=0) == ws
    assert _fwd(out=(1 << 10, 1 << 10, (1 << 11) - 1), batch=65535, ws=None, nws=0) == ws
    assert _fwd(out=(1 << 10, 1 << 10, 1 << 5), L=32, ws=None, nws=0) == ws
    assert _fwd(out=(1 << 10, 1 << 10, (1 << 5) - 1), L=32, warped=D, ws=None, nws=0) == ws
    assert _bytes(out=(1 << 10, 1 << 10, (1 << 11) - 1), L=256, batch=65535) > 0


def test_function_is_public():
    import neurite_amd as ne
    assert 'warp_dice_labels' in ne.fused.__all__ and callable(ne.fused.warp_dice_labels)
    assert 'check_input_limits' not in ne.fused.warp_dice_labels.__code__.co_varnames
    assert 'nothing to check' in ne.fused.warp_dice_labels.__doc__


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    m, f, t = torch.zeros(2, 5, 6, 7, dtype=torch.int32), torch.zeros(2, 5, 6, 7, dtype=torch.int64), torch.zeros(2, 5, 6, 7, 3)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.warp_dice_labels(m, t, f, 4)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.warp_dice_labels(m.unsqueeze(-1), t, f.unsqueeze(-1), 4, fill_value=0, return_warped=True)


def test_host_side_argument_errors():
    import neurite_amd as ne
    t = torch.zeros(2, 5, 6, 7, 3)
    ids = torch.zeros(2, 5, 6, 7, dtype=torch.int32)
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.bool):
        with pytest.raises(TypeError):
            ne.fused.warp_dice_labels(ids.to(dtype), t, ids, 4)
        with pytest.raises(TypeError):
            ne.fused.warp_dice_labels(ids, t, ids.to(dtype), 4)
    with pytest.raises(TypeError):
        ne.fused.warp_dice_labels(ids.numpy(), t, ids, 4)
    for fill in (1.0, -1, 0.5, float('nan')):
        with pytest.raises(NotImplementedError):
            ne.fused.warp_dice_labels(ids, t, ids, 4, fill_value=fill)
    for nb in (0, 257, -1):
        with pytest.raises(NotImplementedError):
            ne.fused.warp_dice_labels(ids, t, ids, nb)
