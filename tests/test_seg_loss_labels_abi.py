"""
CPU tests of ne.fused.seg_loss_labels (no kernel is launched): the four entry points of csrc/segloss_labels.hip are declared, typed and
exported and refuse bad arguments, a short workspace and over-limit sizes before any launch; the Python wrapper validates its arguments
on the host and refuses CPU tensors, and so do the loss objects given an integer y_true.
"""

import pytest
import torch

ENTRY_POINTS = ['nrt_seg_loss_labels_supported', 'nrt_seg_loss_labels_workspace_bytes', 'nrt_seg_loss_labels_f32',
                'nrt_seg_loss_labels_bwd_f32']
D = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
BIG = 1 << 40
DICE, CCE, BOTH = 1, 2, 3


def _L():
    from neurite_amd import _lib
    return _lib


def _fwd(labels=D, y_pred=D, lw=None, nvox=100, L=5, batch=2, want=BOTH, ls=0.0, eps=0.0, sums=D, dice=D, minmax=None, cce=D, ws=D,
         nws=BIG):
    return _L().lib().nrt_seg_loss_labels_f32(labels, y_pred, lw, nvox, L, batch, want, ls, eps, sums, dice, minmax, cce, ws, nws, None)


def _bwd(labels=D, y_pred=D, lw=None, sums=D, gdice=D, gcce=D, nvox=100, L=5, batch=2, ls=0.0, eps=0.0, sm=0, grad=D):
    return _L().lib().nrt_seg_loss_labels_bwd_f32(labels, y_pred, lw, sums, gdice, gcce, nvox, L, batch, ls, eps, sm, grad, None)


def _bytes(nvox=100, L=5, batch=2):
    return _L().lib().nrt_seg_loss_labels_workspace_bytes(nvox, L, batch)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
    assert (L.SEG_WANT_DICE, L.SEG_WANT_CCE) == (DICE, CCE)


def test_every_label_count_up_to_256_is_supported():
    lib = _L().lib()
    assert [n for n in range(-2, 300) if lib.nrt_seg_loss_labels_supported(n)] == list(range(1, 257))
    # the one-hot kernels' own rule is untouched
    assert [n for n in range(1, 70) if lib.nrt_seg_loss_supported(n)] == [4, 8, 16, 32, 64]


def test_bad_arguments_are_refused_before_any_launch():
    inv = _L().NRT_ERR_INVALID_ARG
    for kw in ({'labels': None}, {'y_pred': None}, {'sums': None}, {'dice': None}, {'cce': None}, {'nvox': 0}, {'nvox': -5}, {'batch': 0},
               {'batch': -1}, {'L': 0}, {'L': -4}, {'L': 257}, {'want': 0}, {'want': 4}, {'want': -1},
               {'want': DICE, 'cce': None, 'sums': None}, {'want': CCE, 'dice': None, 'cce': None},
               {'want': CCE, 'minmax': D}):                          # the extrema come out of the Dice reduction only
        assert _fwd(**kw) == inv, kw
    for kw in ({'labels': None}, {'y_pred': None}, {'grad': None}, {'gdice': None, 'gcce': None}, {'sums': None}, {'nvox': 0}, {'batch': 0},
               {'L': 0}, {'L': 257}):
        assert _bwd(**kw) == inv, kw
    for kw in ({'L': 0}, {'L': 257}, {'batch': 0}, {'nvox': 0}, {'nvox': -1}):
        assert _bytes(**kw) == 0, kw
    # what a single loss does not produce may be NULL (the call then gets as far as the workspace check)
    ws = _L().NRT_ERR_WORKSPACE
    assert _fwd(want=DICE, cce=None, ws=None, nws=0) == ws and _fwd(want=CCE, sums=None, dice=None, ws=None, nws=0) == ws
    assert _fwd(want=DICE, minmax=D, ws=None, nws=0) == ws and _fwd(L=1, ws=None, nws=0) == ws and _fwd(L=256, lw=D, ws=None, nws=0) == ws


def test_missing_or_short_workspace_is_refused():
    ws = _L().NRT_ERR_WORKSPACE
    need = _bytes()
    assert need >= 2 * 3 * 5 * 4                                        # at least one row of partial sums per batch entry
    assert _fwd(ws=None, nws=0) == ws and _fwd(ws=None, nws=BIG) == ws and _fwd(ws=256, nws=need - 1) == ws and _fwd(ws=256, nws=4) == ws
    assert _bytes(L=10) > need and _bytes(batch=4) > need
    assert _fwd(L=10, ws=256, nws=need) == ws and _fwd(batch=4, ws=256, nws=need) == ws


def test_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    assert _fwd(batch=65536) == unsup and _bwd(batch=65536) == unsup and _bytes(batch=65536) == 0
    # just inside, and beyond 2^31 voxels (64-bit element offsets): refused only for the workspace it was not given
    ws = _L().NRT_ERR_WORKSPACE
    assert _fwd(batch=65535, ws=None, nws=0) == ws and _fwd(nvox=1 << 33, ws=None, nws=0) == ws
    assert _bytes(nvox=1 << 33, L=256, batch=65535) > 0


def test_function_is_public():
    import neurite_amd as ne
    assert 'seg_loss_labels' in ne.fused.__all__ and callable(ne.fused.seg_loss_labels)
    names = ne.fused.seg_loss_labels.__code__.co_varnames[:ne.fused.seg_loss_labels.__code__.co_argcount]
    assert names == ('labels', 'y_pred', 'label_weights', 'label_smoothing', 'laplace_smoothing', 'check_input_limits')
    assert ne.fused.seg_loss_labels.__defaults__ == (None, 0., 0., True)


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    ids, p = torch.zeros(2, 5, 6, 7, dtype=torch.int32), torch.full((2, 5, 6, 7, 4), 0.25)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.seg_loss_labels(ids, p)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.fused.seg_loss_labels(ids.long().unsqueeze(-1), p, label_weights=[1., 2., 3., 4.], label_smoothing=0.1)
    # the loss objects with an integer y_true: the same refusal (it used to be a TypeError / 'same shape' ValueError)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.Dice().loss(ids, p)
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.losses.CategoricalCrossentropy().loss(ids, p)


def test_host_side_argument_errors():
    import neurite_amd as ne
    ids, p = torch.zeros(2, 5, 6, 7, dtype=torch.int32), torch.full((2, 5, 6, 7, 4), 0.25)
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.bool):
        with pytest.raises(TypeError):
            ne.fused.seg_loss_labels(ids.to(dtype), p)
    with pytest.raises(TypeError):
        ne.fused.seg_loss_labels(ids.numpy(), p)
    for shape in ((2, 5, 6), (2, 5, 6, 8), (2, 5, 6, 7, 4), (2, 5, 6, 7, 2), (1, 5, 6, 7), (2, 5, 6, 7, 1, 1)):
        with pytest.raises(ValueError):
            ne.fused.seg_loss_labels(torch.zeros(shape, dtype=torch.int32), p)
    for dtype in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(NotImplementedError):
            ne.fused.seg_loss_labels(ids, p.to(dtype))
    with pytest.raises(NotImplementedError):
        ne.fused.seg_loss_labels(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 257))
    with pytest.raises(ValueError):
        ne.fused.seg_loss_labels(ids, p, label_weights=[1., 2., 3.])
