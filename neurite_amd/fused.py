"""
neurite_amd.fused -- SpatialTransformer + soft Dice in one pass over HBM.

    d = ne.fused.warp_dice(moving, trf, fixed)                # [B, L]
is numerically the pipeline
    warped = ne.layers.SpatialTransformer()([moving, trf]);  d = ne.metrics.Dice(check_input_limits=False).dice(fixed, warped)
(neurite/tf/models.py:806-807 + neurite/tf/metrics.py:415-482) but never writes `warped`: the blended row is
consumed in registers (csrc/fused.hip).  This is the Dice-of-a-warped-segmentation loss/metric of
VoxelMorph-style training; the reference has no fused form (TensorFlow materialises every intermediate).

    d = ne.fused.warp_dice_labels(moving_ids, trf, fixed_ids, nb_labels)      # [B, L]
is the same pipeline on the one-hot maps of two integer label maps, without building them (csrc/warp_labels.hip).

    cce_sum, dice = ne.fused.seg_loss_labels(label_ids, y_pred)               # [1], [B, L]
is the segmentation pair -- weighted CCE sum and soft Dice of one_hot(label_ids, L) and y_pred -- from one pass over y_pred and the
ids (csrc/segloss_labels.hip).

    out = ne.fused.affine_warp(vol, matrix)                                   # [B, *S, C]
is SpatialTransformer on an affine matrix without the dense displacement field, with the matrix gradient (csrc/affine_warp.hip).

    ids = ne.fused.warp_labels(label_ids, trf)                                # [B, X', Y', Z'], the dtype of label_ids
    ids = ne.fused.fuse_labels(atlas_ids, trfs)                               # [X', Y', Z']
warp an integer label map by linear interpolation + arg-max, and fuse several warped atlases by a weighted vote, without a one-hot
tensor and for any label ids (csrc/warp_argmax.hip).
"""

import numpy as np
import torch

from . import _lib
from . import utils
from .errors import InvalidArgumentError

__all__ = ['warp_dice', 'warp_dice_labels', 'seg_loss_labels', 'affine_warp', 'warp_labels', 'fuse_labels']


class _WarpDiceFn(torch.autograd.Function):
    """dice [B, L] as a function of the (already 'ij'-ordered) displacement field; backward in csrc/backward.hip."""

    @staticmethod
    def forward(ctx, shift, run, run_backward):
        ctx.run_backward = run_backward
        return run()

    @staticmethod
    def backward(ctx, grad_dice):
        return ctx.run_backward(grad_dice), None, None


def warp_dice(moving, trf, fixed, indexing='ij', single_transform=False, fill_value=None, laplace_smoothing=0.,
              check_input_limits=False, return_warped=False, return_sums=False, _tune=0):
    """
    moving [B, X, Y, Z, L], trf [B, X', Y', Z', 3] (voxel displacements), fixed [B, X', Y', Z', L]; float32 maps (or both maps
    stored as bfloat16: float32 arithmetic on the widened values, exact for one-hot label maps, half the bytes), 3-D,
    L a multiple of 4 in [4, 256] (4 * 2^k labels run on lane groups of L / 4 lanes, any other count on the next power of two,
    the lanes past L / 4 idle).  Linear interpolation.  Returns dice [B, L] (optionally also the warped
    volume and the partial sums [B, 3, L]).  check_input_limits defaults to False because a tri-linearly
    warped one-hot map exceeds 1.0 by an ulp (see tests); pass True for the reference's asserts (one read-back of the extrema per
    call), or 'deferred' for the same asserts without the host round trip: the values come back as a `checked.CheckedTensor`
    (neurite_amd/checked.py) that raises when they are brought to the host, or at a later call once the extrema have arrived.
    """
    lib = _lib.lib()
    dev = _lib.require_device(moving, trf, fixed)
    if moving.dim() != 5 or fixed.dim() != 5 or trf.dim() != 5 or trf.shape[-1] != 3:
        raise Exception('warp_dice expects 3-D volumes [B, X, Y, Z, L] and a displacement field [B, X, Y, Z, 3]')
    if indexing not in ('ij', 'xy'):
        raise ValueError("indexing has to be 'ij' (matrix) or 'xy' (cartesian)")
    if moving.dtype != fixed.dtype or moving.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError('warp_dice takes two float32 maps, or two bfloat16 maps (bf16 STORAGE, float32 arithmetic: '
                                  'exact for one-hot label maps, half the bytes per row); got %s and %s'
                                  % (moving.dtype, fixed.dtype))
    bf16 = moving.dtype == torch.bfloat16
    if bf16 and return_warped:
        raise NotImplementedError('warp_dice on bfloat16 maps does not return the warped volume (use layers.SpatialTransformer)')
    B, L = moving.shape[0], moving.shape[-1]
    if L % 4 or not 4 <= L <= 256:
        raise NotImplementedError('warp_dice: nb_labels must be a multiple of 4 in [4, 256], got %d (use the unfused layers)' % L)
    if fixed.shape[0] != B or fixed.shape[-1] != L or tuple(fixed.shape[1:-1]) != tuple(trf.shape[1:-1]):
        raise ValueError('fixed must be [B, *trf_spatial, L]')
    if not single_transform and trf.shape[0] != B:
        raise ValueError('batch size of the transform does not match the volume')
    mov = moving.contiguous()
    fix = fixed.contiguous()
    # the kernels read whole 16-byte row pieces: a view whose storage offset is not a multiple of 16 bytes is copied once
    if mov.data_ptr() % 16:
        mov = mov.clone()
    if fix.data_ptr() % 16:
        fix = fix.clone()
    shift = trf.to(torch.float32)
    if indexing == 'xy':
        shift = torch.cat([shift[..., 1:2], shift[..., 0:1], shift[..., 2:]], -1)
    shift = (shift[:1] if single_transform else shift).contiguous()
    S = list(mov.shape[1:-1])
    O = list(fix.shape[1:-1])
    sums = torch.empty((B, 3, L), dtype=torch.float32, device=dev)
    dice = torch.empty((B, L), dtype=torch.float32, device=dev)
    minmax = torch.empty((4,), dtype=torch.float32, device=dev)
    warped = torch.empty_like(fix) if return_warped else None
    if bf16 and torch.is_grad_enabled() and trf.requires_grad:
        raise NotImplementedError('warp_dice on bfloat16 maps has no backward; pass float32 maps for registration training')
    o_shape = _lib.ints(O)
    nws = lib.nrt_warp_dice_workspace_bytes(o_shape, L, B, int(_tune))
    ws = _lib.workspace(dev, nws)
    has_fill = fill_value is not None

    loc_bs = 0 if single_transform else shift[0].numel()

    def run():
        if bf16:
            _lib.call(dev, 'nrt_warp_dice_soft_bf16', _lib.ptr(mov), _lib.ptr(shift), _lib.ptr(fix), _lib.ints(S), o_shape, L, B, loc_bs,
                      _lib.LOC_SHIFT, int(has_fill), float(fill_value) if has_fill else 0.0, float(laplace_smoothing), _lib.ptr(sums),
                      _lib.ptr(dice), _lib.ptr(minmax) if check_input_limits else None, int(_tune), _lib.ptr(ws), nws)
        else:
            _lib.call(dev, 'nrt_warp_dice_soft_f32', _lib.ptr(mov), _lib.ptr(shift), _lib.ptr(fix), _lib.ptr(warped), _lib.ints(S),
                      o_shape, L, B, loc_bs, _lib.LOC_SHIFT, int(has_fill), float(fill_value) if has_fill else 0.0,
                      float(laplace_smoothing), _lib.ptr(sums), _lib.ptr(dice), _lib.ptr(minmax) if check_input_limits else None,
                      int(_tune), _lib.ptr(ws), nws)
        if check_input_limits == 'deferred':
            from . import checked
            return checked.wrap(dice, minmax, 'fused warp + Dice')
        if check_input_limits:
            mn_t, mx_t, mn_p, mx_p = [float(v) for v in minmax.tolist()]
            if not (mn_t >= 0. and mn_p >= 0. and mx_t <= 1. and mx_p <= 1.):
                raise InvalidArgumentError('value outside range')
        return dice

    def run_backward(grad_dice):
        gshift = torch.empty((B,) + tuple(shift.shape[1:]), dtype=torch.float32, device=dev)
        g = grad_dice.to(torch.float32).contiguous()
        _lib.call(dev, 'nrt_warp_dice_bwd_f32', _lib.ptr(mov), _lib.ptr(shift), _lib.ptr(fix), _lib.ptr(sums), _lib.ptr(g),
                  _lib.ptr(gshift), _lib.ints(S), o_shape, L, B, loc_bs, _lib.LOC_SHIFT, int(has_fill), float(laplace_smoothing))
        return gshift.sum(0, keepdim=True) if single_transform else gshift

    if torch.is_grad_enabled() and (moving.requires_grad or fixed.requires_grad):
        raise NotImplementedError('warp_dice: only the transform is differentiable in the fused form; use '
                                  'layers.SpatialTransformer + metrics.Dice for gradients wrt the volumes')
    if torch.is_grad_enabled() and shift.requires_grad:
        if check_input_limits == 'deferred':
            check_input_limits = True                  # (a graph is being recorded: the assert is looked at before the node exists)
        d = _WarpDiceFn.apply(shift, run, run_backward)
    else:
        d = run()
    out = (d,)
    if return_warped:
        out += (warped,)
    if return_sums:
        out += (sums,)
    return out[0] if len(out) == 1 else out


_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _label_map(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(t).__name__)
    if t.dtype not in _INT_DTYPES:
        raise TypeError('warp_dice_labels: %s must hold integer label ids, got %s' % (name, t.dtype))
    if t.dim() == 5 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 4:
        raise Exception('warp_dice_labels expects 3-D label maps [B, X, Y, Z] (or [B, X, Y, Z, 1])')
    return t


def warp_dice_labels(moving, trf, fixed, nb_labels, indexing='ij', single_transform=False, fill_value=None,
                     laplace_smoothing=0., return_warped=False, return_sums=False):
    """
    warp_dice on the one-hot maps of two integer label maps, without building them: moving [B, X, Y, Z] and fixed [B, X', Y', Z']
    (or with a trailing axis of 1) of any torch integer dtype (int32 is used as is, the others are converted once), trf
    [B, X', Y', Z', 3] (voxel displacements), nb_labels = L in [1, 256] (any count).  With M = one_hot(moving, L), F = one_hot(fixed, L)
    in float32 -- an id outside [0, L) gives an all-zero row, as tf.one_hot does -- this returns what
        SpatialTransformer('linear', indexing, single_transform, fill_value)([M, trf]) -> Dice(laplace_smoothing).dice(F, warped)
    returns: dice [B, L], optionally the warped soft labels [B, X', Y', Z', L] (bit-identical to that pipeline's) and the sums
    [B, 3, L] (sum t p, sum t^2, sum p^2; the counts sum t^2 are exact).  The tri-linear warp of a one-hot map has at most 8 non-zero
    values per voxel, so the kernel reads 8 ids per voxel and no rows (csrc/warp_labels.hip).  Differentiable in trf only; with
    single_transform the gradient is summed over the batch.  fill_value: None or 0 (an out-of-bounds voxel then counts as p = 0 for every
    label); any other value raises NotImplementedError.  There is no check_input_limits argument: the inputs are label ids, not
    probabilities, and there is nothing to check.
    Measured on the bench field at 4 x 160^3 x 32 (tools/warp_dice_labels_bench.py, medians): forward 0.478 ms against 0.863 ms for
    warp_dice on prebuilt float32 one-hot maps, forward + backward 0.774 against 2.067.  It loses on i.i.d. label ids, where every wave
    meets every label in every step: forward 1.153 ms against 0.857 (1.34 x; with the backward 1.50 against 2.01), and at 4 labels the
    forward only ties with warp_dice on bfloat16 maps (0.285 against 0.288 ms).
    """
    mov = _label_map(moving, 'moving')
    fix = _label_map(fixed, 'fixed')
    L = int(nb_labels)
    if not 1 <= L <= 256:
        raise NotImplementedError('warp_dice_labels: nb_labels must lie in [1, 256], got %d' % L)
    has_fill = fill_value is not None
    if has_fill and not float(fill_value) == 0.0:
        raise NotImplementedError('warp_dice_labels: fill_value must be None or 0 (a non-zero fill makes every row of a label map dense)')
    dev = _lib.require_device(mov, trf, fix)
    lib = _lib.lib()
    if trf.dim() != 5 or trf.shape[-1] != 3:
        raise Exception('warp_dice_labels expects 3-D label maps [B, X, Y, Z] and a displacement field [B, X, Y, Z, 3]')
    if indexing not in ('ij', 'xy'):
        raise ValueError("indexing has to be 'ij' (matrix) or 'xy' (cartesian)")
    B = mov.shape[0]
    if fix.shape[0] != B or tuple(fix.shape[1:]) != tuple(trf.shape[1:-1]):
        raise ValueError('fixed must be [B, *trf_spatial]')
    if not single_transform and trf.shape[0] != B:
        raise ValueError('batch size of the transform does not match the volume')
    # (an int64 id beyond int32 stays outside [0, L) instead of wrapping into it)
    mov = (mov.clamp(-1, L) if mov.dtype == torch.int64 else mov).to(torch.int32).contiguous()
    fix = (fix.clamp(-1, L) if fix.dtype == torch.int64 else fix).to(torch.int32).contiguous()
    shift = trf.to(torch.float32)
    if indexing == 'xy':
        shift = torch.cat([shift[..., 1:2], shift[..., 0:1], shift[..., 2:]], -1)
    shift = (shift[:1] if single_transform else shift).contiguous()
    S = list(mov.shape[1:])
    O = list(fix.shape[1:])
    sums = torch.empty((B, 3, L), dtype=torch.float32, device=dev)
    dice = torch.empty((B, L), dtype=torch.float32, device=dev)
    warped = torch.empty(tuple(fix.shape) + (L,), dtype=torch.float32, device=dev) if return_warped else None
    o_shape = _lib.ints(O)
    nws = lib.nrt_warp_dice_labels_workspace_bytes(o_shape, L, B)
    ws = _lib.workspace(dev, nws)
    loc_bs = 0 if single_transform else shift[0].numel()

    def run():
        _lib.call(dev, 'nrt_warp_dice_labels_f32', _lib.ptr(mov), _lib.ptr(shift), _lib.ptr(fix), _lib.ptr(warped), _lib.ints(S), o_shape,
                  L, B, loc_bs, _lib.LOC_SHIFT, int(has_fill), 0.0, float(laplace_smoothing), _lib.ptr(sums), _lib.ptr(dice), _lib.ptr(ws),
                  nws)
        return dice

    def run_backward(grad_dice):
        gshift = torch.empty((B,) + tuple(shift.shape[1:]), dtype=torch.float32, device=dev)
        g = grad_dice.to(torch.float32).contiguous()
        _lib.call(dev, 'nrt_warp_dice_labels_bwd_f32', _lib.ptr(mov), _lib.ptr(shift), _lib.ptr(fix), _lib.ptr(sums), _lib.ptr(g),
                  _lib.ptr(gshift), _lib.ints(S), o_shape, L, B, loc_bs, _lib.LOC_SHIFT, int(has_fill), float(laplace_smoothing))
        return gshift.sum(0, keepdim=True) if single_transform else gshift

    if torch.is_grad_enabled() and shift.requires_grad:
        d = _WarpDiceFn.apply(shift, run, run_backward)
    else:
        d = run()
    out = (d,)
    if return_warped:
        out += (warped,)
    if return_sums:
        out += (sums,)
    return out[0] if len(out) == 1 else out


def seg_loss_labels(labels, y_pred, label_weights=None, label_smoothing=0., laplace_smoothing=0., check_input_limits=True):
    """
    The segmentation loss pair on an integer label map as y_true, without its one-hot map: labels [B, *S] (or [B, *S, 1]) of any torch
    integer dtype (int32 is used as is, int64 is clamped to [-1, L] before narrowing, the others are converted once), y_pred [B, *S, L]
    float32, L in [1, 256].  With T = one_hot(labels, L) in float32 -- an id outside [0, L) gives an all-zero row, as tf.one_hot does --
    this returns what metrics._SegLossFn returns on (T, y_pred):
        cce_sum [1]   the SUM over all voxels of the label-weighted categorical cross-entropy of probabilities (metrics.py:619-650:
                      p / sum p, clipped to [1e-7, 1 - 1e-7], label_weights on T, then label_smoothing); divide by the voxel count for
                      Keras' default reduction
        dice [B, L]   soft Dice (metrics.py:415-482) with laplace_smoothing, or divide_no_nan without
    from one pass over y_pred and 4 bytes of id per voxel (csrc/segloss_labels.hip).  Differentiable in y_pred: one pass back, which
    runs through the producer of the soft-max when y_pred still is its untouched output (models.SoftmaxSource), exactly as
    metrics.JointSegLoss does.  check_input_limits looks at y_pred only (one read-back of its extrema): an id cannot leave [0, 1].
    ne.losses.Dice, ne.losses.CategoricalCrossentropy and their pair inside losses.multiple_losses_decorator take the same integer
    y_true and end up here.
    Measured on blob labels at 4 x 160^3 x 32 (tools/seg_loss_labels_bench.py, medians): forward 0.409 ms against 0.699 ms for the pair
    on a prebuilt float32 one-hot map (1.838 with building it on the device), forward + backward 1.371 against 1.966; 33 labels 0.845 /
    2.526 against 2.581 / 8.671 for the two separate one-hot losses; a tie at 4 labels (0.123 against 0.129).
    """
    from . import metrics
    if not isinstance(labels, torch.Tensor) or not isinstance(y_pred, torch.Tensor):
        raise TypeError('seg_loss_labels: expected torch.Tensors, got %s and %s' % (type(labels).__name__, type(y_pred).__name__))
    if labels.dtype not in _INT_DTYPES:
        raise TypeError('seg_loss_labels: labels must hold integer label ids, got %s' % labels.dtype)
    if y_pred.dtype != torch.float32:
        raise NotImplementedError('seg_loss_labels: y_pred must be float32, got %s (the loss objects take other dtypes, on a one-hot map '
                                  'built on the device)' % y_pred.dtype)
    ids = metrics._label_ids(labels, y_pred)                # ValueError on a spatial shape that is not y_pred's
    L = int(y_pred.shape[-1])
    if not 1 <= L <= 256:
        raise NotImplementedError('seg_loss_labels: the number of labels must lie in [1, 256], got %d' % L)
    if y_pred.numel() == 0 or y_pred.shape[0] > 65535:
        raise NotImplementedError('seg_loss_labels: y_pred of shape %s (no voxels, or a batch beyond 65535)' % (tuple(y_pred.shape),))
    w = None
    if label_weights is not None:
        w = label_weights if isinstance(label_weights, torch.Tensor) else torch.as_tensor(np.asarray(label_weights, dtype=np.float32))
        if w.numel() != L:
            raise ValueError(f'Label weights must be of len {L}, but got {w.numel()}.')
    dev = _lib.require_device(ids, y_pred)
    if w is not None:
        w = w.detach().to(dev, torch.float32).reshape(-1).contiguous()
    cfg = (float(laplace_smoothing), float(label_smoothing), bool(check_input_limits))
    cce_sum, dice, _ = metrics._seg_loss_labels(metrics._ids_i32(ids, L), y_pred, w, cfg, _lib.SEG_WANT_DICE | _lib.SEG_WANT_CCE)
    return cce_sum, dice


class _AffineWarpFn(torch.autograd.Function):
    """warp by an affine matrix (csrc/affine_warp.hip).  Backward: the matrix gradient from the same file (no gradient field, no
    atomics); the volume gradient, when asked for, is the warp's own scatter-add (csrc/backward.hip) on the materialised field."""

    @staticmethod
    def forward(ctx, vol, matrix, cfg):
        with torch.no_grad():
            out = _launch_affine_warp(vol, matrix, cfg)
        ctx.save_for_backward(vol, matrix)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, grad_out):
        vol, matrix = ctx.saved_tensors
        cfg = ctx.cfg
        lib = _lib.lib()
        dev = vol.device
        S, O = list(vol.shape[1:-1]), cfg['out_spatial']
        D, B, C, Bm = len(S), vol.shape[0], vol.shape[-1], matrix.shape[0]
        g = grad_out.to(torch.float32).contiguous()
        gvol = gmat = None
        if ctx.needs_input_grad[1]:
            gmat = torch.empty_like(matrix)
            o_shape = _lib.ints(O)
            nws = lib.nrt_affine_warp_workspace_bytes(D, o_shape, C, B)
            ws = _lib.workspace(dev, nws)
            _lib.call(dev, 'nrt_affine_warp_bwd_f32', _lib.ptr(vol), _lib.ptr(matrix), _lib.ptr(g), _lib.ptr(gmat), D, _lib.ints(S),
                      o_shape, C, B, Bm, int(cfg['shift_center']), cfg['method'], int(cfg['fill_value'] is not None), _lib.ptr(ws), nws)
        if ctx.needs_input_grad[0]:
            shift = utils.affine_to_dense_shift(matrix.detach(), O, shift_center=cfg['shift_center'])
            bcfg = dict(out_spatial=O, loc_mode=_lib.LOC_SHIFT, method=cfg['method'], fill_value=cfg['fill_value'], batched=True,
                        single_transform=Bm == 1)
            gvol, _ = utils._launch_interpn_bwd(vol, shift, g, bcfg, True, False)
        return gvol, gmat, None


def _launch_affine_warp(vol, matrix, cfg):
    dev = vol.device
    S, O = list(vol.shape[1:-1]), cfg['out_spatial']
    B, C = vol.shape[0], vol.shape[-1]
    out = torch.empty([B] + O + [C], dtype=torch.float32, device=dev)
    has_fill = cfg['fill_value'] is not None
    _lib.call(dev, 'nrt_affine_warp_f32', _lib.ptr(vol), _lib.ptr(matrix), _lib.ptr(out), len(S), _lib.ints(S), _lib.ints(O), C, B,
              matrix.shape[0], int(cfg['shift_center']), cfg['method'], int(has_fill), float(cfg['fill_value']) if has_fill else 0.0)
    return out


def affine_warp(vol, matrix, shape=None, interp_method='linear', fill_value=None, shift_center=True, single_transform=False):
    """
    SpatialTransformer on an affine matrix in one kernel: out[b, q, :] = interpn(vol[b], A_b [q - c; 1] + c) with c = (shape - 1) / 2
    when shift_center, 'ij' indexing -- bit for bit
        ne.layers.SpatialTransformer(...)([vol, ne.utils.affine_to_dense_shift(matrix, shape, shift_center)])
    without the dense displacement field in between (csrc/affine_warp.hip).  vol [B, *S, C] float32, 2-D or 3-D, any C;
    matrix [B, D, D + 1] or [B, D + 1, D + 1] float32 (single_transform: the first matrix warps the whole batch); shape: the output's
    spatial shape (default S).  Differentiable: the matrix gradient comes from one reduction kernel and a tiny second one (no gradient
    field, no atomics, run-to-run bit-identical; all zeros for 'nearest'), the volume gradient from the warp's own backward.
    layers.SpatialTransformer sends its affine inputs here, except a linear 3-D warp of 32, 64 or 128 channels whose matrix needs no
    gradient and a warp deferred for the fused Dice kernel, which keep the dense field.
    Measured at 4 x 160^3 against that two-kernel path (tools/affine_warp_bench.py, medians): linear forward 0.100 against 0.141 ms at one
    channel, 0.143 / 0.221 at 3, 0.609 / 0.720 at 16, but 1.302 / 0.967 at 32, 2.771 / 2.473 at 64 and 5.941 / 5.149 at 128 (the
    wave-cache and tile kernels win there); forward + matrix gradient 0.380 against 26.2 ms at one channel and 2.769 against 28.4 at 32, where the field came from
    torch ops.
    """
    if not isinstance(vol, torch.Tensor) or not isinstance(matrix, torch.Tensor):
        raise TypeError('affine_warp: expected torch.Tensors, got %s and %s' % (type(vol).__name__, type(matrix).__name__))
    if vol.dtype != torch.float32 or matrix.dtype != torch.float32:
        raise NotImplementedError('affine_warp: the volume and the matrix must be float32, got %s and %s (layers.SpatialTransformer '
                                  'takes other dtypes, on a dense field)' % (vol.dtype, matrix.dtype))
    D = vol.dim() - 2
    if D not in (2, 3):
        raise NotImplementedError('affine_warp: 2-D and 3-D volumes [B, *S, C], got a tensor of rank %d' % vol.dim())
    if interp_method not in utils._METHODS:
        raise ValueError('method should be linear or nearest, got: %s' % interp_method)
    if matrix.dim() != 3 or matrix.shape[-1] != D + 1 or matrix.shape[-2] not in (D, D + 1):
        raise ValueError('affine matrix must be [B, %d, %d] or [B, %d, %d], got %s' % (D, D + 1, D + 1, D + 1, tuple(matrix.shape)))
    B = vol.shape[0]
    if matrix.shape[0] < 1 or (not single_transform and matrix.shape[0] != B):
        raise ValueError('batch size of the transform (%d) does not match the volume (%d)' % (matrix.shape[0], B))
    O = [int(s) for s in (shape if shape is not None else vol.shape[1:-1])]
    if len(O) != D or min(O) < 0:
        raise ValueError('shape must hold %d non-negative extents, got %s' % (D, O))
    if B > 65535:
        raise NotImplementedError('affine_warp: a batch beyond 65535')
    dev = _lib.require_device(vol, matrix)
    m = (matrix[:1] if single_transform else matrix)[:, :D, :].contiguous()
    v = vol.contiguous()
    cfg = dict(out_spatial=O, method=utils._METHODS[interp_method], fill_value=fill_value, shift_center=bool(shift_center))
    if v.numel() == 0:
        raise ValueError('affine_warp: an empty volume %s has nothing to sample' % (tuple(v.shape),))
    if int(np.prod(O)) == 0:
        return torch.zeros([B] + O + [v.shape[-1]], dtype=torch.float32, device=dev)
    if torch.is_grad_enabled() and (v.requires_grad or m.requires_grad):
        return _AffineWarpFn.apply(v, m, cfg)
    return _launch_affine_warp(v, m, cfg)


# ------------------------------------------------------------------------------------------
# warp / resize / fuse integer label maps by linear interpolation + arg-max (csrc/warp_argmax.hip)
# ------------------------------------------------------------------------------------------
_I32_MIN, _I32_MAX = -(1 << 31), (1 << 31) - 1


def _nb_labels_arg(nb_labels, what):
    """nlabels of the C ABI: 0 for nb_labels=None (every int32 value is a label), else L in [1, 2^31 - 1]"""
    if nb_labels is None:
        return 0
    L = int(nb_labels)
    if L != nb_labels or not 1 <= L <= _I32_MAX:
        raise ValueError('%s: nb_labels must be None or an integer in [1, 2^31 - 1], got %r' % (what, nb_labels))
    return L


def _fill_label_arg(fill_label, what):
    """(has_fill, fill_label) of the C ABI"""
    if fill_label is None:
        return 0, 0
    f = int(fill_label)
    if f != fill_label or not _I32_MIN <= f <= _I32_MAX:
        raise ValueError('%s: fill_label must be None or an int32 label id, got %r' % (what, fill_label))
    return 1, f


def _label_ids(t, nd, name, what):
    """an integer label map [B, *S] of nd spatial axes, without its trailing axis of 1 if it has one"""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(t).__name__))
    if t.dtype not in _INT_DTYPES:
        raise TypeError('%s: %s must hold integer label ids, got %s' % (what, name, t.dtype))
    if t.dim() == nd + 2 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != nd + 1:
        raise ValueError('%s: %s must be [B, %s] (or with a trailing axis of 1), got %s'
                         % (what, name, ', '.join('XYZ'[:nd]), tuple(t.shape)))
    if t.numel() == 0:
        raise ValueError('%s: an empty label map %s has nothing to sample' % (what, tuple(t.shape)))
    if int(np.prod(t.shape[1:])) >= 1 << 31:
        raise NotImplementedError('%s: 2^31 or more voxels in a label map' % what)
    return t


def _ids_i32(t, L, what):
    """int32 ids for the kernels.  int64 is clamped to [-1, L] before narrowing where labels are restricted to [0, L) (an id beyond
    int32 stays outside the range instead of wrapping into it); where every value is a label such an id is an error."""
    if t.dtype == torch.int64:
        if L:
            t = t.clamp(-1, L)
        elif int(t.min()) < _I32_MIN or int(t.max()) > _I32_MAX:
            raise ValueError('%s: a label id beyond int32 (ids in [%d, %d]); pass nb_labels to treat it as background'
                             % (what, int(t.min()), int(t.max())))
    return t.to(torch.int32).contiguous()


def _launch_warp_labels(dev, mov, loc, O, L, loc_bs, loc_mode, has_fill, fill, return_prob):
    """mov [B, X, Y, Z] int32 on dev, loc a float32 field or None (LOC_LINSPACE) -> ids [B, *O] int32, prob or None"""
    B = mov.shape[0]
    ids = torch.empty([B] + list(O), dtype=torch.int32, device=dev)
    prob = torch.empty([B] + list(O), dtype=torch.float32, device=dev) if return_prob else None
    _lib.call(dev, 'nrt_warp_labels_argmax_i32', _lib.ptr(mov), _lib.ptr(loc), _lib.ptr(ids), _lib.ptr(prob), _lib.ints(mov.shape[1:]),
              _lib.ints(O), L, B, loc_bs, loc_mode, has_fill, fill)
    return ids, prob


def warp_labels(moving, trf, nb_labels=None, indexing='ij', single_transform=False, fill_label=None, shape=None, shift_center=True,
                return_prob=False):
    """
    Warp an integer label map by linear interpolation + arg-max: with M = one_hot(moving, L) in float32 this returns
        SpatialTransformer('linear', indexing, single_transform, fill_value=0 or None)([M, trf]).argmax(-1)      (seg.pred_to_label)
    and, with return_prob, the winner's value .max(-1), bit for bit, without the one-hot tensor (csrc/warp_argmax.hip): the tri-linear
    blend of a one-hot map has at most 8 non-zero values per voxel, the sums of the weights of the corners that carry each label.  An
    exact tie goes to the smaller id, as np.argmax has it.
    moving [B, X, Y, Z] (or [B, X, Y, Z, 1]) of any torch integer dtype; the ids come back in that dtype, [B, X', Y', Z'].
    trf: a dense displacement field [B, X', Y', Z', 3] in voxels ('xy' indexing swaps its first two components), or an affine
    [B, 3, 4] / [B, 4, 4] ('ij' only), the output's shape given by shape= (default: that of moving) and shift_center as in affine_warp;
    the location is formed in registers, no field is built.  single_transform: the first transform warps the whole batch.
    nb_labels = L: an id outside [0, L) is background (an all-zero row: it never wins; where nothing else has weight the result is 0).
    nb_labels = None: every int32 value is a label, 2035 or -3 alike, at no extra cost; an int64 id beyond int32 raises ValueError.
    fill_label: None clamps the edge; an id: a voxel sampled outside the volume gets that id and prob 0.
    2-D maps [B, X, Y] with a field [B, X', Y', 2] run as 3-D with a leading extent of 1, bit-identical to the 2-D pipeline (the extent-1
    axis has weights exactly 0 and 1); the cost is one small torch.cat of the field.
    Not differentiable (an arg-max has no gradient): nothing returned requires grad.
    Measured at 4 x 160^3 with 32 blob labels under the bench field (tools/warp_labels_bench.py, medians): 0.231 ms against 1.406 ms for
    SpatialTransformer('linear') -> seg.pred_to_label on a prebuilt float32 one-hot map and 2.451 ms with building the map; the same
    0.228 ms on i.i.d. ids and with every id a label; 0.147 ms for an affine matrix.  SpatialTransformer('nearest') on float ids, the
    biased route, takes 0.116 ms.
    """
    what = 'warp_labels'
    if not isinstance(trf, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(trf).__name__))
    if not trf.is_floating_point():
        raise TypeError('%s: the transform must be floating point, got %s' % (what, trf.dtype))
    L = _nb_labels_arg(nb_labels, what)
    has_fill, fill = _fill_label_arg(fill_label, what)
    if indexing not in ('ij', 'xy'):
        raise ValueError("indexing has to be 'ij' (matrix) or 'xy' (cartesian)")
    affine = trf.dim() == 3
    if affine:
        if tuple(trf.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError('%s: an affine transform must be [B, 3, 4] or [B, 4, 4], got %s' % (what, tuple(trf.shape)))
        if indexing != 'ij':
            raise ValueError("%s: 'xy' indexing is supported for dense fields only" % what)
        D = 3
    else:
        D = trf.shape[-1] if trf.dim() > 0 else 0
        if D not in (2, 3) or trf.dim() != D + 2:
            raise ValueError('%s: the transform must be a dense field [B, X, Y, Z, 3] (or [B, X, Y, 2]) or an affine [B, 3, 4], got %s'
                             % (what, tuple(trf.shape)))
        if shape is not None:
            raise ValueError('%s: shape= goes with an affine transform; a dense field has its own' % what)
    mov = _label_ids(moving, D, 'moving', what)
    B = mov.shape[0]
    if trf.shape[0] < 1 or (not single_transform and trf.shape[0] != B):
        raise ValueError('batch size of the transform (%d) does not match the label map (%d)' % (trf.shape[0], B))
    if B > 65535:
        raise NotImplementedError('%s: a batch beyond 65535' % what)
    S = list(mov.shape[1:])
    O = [int(s) for s in shape] if affine and shape is not None else (list(S) if affine else list(trf.shape[1:-1]))
    if len(O) != D or min(O) < 0:
        raise ValueError('%s: shape must hold %d non-negative extents, got %s' % (what, D, O))
    if int(np.prod(O)) >= 1 << 31:
        raise NotImplementedError('%s: 2^31 or more output voxels' % what)
    mov = _ids_i32(mov, L, what)
    dev = _lib.require_device(mov, trf)
    if int(np.prod(O)) == 0:
        ids = torch.zeros([B] + O, dtype=moving.dtype, device=dev)
        return (ids, torch.zeros([B] + O, dtype=torch.float32, device=dev)) if return_prob else ids
    with torch.no_grad():
        if affine:
            m = (trf[:1] if single_transform else trf)[:, :3, :].to(torch.float32).contiguous()
            ids = torch.empty([B] + O, dtype=torch.int32, device=dev)
            prob = torch.empty([B] + O, dtype=torch.float32, device=dev) if return_prob else None
            _lib.call(dev, 'nrt_affine_warp_labels_argmax_i32', _lib.ptr(mov), _lib.ptr(m), _lib.ptr(ids), _lib.ptr(prob), _lib.ints(S),
                      _lib.ints(O), L, B, m.shape[0], int(bool(shift_center)), has_fill, fill)
        else:
            shift = trf.detach().to(torch.float32)
            if indexing == 'xy':
                shift = torch.cat([shift[..., 1:2], shift[..., 0:1], shift[..., 2:]], -1)
            shift = shift[:1] if single_transform else shift
            O3 = O
            if D == 2:                                  # a leading extent of 1 with a zero displacement along it
                shift = torch.cat([torch.zeros_like(shift[..., :1]), shift], -1).unsqueeze(1)
                mov, O3 = mov.unsqueeze(1), [1] + O
            shift = shift.contiguous()
            ids, prob = _launch_warp_labels(dev, mov, shift, O3, L, 0 if single_transform else shift[0].numel(), _lib.LOC_SHIFT,
                                            has_fill, fill, return_prob)
    ids = ids.reshape([B] + O).to(moving.dtype)
    return (ids, prob.reshape([B] + O)) if return_prob else ids


def _resize_labels(ids, zoom_factor, nb_labels, what):
    """resize_labels for a batch [B, *S] (2-D or 3-D) and one zoom factor per spatial axis -> [B, *S'] in the dtype of ids"""
    L = _nb_labels_arg(nb_labels, what)
    D = len(zoom_factor)
    if D not in (2, 3):
        raise NotImplementedError('%s: 2-D and 3-D label maps, got %d zoom factors' % (what, D))
    mov = _label_ids(ids, D, 'ids', what)
    if all(z == 1 for z in zoom_factor):                                        # utils.py:250-251
        return mov
    O = utils._new_shape(list(mov.shape[1:]), list(zoom_factor))
    if min(O) < 0 or int(np.prod(O)) >= 1 << 31:
        raise NotImplementedError('%s: cannot resize %s to %s' % (what, tuple(mov.shape[1:]), O))
    B = mov.shape[0]
    if B > 65535:
        raise NotImplementedError('%s: a batch beyond 65535' % what)
    mov32 = _ids_i32(mov, L, what)
    dev = _lib.require_device(mov32)
    if int(np.prod(O)) == 0:
        return torch.zeros([B] + O, dtype=ids.dtype, device=dev)
    with torch.no_grad():
        out, _ = _launch_warp_labels(dev, mov32.unsqueeze(1) if D == 2 else mov32, None, [1] + O if D == 2 else O, L, 0,
                                     _lib.LOC_LINSPACE, 0, 0, False)
    return out.reshape([B] + O).to(ids.dtype)


def fuse_labels(atlases, trfs, weights=None, nb_labels=None, fill_label=None, return_votes=False):
    """
    Multi-atlas label fusion by a weighted vote: atlases [N, X, Y, Z] (or [N, X, Y, Z, 1]) of any torch integer dtype, 1 <= N <= 16,
    each warped by its own displacement field trfs [N, X', Y', Z', 3] (or all by one field [X', Y', Z', 3] / [1, X', Y', Z', 3]);
    weights: N finite values >= 0 (default: all 1).  With p_n = the tri-linear warp of one_hot(atlases[n]) (warp_labels' p),
        V = sum_n weights[n] * p_n   (float32, in atlas order);   ids = V.argmax(-1)  [X', Y', Z'],   votes = V.max(-1)
    in one kernel without any one-hot tensor (csrc/warp_argmax.hip), exact for every input, 8 N distinct labels at one voxel included.
    Ties go to the smaller id; where no label has a vote the result is 0.  nb_labels as in warp_labels.
    fill_label: None clamps the edge; an id: an atlas sampled outside its volume does not vote, and where none votes the result is
    that id.  Returns the ids in the dtype of atlases, with return_votes also the winner's (not normalised) vote.  Not differentiable.
    A lane's candidate list holds 32 labels; a voxel that meets more (not on anatomical maps) takes a slower, equally exact pass.
    Measured at 160^3 with 32 blob labels (tools/warp_labels_bench.py, medians): 4 atlases 0.659 ms against 1.956 ms for 4 one-hot
    warps added by torch and one arg-max, 16 atlases 4.395 against 8.133.
    """
    what = 'fuse_labels'
    if not isinstance(trfs, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(trfs).__name__))
    if not trfs.is_floating_point():
        raise TypeError('%s: the fields must be floating point, got %s' % (what, trfs.dtype))
    L = _nb_labels_arg(nb_labels, what)
    has_fill, fill = _fill_label_arg(fill_label, what)
    atl = _label_ids(atlases, 3, 'atlases', what)
    N = atl.shape[0]
    if N > 16:
        raise NotImplementedError('%s: at most 16 atlases, got %d' % (what, N))
    if trfs.dim() == 4:
        trfs = trfs.unsqueeze(0)
    if trfs.dim() != 5 or trfs.shape[-1] != 3 or trfs.shape[0] not in (1, N):
        raise ValueError('%s: the fields must be [N, X, Y, Z, 3], or one [X, Y, Z, 3] for every atlas, got %s' % (what, tuple(trfs.shape)))
    O = list(trfs.shape[1:-1])
    if int(np.prod(O)) >= 1 << 31:
        raise NotImplementedError('%s: 2^31 or more output voxels' % what)
    w = None
    if weights is not None:
        w = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float32).reshape(-1)
        if w.size != N or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError('%s: weights must be %d finite values >= 0, got %s' % (what, N, w))
    atl32 = _ids_i32(atl, L, what)
    dev = _lib.require_device(atl32, trfs)
    if int(np.prod(O)) == 0:
        ids = torch.zeros(O, dtype=atlases.dtype, device=dev)
        return (ids, torch.zeros(O, dtype=torch.float32, device=dev)) if return_votes else ids
    with torch.no_grad():
        shift = trfs.detach().to(torch.float32).contiguous()
        wt = torch.from_numpy(w).to(dev) if w is not None else None
        ids = torch.empty(O, dtype=torch.int32, device=dev)
        votes = torch.empty(O, dtype=torch.float32, device=dev) if return_votes else None
        _lib.call(dev, 'nrt_fuse_labels_i32', _lib.ptr(atl32), _lib.ptr(shift), _lib.ptr(wt), _lib.ptr(ids), _lib.ptr(votes),
                  _lib.ints(atl32.shape[1:]), _lib.ints(O), L, N, 0 if shift.shape[0] == 1 else shift[0].numel(), has_fill, fill)
    ids = ids.to(atlases.dtype)
    return (ids, votes) if return_votes else ids
