"""
neurite_amd.utils -- the tensor utilities of neurite's hot path on MI355X.

Mirrors the names, arguments, defaults and error behaviour of neurite/tf/utils/utils.py for
interpn (:73), resize/zoom (:223,:265), volshape_to_ndgrid (:333), volshape_to_meshgrid (:356),
ndgrid (:382), meshgrid (:398), sub2ind2d (:1068), prod_n (:1085), batch_channel_flatten (:1175),
flatten_axes (:1195), barycenter (:512); plus voxelmorph's transform()/affine_to_dense_shift, which the reference
calls but does not vendor (neurite/tf/models.py:806-807, 1157-1159), and voxelmorph's jacobian_determinant (restated: DESIGN 4.6i) and its
dist_trf / signed_dist_trf / vol_to_sdt family (restated: DESIGN 4.6j); and connected components with the mask clean-up built on them
(scipy.ndimage.label / binary_fill_holes on the device: DESIGN 4.6k); and exact percentiles with the percentile intensity normalisation
(np.percentile on the device, by a radix select: DESIGN 4.6l); and per-label region statistics of an integer id map (scipy.ndimage.sum /
center_of_mass / find_objects on the device: DESIGN 4.6n); and binary morphology, box minimum / maximum filters and box rank filters
(scipy.ndimage.binary_erosion ... median_filter on the device: DESIGN 4.6o; the code is in neurite_amd/morphology.py).

Tensors are torch tensors on a ROCm device in the reference's channels-last layout.  All sampling
work is done by the HIP kernels in csrc/interpn.hip through the C ABI; nothing here falls back
to PyTorch or the CPU.
"""

import ctypes as C

import numpy as np
import torch

from . import _lib
from .deferred import materialize
from .morphology import (binary_closing, binary_dilation, binary_erosion, binary_opening, grey_closing, grey_dilation,   # noqa: F401
                         grey_erosion, grey_opening, maximum_filter, median_filter, minimum_filter, percentile_filter, rank_filter)

__all__ = ['interpn', 'resize', 'zoom', 'resize_labels', 'zoom_labels', 'transform', 'affine_to_dense_shift', 'integrate_vec', 'compose',
           'gaussian_kernel', 'separable_conv', 'minmax_norm', 'soft_quantize', 'barycenter', 'jacobian_determinant',
           'dist_trf', 'signed_dist_trf', 'vol_to_sdt', 'vol_to_sdt_batch', 'label_dist_trf',
           'connected_components', 'largest_component', 'keep_largest_components', 'remove_small_components', 'fill_holes',
           'percentile', 'quantile', 'median', 'percentile_norm', 'label_stats', 'label_volumes', 'label_centroids',
           'binary_erosion', 'binary_dilation', 'binary_opening', 'binary_closing', 'minimum_filter', 'maximum_filter', 'grey_erosion',
           'grey_dilation', 'grey_opening', 'grey_closing', 'median_filter', 'rank_filter', 'percentile_filter',
           'rescale_dense_transform', 'rescale_affine', 'is_affine_shape', 'validate_affine_shape', 'make_square_affine', 'volshape_to_ndgrid',
           'volshape_to_meshgrid', 'ndgrid', 'meshgrid', 'sub2ind2d', 'prod_n', 'batch_channel_flatten',
           'flatten_batch_channel', 'flatten_axes']

_METHODS = {'linear': _lib.INTERP_LINEAR, 'nearest': _lib.INTERP_NEAREST}
_SMALL_INTS = (torch.int8, torch.uint8, torch.int16, torch.bool)


class _NoBackward(torch.autograd.Function):
    """Forward-only ops: reaching backward is an error, never a silent zero gradient."""

    @staticmethod
    def forward(ctx, fn, *tensors):
        with torch.no_grad():
            return fn()

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError('neurite_amd: backward of the HIP hot-path ops is not implemented yet '
                                  '(forward-only build; see DESIGN.md "what comes next").')


def _maybe_tracked(fn, *tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        return _NoBackward.apply(fn, *[t for t in tensors if isinstance(t, torch.Tensor)])
    return fn()


class _InterpnFn(torch.autograd.Function):
    """
    interpn (float32, 1-3-D) with the hand-written backward of csrc/backward.hip: gradients wrt the volume (scatter-add)
    and, for linear interpolation, wrt the sampling locations / displacement field (what TF's autodiff derives from
    utils.py:137-213); nearest interpolation passes no gradient to the locations (tf.round).
    """

    @staticmethod
    def forward(ctx, vol, loc, cfg):
        vol = vol.contiguous()
        loc = None if loc is None else loc.contiguous()
        with torch.no_grad():
            out = _launch_interpn(vol, loc, **cfg)
        ctx.save_for_backward(vol, loc)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, grad_out):
        vol, loc = ctx.saved_tensors
        need_vol = ctx.needs_input_grad[0]
        need_loc = loc is not None and ctx.needs_input_grad[1]
        gvol, gloc = _launch_interpn_bwd(vol, loc, grad_out, ctx.cfg, need_vol, need_loc)
        return gvol, gloc, None


def _launch_interpn_bwd(vol, loc, grad_out, cfg, need_vol, need_loc):
    dev = _lib.require_device(vol, loc, grad_out)
    batched, single = cfg['batched'], cfg.get('single_transform', False)
    B = vol.shape[0] if batched else 1
    S = list(vol.shape[1:-1]) if batched else list(vol.shape[:-1])
    Cc, D = vol.shape[-1], len(S)
    out_spatial = [int(s) for s in cfg['out_spatial']]
    abi_spatial = out_spatial if len(out_spatial) == D else [int(np.prod(out_spatial))] + [1] * (D - 1)     # see _launch_interpn
    g = grad_out.to(torch.float32).contiguous()
    if cfg['method'] == _lib.INTERP_NEAREST:
        # utils.py:193-204: tf.round has no gradient (TF returns None for loc; zeros here so that optimisers see a tensor),
        # the volume receives tf.gather's scatter-add
        gvol = torch.zeros_like(vol) if need_vol else None
        gloc = torch.zeros_like(loc) if (need_loc and loc is not None) else None
        if gvol is not None and g.numel():
            nvol = int(np.prod(S)) * Cc
            nloc = int(np.prod(out_spatial)) * D
            loc_bs = 0 if (single or loc is None) else nloc
            _lib.call(dev, 'nrt_interpn_nearest_bwd_f32', _lib.ptr(loc), _lib.ptr(g), _lib.ptr(gvol), D, _lib.ints(S),
                      _lib.ints(abi_spatial), Cc, B, nvol, loc_bs, cfg['loc_mode'], int(cfg['fill_value'] is not None))
        return gvol, gloc
    gvol = torch.zeros_like(vol) if need_vol else None
    gloc = None
    if need_loc:
        gloc = torch.empty(([B] if batched else []) + out_spatial + [D], dtype=torch.float32, device=dev)
    if g.numel() == 0 or not (need_vol or need_loc):
        if gloc is not None:
            gloc.zero_()
    else:
        nvol = int(np.prod(S)) * Cc
        nloc = int(np.prod(out_spatial)) * D
        loc_bs = 0 if (single or loc is None) else nloc
        _lib.call(dev, 'nrt_interpn_bwd_f32', _lib.ptr(vol), _lib.ptr(loc), _lib.ptr(g), _lib.ptr(gvol), _lib.ptr(gloc), D, _lib.ints(S),
                  _lib.ints(abi_spatial), Cc, B, nvol, loc_bs, cfg['loc_mode'], int(cfg['fill_value'] is not None))
    if gloc is not None and single and batched:
        gloc = gloc.sum(0, keepdim=True)       # one transform shared by the whole batch
    return gvol, gloc


def _interp_op(vol, loc, out_spatial, loc_mode, method, fill_value, batched, single_transform=False,
               variant=0, tune=0):
    """Forward launch, recorded for autograd when an input requires grad (linear float32, 1-3-D only)."""
    cfg = dict(out_spatial=[int(s) for s in out_spatial], loc_mode=loc_mode, method=method, fill_value=fill_value,
               batched=batched, single_transform=single_transform, variant=variant, tune=tune)
    needs = torch.is_grad_enabled() and (vol.requires_grad or (loc is not None and loc.requires_grad))
    if not needs:
        return _launch_interpn(vol, loc, **cfg)
    vol_rank = vol.dim() - (2 if batched else 1)                        # the backward kernels take 1- to 3-D volumes
    if vol.dtype == torch.float32 and vol_rank <= 3:
        return _InterpnFn.apply(vol, loc, cfg)
    return _NoBackward.apply(lambda: _launch_interpn(vol, loc, **cfg), vol, *([] if loc is None else [loc]))


def _launch_interpn(vol, loc, out_spatial, loc_mode, method, fill_value, batched, single_transform=False,
                    variant=0, tune=0):
    """
    vol [B?, *S, C] contiguous; loc [B?, *S', D] float32 contiguous or None (LINSPACE).
    Returns out [B?, *S', C] with vol's dtype.
    """
    dev = _lib.require_device(vol, loc)
    vol = vol.contiguous()
    if batched:
        B = vol.shape[0]
        S = list(vol.shape[1:-1])
    else:
        B = 1
        S = list(vol.shape[:-1])
    Cc = vol.shape[-1]
    D = len(S)
    if D < 1 or D > _ANY_MAXD:
        raise NotImplementedError('neurite_amd.interpn supports 1- to %d-D volumes, got %d-D (2^D corner rows per output; '
                                  'the reference, neurite/tf/utils/utils.py:159, has no rank limit)' % (_ANY_MAXD, D))
    out_spatial = [int(s) for s in out_spatial]
    out_shape = ([B] if batched else []) + out_spatial + [Cc]
    out = torch.empty(out_shape, dtype=vol.dtype, device=dev)
    if out.numel() == 0:
        return out
    nvol = int(np.prod(S)) * Cc
    nloc = int(np.prod(out_spatial)) * D
    # the C ABI takes exactly D output extents.  The reference accepts location tensors of any leading rank (e.g. [N, D] sample
    # points for a 3-D volume): flatten them to [N, 1, ...]; the output is contiguous, so the shape above already is its final one
    if len(out_spatial) != D:
        if loc_mode == _lib.LOC_LINSPACE:
            raise ValueError('resize needs one output extent per volume dimension')
        out_spatial = [int(np.prod(out_spatial))] + [1] * (D - 1)
    if loc is not None:
        loc = loc.contiguous()
    vol_bs = nvol
    loc_bs = 0 if (single_transform or loc is None) else nloc
    has_fill = fill_value is not None
    if vol.dtype in _ANY_DTYPES and (D > 3 or vol.dtype not in (torch.float32, torch.int32)):
        # float16 / bfloat16 / float64 volumes, and ranks 4-8: the dtype- and rank-generic kernel (csrc/interpn_any.hip);
        # arithmetic in the volume dtype, one rounding per op, as TensorFlow evaluates utils.py:137-213
        if vol.dtype == torch.int32:
            assert method == _lib.INTERP_NEAREST
        loc64 = loc is not None and loc.dtype == torch.float64
        assert not loc64 or (vol.dtype == torch.float64 and loc_mode == _lib.LOC_ABSOLUTE)
        _lib.call(dev, 'nrt_interpn_any', _lib.ptr(vol), _lib.ptr(loc), _lib.ptr(out), _ANY_DTYPES[vol.dtype], D, _lib.ints(S),
                  _lib.ints(out_spatial), Cc, B, vol_bs, loc_bs, loc_mode, int(loc64), method, int(has_fill),
                  float(fill_value) if has_fill else 0.0)
    elif vol.dtype == torch.float32:
        _lib.call(dev, 'nrt_interpn_f32_ex', _lib.ptr(vol), _lib.ptr(loc), _lib.ptr(out), D, _lib.ints(S), _lib.ints(out_spatial), Cc, B,
                  vol_bs, loc_bs, loc_mode, method, int(has_fill), float(fill_value) if has_fill else 0.0, int(variant), int(tune))
    elif vol.dtype == torch.int32:
        assert method == _lib.INTERP_NEAREST
        _lib.call(dev, 'nrt_interpn_nearest_i32', _lib.ptr(vol), _lib.ptr(loc), _lib.ptr(out), D, _lib.ints(S), _lib.ints(out_spatial),
                  Cc, B, vol_bs, loc_bs, loc_mode, int(has_fill), int(fill_value) if has_fill else 0)
    else:
        raise NotImplementedError('unsupported volume dtype %s' % vol.dtype)
    return out


_ANY_MAXD = 8
_ANY_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16,
               torch.float64: _lib.DT_F64, torch.int32: _lib.DT_I32}


def _loc_for(vol, loc):
    """`loc` as the kernels take it.  The reference casts loc to the volume's dtype when both are floating (utils.py:123-127)
    and integer locations to float32 (:124-125).  The kernels read float32 locations and round them to the volume dtype
    themselves (float16 / bfloat16: RNE, the same rounding as tf.cast; values that already are of the narrow type survive the
    float32 detour unchanged); only a float64 volume reads float64 locations."""
    if not loc.dtype.is_floating_point:
        return loc.to(torch.float32)
    if vol.dtype == torch.float64:
        return loc.to(torch.float64)
    if vol.dtype in (torch.float16, torch.bfloat16):
        return loc.to(vol.dtype).to(torch.float32) if loc.dtype == torch.float64 else loc.to(torch.float32)
    return loc.to(torch.float32)


def _prepare_vol(vol, interp_method):
    """dtype policy of the HIP path.  Returns (vol as the kernels take it, restore_dtype)."""
    if vol.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        return vol, None
    # integer volumes
    if interp_method == 'linear':
        # the reference multiplies float weights with the gathered values (utils.py:191): TF raises
        raise TypeError('linear interpolation of an integer volume (%s) is a dtype error in the reference; '
                        'cast the volume to float32 first' % vol.dtype)
    if vol.dtype == torch.int32:
        return vol, None
    if vol.dtype in _SMALL_INTS:
        return vol.to(torch.int32), vol.dtype
    raise NotImplementedError('nearest interpolation of %s volumes is not implemented' % vol.dtype)


def interpn(vol, loc, interp_method='linear', fill_value=None, *, _variant=0, _tune=0):
    """
    N-D gridded interpolation (neurite/tf/utils/utils.py:73-220).

    vol: [*vol_shape] or [*vol_shape, C];  loc: list of D tensors or a [*new_shape, D] tensor;
    interp_method 'linear' | 'nearest'; fill_value: value outside the domain (None = edge clamp).
    Returns a tensor shaped like the entries of loc (+ channel axis if vol had one).
    """
    if isinstance(loc, (list, tuple)):
        loc = torch.stack([torch.as_tensor(l) for l in loc], -1)             # :106-107
    nb_dims = loc.shape[-1]                                                  # :108
    input_vol_ndim = vol.dim()

    if vol.dim() not in [nb_dims, nb_dims + 1]:                              # :111-113
        raise Exception("Number of loc Tensors %d does not match volume dimension %d"
                        % (nb_dims, len(vol.shape[:-1])))
    if nb_dims > vol.dim():                                                  # :115-117
        raise Exception("Loc dimension %d does not match volume dimension %d" % (nb_dims, vol.dim()))
    if interp_method != 'linear':                                            # :193-195
        assert interp_method == 'nearest', 'method should be linear or nearest, got: %s' % interp_method

    _lib.require_device(vol, loc)
    if vol.dim() == nb_dims:                                                 # :119-120
        vol = vol.unsqueeze(-1)
    loc = _loc_for(vol, loc)                                                 # :123-127
    vol32, restore = _prepare_vol(vol, interp_method)
    if vol32.dtype == torch.int32 and fill_value is not None and float(fill_value) != int(fill_value):
        raise ValueError('fill_value %r is not representable in the integer volume dtype' % (fill_value,))

    out = _interp_op(vol32, loc, loc.shape[:-1], _lib.LOC_ABSOLUTE, _METHODS[interp_method],
                     fill_value, batched=False, variant=_variant, tune=_tune)
    if restore is not None:
        out = out.to(restore)
    if input_vol_ndim == nb_dims:                                            # :216-218
        out = out[..., 0]
    return out


def _new_shape(vol_shape, zoom_factor):
    return [int(vol_shape[f] * zoom_factor[f]) for f in range(len(zoom_factor))]     # :256-257


def resize(vol, zoom_factor, interp_method='linear'):
    """
    Align-corners resize of one (un-batched) volume (neurite/tf/utils/utils.py:223-262).
    If zoom_factor is a list it determines ndims and vol may or may not carry a channel axis; if it
    is a scalar, vol must be [*vol_shape, C].
    """
    if isinstance(zoom_factor, (list, tuple)):                               # :237-242
        ndims = len(zoom_factor)
        vol_shape = list(vol.shape[:ndims])
        assert len(vol_shape) in (ndims, ndims + 1), \
            "zoom_factor length %d does not match ndims %d" % (len(vol_shape), ndims)
    else:                                                                    # :244-247
        vol_shape = list(vol.shape[:-1])
        ndims = len(vol_shape)
        zoom_factor = [zoom_factor] * ndims
    if all(z == 1 for z in zoom_factor):                                     # :250-251
        return vol
    if interp_method != 'linear':
        assert interp_method == 'nearest', 'method should be linear or nearest, got: %s' % interp_method
    _lib.require_device(vol)
    if vol.dim() not in (ndims, ndims + 1):
        raise Exception("Number of loc Tensors %d does not match volume dimension %d"
                        % (ndims, len(vol.shape[:-1])))
    new_shape = _new_shape(vol_shape, zoom_factor)
    squeeze = vol.dim() == ndims
    v = vol.unsqueeze(-1) if squeeze else vol
    vol32, restore = _prepare_vol(v, interp_method)

    out = _interp_op(vol32, None, new_shape, _lib.LOC_LINSPACE, _METHODS[interp_method], None, batched=False)
    if restore is not None:
        out = out.to(restore)
    return out[..., 0] if squeeze else out


zoom = resize


def resize_labels(ids, zoom_factor, nb_labels=None):
    """
    Align-corners resize of one (un-batched) integer label map [X, Y, Z] or [X, Y] by linear interpolation + arg-max: what
    resize(one_hot(ids), zoom_factor).argmax(-1) gives, without the one-hot tensor (fused.warp_labels on resize's grid, which is formed
    in registers; csrc/warp_argmax.hip).  zoom_factor: a scalar or one factor per axis; the output shape follows resize's rule
    (int(size * factor)).  Any torch integer dtype, returned as it came; ties go to the smaller id.  nb_labels = L: ids outside
    [0, L) are background; None: every int32 value is a label.  Not differentiable.
    """
    from . import fused
    if not isinstance(ids, torch.Tensor):
        raise TypeError('resize_labels: expected a torch.Tensor, got %s' % type(ids).__name__)
    if not isinstance(zoom_factor, (list, tuple)):
        zoom_factor = [zoom_factor] * ids.dim()
    if len(zoom_factor) != ids.dim():
        raise ValueError('resize_labels: %d zoom factors for a label map of rank %d' % (len(zoom_factor), ids.dim()))
    return fused._resize_labels(ids.unsqueeze(0), list(zoom_factor), nb_labels, 'resize_labels')[0]


zoom_labels = resize_labels


def transform(vol, loc_shift, interp_method='linear', indexing='ij', fill_value=None):
    """
    voxelmorph.utils.transform for one (un-batched) volume: out[q] = interpn(vol, q + loc_shift[q]).
    The identity grid is never materialised (the kernel derives q from its thread index).
    vol [*S, C] (or [*S]); loc_shift [*S', D] in voxel units.
    """
    if indexing not in ('ij', 'xy'):
        raise ValueError("indexing has to be 'ij' (matrix) or 'xy' (cartesian)")
    D = loc_shift.shape[-1]
    if vol.dim() not in (D, D + 1):
        raise Exception("Number of loc Tensors %d does not match volume dimension %d"
                        % (D, len(vol.shape[:-1])))
    if interp_method != 'linear':
        assert interp_method == 'nearest', 'method should be linear or nearest, got: %s' % interp_method
    _lib.require_device(vol, loc_shift)
    squeeze = vol.dim() == D
    v = vol.unsqueeze(-1) if squeeze else vol
    shift = loc_shift.to(torch.float32)
    if indexing == 'xy' and D > 1:
        shift = torch.cat([shift[..., 1:2], shift[..., 0:1], shift[..., 2:]], -1)
    vol32, restore = _prepare_vol(v, interp_method)

    out = _interp_op(vol32, shift, shift.shape[:-1], _lib.LOC_SHIFT, _METHODS[interp_method], fill_value,
                     batched=False)
    if restore is not None:
        out = out.to(restore)
    return out[..., 0] if squeeze else out


def affine_to_dense_shift(matrix, shape, shift_center=True, indexing='ij'):
    """
    voxelmorph.utils.affine_to_dense_shift: dense displacement field [*shape, D] of an affine
    [D, D+1] (or [D+1, D+1]); a batch of affines [B, D, D+1] gives [B, *shape, D].  float32.  Device matrices: one kernel
    (csrc/vxm.hip); host matrices, 'xy' indexing and matrices that need a gradient: torch ops (tiny matmul over the grid).
    """
    D = len(shape)
    matrix = torch.as_tensor(matrix, dtype=torch.float32)
    if matrix.shape[-2] == D + 1:
        matrix = matrix[..., :D, :]
    if tuple(matrix.shape[-2:]) != (D, D + 1):
        raise ValueError('affine matrix must be [%d, %d] or [%d, %d]' % (D, D + 1, D + 1, D + 1))
    if (indexing == 'ij' and matrix.device.type == 'cuda' and D in (2, 3) and matrix.dim() in (2, 3)
            and not (torch.is_grad_enabled() and matrix.requires_grad)):
        # one kernel writes the D floats of a voxel (csrc/vxm.hip); a leading batch axis gives [B, *shape, D].  Under autograd
        # (an affine that a network predicted) the differentiable torch form below runs instead.
        m = matrix.detach().contiguous()
        batch = m.shape[0] if m.dim() == 3 else 1
        out = torch.empty(((batch,) if m.dim() == 3 else ()) + tuple(int(n) for n in shape) + (D,), dtype=torch.float32, device=m.device)
        if out.numel():
            _lib.call(m.device, 'nrt_affine_to_dense_shift_f32', _lib.ptr(m), int(batch), D, _lib.ints([int(n) for n in shape]),
                      int(bool(shift_center)), _lib.ptr(out))
        return out
    if matrix.dim() == 3:
        return torch.stack([affine_to_dense_shift(matrix[b], shape, shift_center=shift_center, indexing=indexing)
                            for b in range(matrix.shape[0])], 0)
    if indexing == 'ij' and matrix.device.type == 'cuda':
        # the grid is built where the matrix lives (the host grid + copy cost ~15 ms per 160^3 field)
        lin = [torch.arange(int(n), dtype=torch.float32, device=matrix.device) for n in shape]
        mesh = list(torch.meshgrid(*lin, indexing='ij'))
    else:
        mesh = volshape_to_meshgrid(shape, indexing=indexing)
        mesh = [m.to(matrix.device, torch.float32) for m in mesh]
    if shift_center:
        mesh = [mesh[d] - (shape[d] - 1) / 2 for d in range(D)]
    flat = [m.reshape(-1) for m in mesh]
    flat.append(torch.ones_like(flat[0]))
    mesh_matrix = torch.stack(flat, 0)                        # [D+1, V]
    loc = (matrix @ mesh_matrix).transpose(0, 1).reshape(list(shape) + [D])
    return loc - torch.stack(mesh, -1)


# --------------------------------------------------------------------------------------
# VoxelMorph companions of SpatialTransformer (called by the reference next to it, neurite/tf/models.py:802-804,
# 1131, 1149-1154; voxelmorph itself is not vendored, so these follow its published semantics)
# --------------------------------------------------------------------------------------

def _warp_add(src, shift, batched, interp_method='linear', fill_value=None):
    """
    shift + transform(src, shift) in 'ij' coordinates: one kernel pass (csrc/interpn.hip, nrt_interpn_add_f32).
    src [B?, *S, C], shift [B?, *S', D] float32.  Falls back to the differentiable two-op form under autograd.
    """
    dev = _lib.require_device(src, shift)
    if interp_method != 'linear':
        assert interp_method == 'nearest', 'method should be linear or nearest, got: %s' % interp_method
    if src.dtype != torch.float32 or shift.dtype != torch.float32:
        raise NotImplementedError('displacement fields must be float32')
    D = shift.shape[-1]
    if src.shape[-1] != shift.shape[-1] and src.shape[-1] != D:
        raise ValueError('cannot add a %d-channel warped field to a %d-D displacement' % (src.shape[-1], D))
    needs = torch.is_grad_enabled() and (src.requires_grad or shift.requires_grad)
    out_spatial = list(shift.shape[1:-1] if batched else shift.shape[:-1])
    if needs or interp_method != 'linear':
        return shift + _interp_op(src, shift, out_spatial, _lib.LOC_SHIFT, _METHODS[interp_method], fill_value,
                                  batched=batched)
    src = src.contiguous()
    shift = shift.contiguous()
    B = src.shape[0] if batched else 1
    S = list(src.shape[1:-1] if batched else src.shape[:-1])
    if len(S) != D or D < 1 or D > 3:
        raise Exception("Number of loc Tensors %d does not match volume dimension %d" % (D, len(S)))
    if batched and shift.shape[0] != B:
        raise ValueError('batch size of the two transforms differs')
    Cc = src.shape[-1]
    out = torch.empty_like(shift)
    if out.numel() == 0:
        return out
    has_fill = fill_value is not None
    _lib.call(dev, 'nrt_interpn_add_f32', _lib.ptr(src), _lib.ptr(shift), _lib.ptr(shift), _lib.ptr(out), D, _lib.ints(S),
              _lib.ints(out_spatial), Cc, B, int(np.prod(S)) * Cc, int(np.prod(out_spatial)) * D, int(np.prod(out_spatial)) * Cc,
              _lib.LOC_SHIFT, int(has_fill), float(fill_value) if has_fill else 0.0)
    return out


def integrate_vec(vec, time_dep=False, method='ss', _batched=False, **kwargs):
    """
    voxelmorph.utils.integrate_vec for one stationary velocity field [*S, D] ('ij' coordinates).
    'ss' / 'scaling_and_squaring': vec /= 2**nb_steps; nb_steps x (vec += transform(vec, vec)).
    'quadrature': vec /= nb_steps; disp = vec; (nb_steps - 1) x (disp += transform(vec, disp)).
    """
    if method not in ['ss', 'scaling_and_squaring', 'ode', 'quadrature']:
        raise ValueError("method has to be 'scaling_and_squaring' or 'ode'. found: %s" % method)
    if time_dep:
        raise NotImplementedError('integrate_vec: time-dependent velocity fields are not implemented')
    if method == 'ode':
        raise NotImplementedError("integrate_vec: method='ode' (tf odeint) is not implemented")
    _lib.require_device(vec)
    vec = vec.to(torch.float32)
    nb_steps = kwargs['nb_steps']
    if method in ['ss', 'scaling_and_squaring']:
        assert nb_steps >= 0, 'nb_steps should be >= 0, found: %d' % nb_steps
        vec = vec / (2 ** nb_steps)
        for _ in range(nb_steps):
            vec = _warp_add(vec, vec, _batched)
        return vec
    assert nb_steps >= 1, 'nb_steps should be >= 1, found: %d' % nb_steps
    vec = vec / nb_steps
    disp = vec
    for _ in range(nb_steps - 1):
        disp = _warp_add(vec, disp, _batched)
    return disp


def validate_affine_shape(shape):
    """voxelmorph.utils.validate_affine_shape: (..., N, N+1) or (..., N+1, N+1) with N in (2, 3)."""
    ndim = shape[-1] - 1
    rows = shape[-2]
    if ndim not in (2, 3) or rows not in (ndim, ndim + 1):
        raise ValueError(f'Affine matrix must be of shape (2, 3) or (3, 4), got {tuple(shape[-2:])}.')


def is_affine_shape(shape):
    """voxelmorph.utils.is_affine_shape on a shape without the batch axis."""
    if len(shape) == 2 and shape[-1] != 1:
        validate_affine_shape(shape)
        return True
    return False


def make_square_affine(mat):
    """voxelmorph.utils.make_square_affine: append the homogeneous row to [..., N, N+1] matrices."""
    validate_affine_shape(mat.shape)
    if mat.shape[-2] == mat.shape[-1]:
        return mat
    row = torch.zeros(tuple(mat.shape[:-2]) + (1, mat.shape[-1]), dtype=mat.dtype, device=mat.device)
    row[..., -1] = 1
    return torch.cat([mat, row], -2)


def rescale_affine(mat, factor):
    """voxelmorph.utils.rescale_affine: scale the translation column."""
    return torch.cat([mat[..., :-1], (mat[..., -1] * factor).unsqueeze(-1)], -1)


def rescale_dense_transform(transform_field, factor, interp_method='linear', _batched=False):
    """
    voxelmorph.utils.rescale_dense_transform: resize a displacement field and scale its vectors; the resize comes
    first when shrinking (factor < 1) and last when growing, as upstream.
    """
    from . import layers as _layers

    def rs(t):
        if _batched:
            return _layers.Resize(factor, interp_method=interp_method)(t)
        return resize(t, factor, interp_method=interp_method)

    if factor < 1:
        return rs(transform_field) * factor
    return rs(transform_field * factor)


def compose(transforms, interp_method='linear', shift_center=True, indexing='ij', _batched=False):
    """
    voxelmorph.utils.compose: compose a list of affine matrices and/or dense displacement fields (un-batched) into
    one transform, T = transforms[0] o transforms[1] o ...; the result is dense if any input is.
    """
    if indexing != 'ij':
        raise ValueError('Compose transform only supports ij indexing')
    if len(transforms) < 2:
        raise ValueError('Compose transform list size must be greater than 1')

    def affine(t):
        return is_affine_shape(t.shape[1:] if _batched else t.shape)

    def densify(t, shape):
        if not affine(t):
            return t
        return affine_to_dense_shift(t, shape, shift_center=shift_center, indexing=indexing)     # [B, D, D+1] -> [B, *shape, D]

    curr = transforms[-1]
    for nxt in reversed(transforms[:-1]):
        dense = next((t for t in (nxt, curr) if not affine(t)), None)
        if dense is not None:
            shape = list(dense.shape[1:-1] if _batched else dense.shape[:-1])
            nxt_d, curr_d = densify(nxt, shape), densify(curr, shape)
            curr = _warp_add(nxt_d.to(torch.float32), curr_d.to(torch.float32), _batched, interp_method)
        else:
            curr = torch.matmul(make_square_affine(nxt), make_square_affine(curr))[..., :-1, :]
    return curr


# --------------------------------------------------------------------------------------
# filtering and normalisation (synthesis front-end; neurite/tf/utils/utils.py:581-751, 953-968)
# --------------------------------------------------------------------------------------

def gaussian_kernel(sigma, windowsize=None, indexing='ij', separate=False, random=False, min_sigma=0,
                    dtype=torch.float32, seed=None, device=None, _draws=None):
    """
    N-dimensional Gaussian kernel (utils.py:581-662), or a list of N 1-D kernels with separate=True.  Host-side: the
    kernels are a few dozen numbers.  random=True draws each SD uniformly from [min_sigma, sigma) with torch's RNG
    (the reference uses tf.random.uniform: same distribution, different stream).  sigma is a host number: the gradient with
    respect to sigma is out of scope (the taps it returns are constants of any graph they enter).
    """
    if not dtype.is_floating_point:
        raise AssertionError(f'{dtype} is not a real floating-point type')
    npdt = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16}.get(dtype, np.float32)
    if not isinstance(sigma, (list, tuple)):
        sigma = [sigma]
    if not isinstance(min_sigma, (list, tuple)):
        min_sigma = [min_sigma] * len(sigma)
    sigma = [max(f, np.finfo(npdt).eps) for f in sigma]
    min_sigma = [max(f, np.finfo(npdt).eps) for f in min_sigma]
    if windowsize is None:
        windowsize = [np.round(f * 3) * 2 + 1 for f in sigma]
    if not isinstance(windowsize, (list, tuple)):
        windowsize = [windowsize]
    if len(sigma) != len(windowsize):
        raise ValueError(f'sigma {sigma} and width {windowsize} differ in length')
    center = [(w - 1) / 2 for w in windowsize]
    mesh = [np.arange(w) - c for w, c in zip(windowsize, center)]
    mesh = [-0.5 * x ** 2 for x in mesh]
    if not separate:
        mesh = np.meshgrid(*mesh, indexing=indexing)
    mesh = [torch.as_tensor(np.asarray(m), dtype=dtype, device=device) for m in mesh]
    if random:
        gen = torch.Generator(device='cpu')
        gen.manual_seed(int(np.random.default_rng(seed).integers(2 ** 31 - 1)))
        draws = None if _draws is None else list(_draws)         # tests: the uniform [0, 1) numbers to use

        def uniform():
            return np.float32(draws.pop(0)) if draws is not None else np.float32(float(torch.rand((), generator=gen)))
        # tf.random.uniform(minval=a, maxval=b) = u * (b - a) + a in float32
        sigma = [float(uniform() * np.float32(np.float32(b) - np.float32(a)) + np.float32(a)) for a, b in zip(min_sigma, sigma)]
    exponent = [m / torch.tensor(s, dtype=dtype) ** 2 for m, s in zip(mesh, sigma)]
    if not separate:
        exponent = [torch.stack(exponent).sum(0)]
    kernel = [torch.exp(x) for x in exponent]
    kernel = [x / x.sum() for x in kernel]
    return kernel if len(kernel) > 1 else kernel[0]


def _conv1d_geometry(n, w, padding, stride, dilation):
    """(outputs, padding in front) of one pass over an axis of n samples by the TF rules"""
    ke = (w - 1) * dilation + 1
    if padding.upper() == 'SAME':
        o = -(-n // stride)
        return o, max((o - 1) * stride + ke - n, 0) // 2
    if padding.upper() == 'VALID':
        o = (n - ke) // stride + 1
        if o < 1:
            raise ValueError('Negative dimension size caused by a VALID convolution of width %d along a length-%d axis' % (ke, n))
        return o, 0
    raise ValueError('padding must be "SAME" or "VALID"')


def _conv1d_launch(x, k, ax, o, before, stride, dilation):
    dev = x.device
    n, w = x.shape[ax], k.numel()
    outer = int(np.prod(x.shape[:ax])) if ax else 1
    inner = int(np.prod(x.shape[ax + 1:]))
    y = torch.empty(tuple(x.shape[:ax]) + (o,) + tuple(x.shape[ax + 1:]), dtype=torch.float32, device=dev)
    if y.numel():
        _lib.call(dev, 'nrt_conv1d_axis_f32', _lib.ptr(x), _lib.ptr(k), _lib.ptr(y), outer, n, inner, o, w, int(stride), int(dilation),
                  int(before))
    return y


class _Conv1dAxisFn(torch.autograd.Function):
    """
    One separable pass with the hand-written backward of csrc/filter.hip: the input gradient (stride 1: a forward pass over the
    incoming gradient with the taps reversed; stride > 1: a gather kernel) and, only when the taps require grad, the tap gradient.
    x is saved only for the tap gradient, the taps only for the input gradient.
    """

    @staticmethod
    def forward(ctx, x, k, ax, o, before, stride, dilation):
        y = _conv1d_launch(x, k, ax, o, before, stride, dilation)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, k if ctx.needs_input_grad[0] else None)
        ctx.geom = (tuple(x.shape), ax, o, before, stride, dilation, k.numel())
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, k = ctx.saved_tensors
        shape, ax, o, before, stride, dilation, w = ctx.geom
        dev = grad_y.device
        g = grad_y.contiguous()
        if g.dtype != torch.float32:
            raise NotImplementedError('separable_conv backward: float32 gradients, got %s' % g.dtype)
        n = shape[ax]
        outer = int(np.prod(shape[:ax])) if ax else 1
        inner = int(np.prod(shape[ax + 1:]))
        gx = gk = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(shape, dtype=torch.float32, device=dev)
            if gx.numel():
                _lib.call(dev, 'nrt_conv1d_axis_bwd_f32', _lib.ptr(g), _lib.ptr(k), _lib.ptr(gx), outer, n, inner, o, w, stride, dilation,
                          before)
        if ctx.needs_input_grad[1]:
            gk = torch.empty((w,), dtype=torch.float32, device=dev)
            nws = int(_lib.lib().nrt_conv1d_axis_bwd_kernel_workspace_bytes(outer, o, inner, w))
            ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=dev)
            _lib.call(dev, 'nrt_conv1d_axis_bwd_kernel_f32', _lib.ptr(x), _lib.ptr(g), _lib.ptr(gk), outer, n, inner, o, w, stride,
                      dilation, before, _lib.ptr(ws), nws)
        return gx, gk, None, None, None, None, None


def _conv1d_axis(x, k, ax, padding, stride, dilation):
    """one separable pass along tensor axis `ax` of the contiguous float32 tensor x (csrc/filter.hip); recorded for autograd only
    when grad is enabled and x or the taps require it -- otherwise the launch and the output are those of the forward-only op"""
    o, before = _conv1d_geometry(x.shape[ax], k.numel(), padding, stride, dilation)
    if torch.is_grad_enabled() and (x.requires_grad or k.requires_grad):
        return _Conv1dAxisFn.apply(x, k, ax, o, before, int(stride), int(dilation))
    return _conv1d_launch(x, k, ax, o, before, stride, dilation)


def separable_conv(x, kernels, axis=None, batched=False, padding='SAME', strides=None, dilations=None):
    """
    Apply 1-D kernels along spatial axes of a tensor with a trailing feature dimension, the same filters across
    features (utils.py:665-751).  One kernel pass per axis on the tensor as it lies in memory -- no transposes.
    Differentiable (float32, once) with respect to x and to tap tensors that require grad; taps that already live on x's device are
    used where they are.
    """
    dev = _lib.require_device(x)
    if x.dtype != torch.float32:
        raise NotImplementedError('separable_conv: float32 tensors, got %s' % x.dtype)
    if not batched:
        x = x.unsqueeze(0)
    num_dim = x.dim() - 2
    if np.isscalar(axis):
        axis = [axis]
    axes_space = range(num_dim)
    if axis is None:
        axis = list(axes_space)
    assert all(ax in axes_space for ax in axis), 'non-spatial axis passed'

    def conform(v):
        v = np.ravel(1 if v is None else v).tolist()
        return v * len(axis) if len(v) == 1 else v
    strides, dilations = conform(strides), conform(dilations)
    assert len(strides) == len(axis), 'number of strides and axes differ'
    assert len(dilations) == len(axis), 'number of dilations and axes differ'
    if not isinstance(kernels, (tuple, list)):
        kernels = [kernels]
    if len(kernels) == 1:
        kernels = list(kernels) * len(axis)
    assert len(kernels) == len(axis), 'number of kernels and axes differ'
    x = x.contiguous()
    for ax, k, s, d in zip(axis, kernels, strides, dilations):
        if isinstance(k, torch.Tensor):                          # keeps the graph of a tap tensor; no copy if it is in place already
            k = k.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        else:
            k = torch.as_tensor(k, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        x = _conv1d_axis(x, k, ax + 1, padding, int(s), int(d))
    return x if batched else x[0]


def _minmax_launch(x, outer, red, inner):
    dev = x.device
    y = torch.empty_like(x)
    nws = _lib.lib().nrt_minmax_workspace_bytes(outer, inner)
    ws = torch.empty((max(int(nws), 16),), dtype=torch.uint8, device=dev)
    _lib.call(dev, 'nrt_minmax_norm_f32', _lib.ptr(x), _lib.ptr(y), outer, red, inner, _lib.ptr(ws), nws)
    return y


class _MinmaxNormFn(torch.autograd.Function):
    """minmax_norm with the backward of csrc/filter.hip (ties of the extrema share their gradient evenly; a constant group gets 0)."""

    @staticmethod
    def forward(ctx, x, outer, red, inner):
        ctx.save_for_backward(x)
        ctx.geom = (outer, red, inner)
        return _minmax_launch(x, outer, red, inner)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, = ctx.saved_tensors
        outer, red, inner = ctx.geom
        dev = x.device
        g = grad_y.contiguous()
        if g.dtype != torch.float32:
            raise NotImplementedError('minmax_norm backward: float32 gradients, got %s' % g.dtype)
        gx = torch.empty_like(x)
        nws = int(_lib.lib().nrt_minmax_norm_bwd_workspace_bytes(outer, red, inner))
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=dev)
        _lib.call(dev, 'nrt_minmax_norm_bwd_f32', _lib.ptr(x), _lib.ptr(g), _lib.ptr(gx), outer, red, inner, _lib.ptr(ws), nws)
        return gx, None, None, None


def minmax_norm(x, axis=None):
    """
    Min-max normalise with a safe division (utils.py:953-968).  axis: dimensions to reduce (None = all); they must
    form one contiguous run (e.g. all, all but the batch, all spatial axes of a channels-last batch).  Differentiable (float32, once).
    """
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise NotImplementedError('minmax_norm: float32 tensors, got %s' % x.dtype)
    nd = x.dim()
    axes = sorted(set(range(nd))) if axis is None else sorted(set(int(a) % nd for a in np.ravel(axis)))
    if not axes or axes != list(range(axes[0], axes[-1] + 1)):
        raise NotImplementedError('minmax_norm: the reduced axes must be contiguous, got %r' % (axis,))
    x = x.contiguous()
    outer = int(np.prod(x.shape[:axes[0]])) if axes[0] else 1
    red = int(np.prod(x.shape[axes[0]:axes[-1] + 1]))
    inner = int(np.prod(x.shape[axes[-1] + 1:]))
    if x.numel() == 0:
        return torch.empty_like(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _MinmaxNormFn.apply(x, outer, red, inner)
    return _minmax_launch(x, outer, red, inner)


def _device_minmax(x):
    """[min, max] of a float32 tensor as a 2-element device tensor (csrc/filter.hip; no host synchronisation)."""
    lib = _lib.lib()
    dev = x.device
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    nws = int(lib.nrt_minmax_workspace_bytes(1, 1))
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _lib.call(dev, 'nrt_minmax_f32', _lib.ptr(x), x.numel(), _lib.ptr(out), _lib.ptr(ws), nws)
    return out


def _bin_centers(x, bin_centers, nb_bins):
    """bin centres of soft_quantize as a float32 device tensor: given, or tf.linspace(min(x), max(x), nb_bins) (:1152-1154)."""
    dev = x.device
    if bin_centers is not None:
        assert nb_bins is None, 'cannot provide both bin_centers and nb_bins'
        return torch.as_tensor(bin_centers, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    if nb_bins is None:
        nb_bins = 16
    # one reduction + one tiny kernel (csrc/filter.hip): start + delta * i, the ends exact as tf.linspace's are
    lib = _lib.lib()
    x = x.contiguous()
    c = torch.empty((int(nb_bins),), dtype=torch.float32, device=dev)
    nws = int(lib.nrt_minmax_workspace_bytes(1, 1))
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _lib.call(dev, 'nrt_bin_centers_f32', _lib.ptr(x), x.numel(), int(nb_bins), _lib.ptr(c), _lib.ptr(ws), nws)
    return c


def soft_quantize(x, bin_centers=None, nb_bins=16, alpha=1, min_clip=-np.inf, max_clip=np.inf, return_log=False):
    """
    (Softly) quantise the values of a tensor with RBFs (utils.py:1099-1172): value v gets weight exp(-alpha (v - c)^2) for
    every bin centre c.  Returns a tensor with one more dimension [..., B].  Specify bin_centers OR nb_bins (centres are then
    spread between the extrema of x).
    """
    dev = _lib.require_device(x)
    if x.dtype != torch.float32:
        raise NotImplementedError('soft_quantize: float32 tensors, got %s' % x.dtype)
    x = x.contiguous()
    centers = _bin_centers(x.detach(), bin_centers, nb_bins)
    cfg = (float(alpha), float(min_clip), float(max_clip), int(bool(return_log)))
    if torch.is_grad_enabled() and x.requires_grad:
        return _SoftQuantizeFn.apply(x, centers, cfg)
    return _soft_quantize_fwd(x, centers, cfg)


def _soft_quantize_fwd(x, centers, cfg):
    dev = x.device
    nb = centers.numel()
    out = torch.empty(tuple(x.shape) + (nb,), dtype=torch.float32, device=dev)
    if x.numel():
        _lib.call(dev, 'nrt_soft_quantize_f32', _lib.ptr(x), _lib.ptr(centers), cfg[0], cfg[1], cfg[2], cfg[3], _lib.ptr(out), x.numel(),
                  nb)
    return out


class _SoftQuantizeFn(torch.autograd.Function):
    """soft_quantize with its backward wrt x (csrc/mi.hip: soft_quantize_bwd).  The bin centres are treated as constants:
    when they come from tf.linspace(min(x), max(x)) the reference also sends a term to the two extremal voxels -- the same
    convention as the fused MutualInformation backward."""

    @staticmethod
    def forward(ctx, x, centers, cfg):
        ctx.save_for_backward(x, centers)
        ctx.cfg = cfg
        with torch.no_grad():
            return _soft_quantize_fwd(x, centers, cfg)

    @staticmethod
    def backward(ctx, g):
        x, centers = ctx.saved_tensors
        cfg = ctx.cfg
        dev = x.device
        g = g.to(torch.float32).contiguous()
        gx = torch.empty_like(x)
        if x.numel():
            _lib.call(dev, 'nrt_soft_quantize_bwd_f32', _lib.ptr(x), _lib.ptr(centers), cfg[0], cfg[1], cfg[2], cfg[3], _lib.ptr(g),
                      _lib.ptr(gx), x.numel(), centers.numel())
        return gx, None, None


def soft_digitize(*args, **kwargs):
    """alias of soft_quantize (utils.py:1095-1096)"""
    return soft_quantize(*args, **kwargs)


_BARYCENTER_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}


def _barycenter_axes(axes, nd):
    """axes of barycenter as a list of distinct non-negative ints, in the order given"""
    if axes is None:
        return list(range(nd))
    axes = [axes] if isinstance(axes, (int, np.integer)) else list(axes)
    out = []
    for ax in axes:
        if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)):
            raise ValueError('barycenter: axes must be ints, got %r' % (ax,))
        if not -nd <= ax < nd:
            raise ValueError('barycenter: axis %d is out of range for a tensor of %d dimensions' % (ax, nd))
        out.append(int(ax) % nd)
    if len(set(out)) != len(out):
        raise ValueError('barycenter: duplicate axes in %r' % (axes,))
    if not out:
        raise ValueError('barycenter: no axes to reduce')
    return out


class _BarycenterFn(torch.autograd.Function):
    """x [outer, *red, inner] contiguous (float32 / bfloat16 / float16) -> y [outer, inner, k] float32 (csrc/barycenter.hip).  The
    backward needs y and the sums the forward leaves, not x."""

    @staticmethod
    def forward(ctx, x, red, flags):
        lib = _lib.lib()
        dev = x.device
        k = len(red)
        outer, inner = int(x.shape[0]), int(x.shape[-1])
        code = _BARYCENTER_DTYPES[x.dtype]
        y = torch.empty((outer, inner, k), dtype=torch.float32, device=dev)
        sums = torch.empty((outer, inner, k + 1), dtype=torch.float32, device=dev)
        shape = _lib.ints(red)
        nws = int(lib.nrt_barycenter_workspace_bytes(code, outer, shape, k, inner))
        ws = _lib.workspace(dev, max(nws, 16))
        _lib.call(dev, 'nrt_barycenter', _lib.ptr(x), code, outer, shape, k, inner, flags[0], flags[1], _lib.ptr(y), _lib.ptr(sums),
                  _lib.ptr(ws), nws)
        ctx.save_for_backward(y, sums)
        ctx.cfg = (code, outer, tuple(red), inner, flags, x.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, sums = ctx.saved_tensors
        code, outer, red, inner, flags, dtype = ctx.cfg
        lib = _lib.lib()
        dev = y.device
        k = len(red)
        gy = gy.to(torch.float32).contiguous()
        gx = torch.empty((outer,) + red + (inner,), dtype=dtype, device=dev)
        shape = _lib.ints(red)
        nws = int(lib.nrt_barycenter_workspace_bytes(code, outer, shape, k, inner))
        ws = _lib.workspace(dev, max(nws, 16))
        _lib.call(dev, 'nrt_barycenter_bwd', _lib.ptr(gy), _lib.ptr(y), _lib.ptr(sums), code, outer, shape, k, inner, flags[0], flags[1],
                  _lib.ptr(gx), _lib.ptr(ws), nws)
        return gx, None, None


def barycenter(x, axes=None, normalize=False, shift_center=False, dtype=torch.float32):
    """
    Barycenter (centre of mass) along the given axes (utils.py:512-573), in one pass over x (csrc/barycenter.hip).

    x:            tensor of any type; float32, bfloat16 and float16 are read as stored, anything else is cast to float32 first.
    axes:         axes along which to compute the barycenter, an int or a sequence of ints; None means all axes.  Negative axes count
                  from the end (the reference fails on them); duplicates and out-of-range values raise ValueError.
    normalize:    normalise the grid dimensions to unit length.
    shift_center: shift the grid to the image centre.
    dtype:        output data type; the computation always uses single precision.

    Returns [*kept axes in their order, len(axes)]; the last index runs over `axes` in the order given.  Where x sums to zero the result
    is exactly 0 (tf.math.divide_no_nan).  Differentiable in x, the gradient comes back in x's dtype; nothing travels to the host, so
    a forward + backward captures into a graph.

    Axes that form an ascending run of neighbours (all axes, the spatial axes of a channels-last batch, trailing axes) are reduced in
    place from a contiguous x; any other `axes` pays one permute(...).contiguous() copy of x that moves them to the end.
    """
    if not isinstance(x, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(x).__name__)
    nd = x.dim()
    if nd == 0:
        raise ValueError('barycenter: x has no axes')
    axes = _barycenter_axes(axes, nd)
    _lib.require_device(x)
    if x.dtype not in _BARYCENTER_DTYPES:
        x = x.to(torch.float32)
    k = len(axes)
    if k > 8:
        raise NotImplementedError('barycenter: up to 8 axes, got %d' % k)
    kept = [ax for ax in range(nd) if ax not in axes]
    if axes != list(range(axes[0], axes[0] + k)):
        x = x.permute(*kept, *axes)                     # as the reference moves them: one copy
        lead, trail = [int(x.shape[i]) for i in range(len(kept))], []
    else:
        lead, trail = [int(v) for v in x.shape[:axes[0]]], [int(v) for v in x.shape[axes[0] + k:]]
    red = tuple(int(x.shape[len(lead) + i]) for i in range(k))
    out_shape = tuple(lead) + tuple(trail) + (k,)
    if x.numel() == 0:
        return torch.zeros(out_shape, dtype=dtype, device=x.device)
    outer, inner = int(np.prod(lead, dtype=np.int64)), int(np.prod(trail, dtype=np.int64))
    x3 = x.contiguous().view((outer,) + red + (inner,))
    y = _BarycenterFn.apply(x3, red, (int(bool(normalize)), int(bool(shift_center)))).view(out_shape)
    return y if dtype == torch.float32 else y.to(dtype)


# --------------------------------------------------------------------------------------
# the Jacobian determinant of a displacement field (csrc/jacobian.hip)
# --------------------------------------------------------------------------------------

def _jacdet_checked(disp, what):
    """the host-side checks of a field, before its device is looked at: returns (disp [B, *S, D] contiguous, batched)"""
    if not isinstance(disp, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(disp).__name__))
    disp = materialize(disp)
    if disp.dim() < 2:
        raise ValueError('%s: expected [*spatial, D] or [batch, *spatial, D], got shape %s' % (what, tuple(disp.shape)))
    D = int(disp.shape[-1])
    batched = disp.dim() != D + 1                       # the rank decides: [*S, D] has D + 1 axes
    nd = disp.dim() - (2 if batched else 1)
    if nd not in (2, 3):
        raise NotImplementedError('%s: 2 or 3 spatial axes, got shape %s' % (what, tuple(disp.shape)))
    if D != nd:
        raise ValueError('%s: %d spatial axes need %d channels, got shape %s' % (what, nd, nd, tuple(disp.shape)))
    if disp.dtype != torch.float32:
        raise NotImplementedError('%s: float32 only, got %s' % (what, disp.dtype))
    if not batched:
        disp = disp.unsqueeze(0)
    if disp.shape[0] < 1 or any(int(v) < 2 for v in disp.shape[1:-1]):
        raise ValueError('%s: every spatial extent must be at least 2 (and the batch at least 1), got shape %s' % (what, tuple(disp.shape)))
    if disp.shape[0] > 65535 or disp.numel() >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 elements, got shape %s' % (what, tuple(disp.shape)))
    _lib.require_device(disp)
    return disp.contiguous(), batched


def _jacdet_launch(disp, want_det=False, want_stats=False, want_loss=False):
    """one pass of nrt_jacdet_f32 over disp [B, *S, D] (checked, contiguous): (det [B, *S] | None, stats [B, 5] float64 | None,
    loss [B] | None).  Slot 0 of a stats row holds an int64."""
    dev = disp.device
    batch, shape = int(disp.shape[0]), [int(v) for v in disp.shape[1:-1]]
    cshape = _lib.ints(shape)
    det = torch.empty(tuple(disp.shape[:-1]), dtype=torch.float32, device=dev) if want_det else None
    stats = torch.empty((batch, 5), dtype=torch.float64, device=dev) if want_stats else None
    loss = torch.empty((batch,), dtype=torch.float32, device=dev) if want_loss else None
    ws, nws = None, 0
    if want_stats or want_loss:
        nws = int(_lib.lib().nrt_jacdet_workspace_bytes(batch, cshape, len(shape)))
        ws = _lib.workspace(dev, max(nws, 16))
    _lib.call(dev, 'nrt_jacdet_f32', _lib.ptr(disp), batch, cshape, len(shape), _lib.ptr(det), _lib.ptr(stats), _lib.ptr(loss),
              _lib.ptr(ws), nws)
    return det, stats, loss


class _JacDetFn(torch.autograd.Function):
    """disp [B, *S, D] float32 contiguous -> the map [B, *S] (as_loss False) or mean(max(0, -det)) [B] (as_loss True).  The backward
    keeps disp only: one gather pass rebuilds the Jacobian."""

    @staticmethod
    def forward(ctx, disp, as_loss):
        det, _, loss = _jacdet_launch(disp, want_det=not as_loss, want_loss=as_loss)
        ctx.save_for_backward(disp)
        ctx.as_loss = as_loss
        return loss if as_loss else det

    @staticmethod
    def backward(ctx, g):
        disp, = ctx.saved_tensors
        dev = disp.device
        g = g.to(torch.float32).contiguous()
        gdisp = torch.empty_like(disp)
        shape = [int(v) for v in disp.shape[1:-1]]
        _lib.call(dev, 'nrt_jacdet_bwd_f32', _lib.ptr(disp), None if ctx.as_loss else _lib.ptr(g), _lib.ptr(g) if ctx.as_loss else None,
                  int(disp.shape[0]), _lib.ints(shape), len(shape), _lib.ptr(gdisp))
        return gdisp, None


def jacobian_determinant(disp):
    """
    The Jacobian determinant of the transform x -> x + disp(x) at every voxel: vxm.py.utils.jacobian_determinant, restated (voxelmorph
    is not in the reference tree) and computed on the device (csrc/jacobian.hip).

    disp: [B, *S, D] or, as the VoxelMorph function takes it, [*S, D]; D = len(S) in {2, 3}, float32, 'ij' coordinates.  The rank
          decides: a tensor of D + 1 axes (D = shape[-1]) is unbatched.  A non-contiguous field is made contiguous.

    Returns the map [B, *S] (or [*S]) in float32: the derivatives are np.gradient's (central differences inside, one-sided first-order
    differences at both ends of an axis), so every spatial extent must be at least 2 (ValueError, as np.gradient raises).  VoxelMorph's
    own result is float64 (float32 + an integer grid promotes); this one differs from it by at most 12 * 2^-24 * sum over the
    permutations pi of prod_a (|G[a][pi(a)]| + delta).  Differentiable in disp; nothing travels to the host, so forward and backward
    capture into a graph.
    """
    disp, batched = _jacdet_checked(disp, 'jacobian_determinant')
    det = _JacDetFn.apply(disp, False)
    return det if batched else det[0]


# --------------------------------------------------------------------------------------
# exact Euclidean distance transforms (csrc/edt.hip)
# --------------------------------------------------------------------------------------

_EDT_MAX_EXTENT, _EDT_MAX_LABELS = 1024, 256
_edt_label_cache = {}


def _edt_sampling(sampling, nd, what):
    """None, a scalar or nd voxel sizes -> None or a tuple of nd float32 values held as Python floats"""
    if sampling is None:
        return None
    vals = np.asarray(sampling, dtype=np.float64).reshape(-1)
    if vals.size == 1:
        vals = np.repeat(vals, nd)
    if vals.size != nd:
        raise ValueError('%s: sampling must be a scalar or %d voxel sizes, got %r' % (what, nd, sampling))
    if not np.all(np.isfinite(vals)) or not np.all(vals > 0):
        raise ValueError('%s: voxel sizes must be finite and positive, got %r' % (what, sampling))
    return tuple(float(np.float32(v)) for v in vals)


def _edt_check_geometry(shape, channels, what):
    """the limits of csrc/edt.hip for out [B, *S, channels], before the device is looked at"""
    batch, spatial = int(shape[0]), [int(v) for v in shape[1:]]
    if len(spatial) not in (2, 3):
        raise NotImplementedError('%s: 2 or 3 spatial axes, got %d (shape %s)' % (what, len(spatial), tuple(shape)))
    if batch < 1 or any(v < 1 for v in spatial):
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(shape)))
    if any(v > _EDT_MAX_EXTENT for v in spatial):
        raise NotImplementedError('%s: extents up to %d, got shape %s' % (what, _EDT_MAX_EXTENT, tuple(shape)))
    if not 1 <= channels <= _EDT_MAX_LABELS:
        raise NotImplementedError('%s: 1 to %d labels, got %d' % (what, _EDT_MAX_LABELS, channels))
    if batch > 65535 or batch * int(np.prod(spatial, dtype=np.int64)) * channels >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 output elements, got shape %s x %d labels'
                                  % (what, tuple(shape), channels))


def _edt_labels(labels, what):
    """a label list -> a tuple of distinct Python ints that int32 holds"""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    arr = np.asarray(labels).reshape(-1)
    if arr.size and not np.all(arr == np.round(arr)):
        raise ValueError('%s: label ids must be integers, got %r' % (what, labels))
    ids = tuple(int(v) for v in arr)
    if len(set(ids)) != len(ids):
        raise ValueError('%s: label ids must be distinct, got %r' % (what, ids))
    if any(not -2 ** 31 <= v < 2 ** 31 for v in ids):
        raise ValueError('%s: label ids must fit int32, got %r' % (what, ids))
    return ids


def _edt_label_tensor(ids, dev):
    """the int32 device copy of a label tuple, made once per (device, list): no host-to-device copy on later calls, so they capture"""
    key = (dev, ids)
    t = _edt_label_cache.get(key)
    if t is None:
        t = torch.tensor(ids, dtype=torch.int32).to(dev)
        _edt_label_cache[key] = t
    return t


def _edt_ids_checked(ids, what):
    """an integer or bool label map, checked on the host (the callers convert it to int32 once its device is known)"""
    if not isinstance(ids, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(ids).__name__))
    ids = materialize(ids)
    if ids.dtype.is_floating_point or ids.dtype.is_complex:
        raise NotImplementedError('%s: an integer (or bool) label map, got %s' % (what, ids.dtype))
    return ids


def _edt_launch(out_shape, dev, mask=None, ids=None, labels=None, sampling=None, flags=0):
    """nrt_edt_f32 into a new tensor of out_shape = [B, *S, channels]; mask uint8 [B, *S] or ids int32 [B, *S] + labels (device int32)"""
    batch, spatial, channels = int(out_shape[0]), [int(v) for v in out_shape[1:-1]], int(out_shape[-1])
    cshape = _lib.ints(spatial)
    out = torch.empty(tuple(out_shape), dtype=torch.float32, device=dev)
    ws, nws = None, 0
    if flags & _lib.EDT_SIGNED:
        nws = int(_lib.lib().nrt_edt_workspace_bytes(batch, cshape, len(spatial), channels))
        ws = _lib.workspace(dev, max(nws, 16))
    csamp = (C.c_float * len(spatial))(*sampling) if sampling is not None else None
    _lib.call(dev, 'nrt_edt_f32', _lib.ptr(mask), _lib.ptr(ids), _lib.ptr(labels), 1 if labels is None else int(labels.numel()), batch,
              cshape, len(spatial), csamp, int(flags), _lib.ptr(out), _lib.ptr(ws), nws)
    return out


def _dist_trf(bwvol, sampling, squared, batched, signed, what):
    if not isinstance(bwvol, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(bwvol).__name__))
    bwvol = materialize(bwvol)
    if bwvol.dtype.is_complex:
        raise NotImplementedError('%s: a real volume, got %s' % (what, bwvol.dtype))
    vol = bwvol if batched else bwvol.unsqueeze(0)
    if vol.dim() < 2:
        raise ValueError('%s: expected [*spatial]%s, got shape %s' % (what, ' behind a batch axis' if batched else '', tuple(bwvol.shape)))
    _edt_check_geometry(vol.shape, 1, what)
    samp = _edt_sampling(sampling, vol.dim() - 1, what)
    dev = _lib.require_device(vol)
    if vol.dtype == torch.bool:
        vol = vol.contiguous().view(torch.uint8)
    elif vol.dtype != torch.uint8:
        vol = vol.ne(0).view(torch.uint8)                # (any other dtype: "nonzero" is decided here, one elementwise op)
    flags = (_lib.EDT_SIGNED if signed else 0) | (_lib.EDT_SQUARED if squared else 0)
    out = _edt_launch(tuple(vol.shape) + (1,), dev, mask=vol.contiguous(), sampling=samp, flags=flags).squeeze(-1)
    return out if batched else out[0]


def dist_trf(bwvol, sampling=None, squared=False, batched=False):
    """
    Euclidean distance from every voxel to the nearest nonzero voxel of bwvol, 0 on the set: VoxelMorph's dist_trf,
    scipy.ndimage.distance_transform_edt(~bwvol), restated (voxelmorph is not in the reference tree) and computed exactly
    on the device (csrc/edt.hip) -- nothing travels to the host, so the call captures into a graph.

    bwvol:    [*S], or [B, *S] with batched=True; len(S) in {2, 3}, every extent at most 1024.  bool and uint8 are read as they are;
              any other real dtype goes through one `!= 0`.
    sampling: None (unit voxels), a scalar, or len(S) voxel sizes, as scipy's argument.
    squared:  the squared distance, without the root.
    Returns float32 of bwvol's shape.  At unit spacing the result is the correctly rounded root of the exact integer squared distance
    (scipy's float64 result rounded to float32); with a sampling, d^2 is within 6 * 2^-24 and d within 4 * 2^-24 relative of the exact
    values at the float32 voxel sizes.  Not differentiable: the input is a set.

    Deviation from scipy: an EMPTY set gives +inf everywhere.  scipy returns arbitrary finite values when its input has no background.
    """
    return _dist_trf(bwvol, sampling, squared, batched, False, 'dist_trf')


def signed_dist_trf(bwvol, sampling=None, squared=False, batched=False):
    """
    VoxelMorph's signed_dist_trf (posdst * ~bw - negdst * bw; restated): +d(p, set) outside the set of nonzero voxels,
    -d(p, complement) inside it; with squared=True the squared distances carry the sign.  Arguments, limits and accuracy as `dist_trf`.

    Deviations: an EMPTY set gives +inf everywhere and a FULL set -inf everywhere (VoxelMorph's expression gives NaN from inf * 0 on
    top of scipy's arbitrary values there).
    """
    return _dist_trf(bwvol, sampling, squared, batched, True, 'signed_dist_trf')


def vol_to_sdt(X_label, sdt=True, sdt_vol_resize=1):
    """
    VoxelMorph's vol_to_sdt (restated): the signed distance transform of one volume [*S], its absolute value with
    sdt=False.  sdt_vol_resize != 1 is not implemented.
    """
    if sdt_vol_resize != 1:
        raise NotImplementedError('vol_to_sdt: sdt_vol_resize != 1 is not implemented')
    X_dt = _dist_trf(X_label, None, False, False, True, 'vol_to_sdt')
    return X_dt if sdt else X_dt.abs()


def vol_to_sdt_batch(X_label, sdt=True, sdt_vol_resize=1):
    """VoxelMorph's vol_to_sdt_batch (restated): `vol_to_sdt` of every entry of [B, *S, 1], returned as [B, *S, 1]; one launch set."""
    if sdt_vol_resize != 1:
        raise NotImplementedError('vol_to_sdt_batch: sdt_vol_resize != 1 is not implemented')
    if not isinstance(X_label, torch.Tensor):
        raise TypeError('vol_to_sdt_batch: expected a torch.Tensor, got %s' % type(X_label).__name__)
    if X_label.dim() < 3 or X_label.shape[-1] != 1:
        raise ValueError('vol_to_sdt_batch: expected [batch, *spatial, 1], got shape %s' % (tuple(X_label.shape),))
    X_dt = _dist_trf(materialize(X_label)[..., 0], None, False, True, True, 'vol_to_sdt_batch').unsqueeze(-1)
    return X_dt if sdt else X_dt.abs()


def _label_dist_trf(ids, labels, sampling, flags, what, any_of=False):
    """ids [B, *S] integer, labels a tuple of ints -> [B, *S, L] (or [B, *S, 1] with any_of), checked"""
    ids = _edt_ids_checked(ids, what)
    if ids.dim() < 2:
        raise ValueError('%s: expected [batch, *spatial], got shape %s' % (what, tuple(ids.shape)))
    if not 1 <= len(labels) <= _EDT_MAX_LABELS:
        raise NotImplementedError('%s: 1 to %d labels, got %d' % (what, _EDT_MAX_LABELS, len(labels)))
    channels = 1 if any_of else len(labels)
    _edt_check_geometry(ids.shape, channels, what)
    samp = _edt_sampling(sampling, ids.dim() - 1, what)
    dev = _lib.require_device(ids)
    ids = ids.to(torch.int32).contiguous()
    return _edt_launch(tuple(ids.shape) + (channels,), dev, ids=ids, labels=_edt_label_tensor(labels, dev), sampling=samp,
                       flags=flags | (_lib.EDT_ANY_OF if any_of else 0))


def label_dist_trf(ids, labels, signed=False, sampling=None, squared=False):
    """
    The distance transform of every label of an integer label map at once (an extension): channel l of the result
    [B, *S, L] is `dist_trf` (or `signed_dist_trf`) of ids == labels[l], and all L come from one read of the id map -- no one-hot
    volume and no mask exist.  ids [B, *S] integer (bool counts as 0 / 1); labels: 1 to 256 distinct ids; a label that does not occur
    gives +inf in its channel.  Limits and accuracy as `dist_trf`; B * prod(S) * L must stay below 2^31.
    """
    labels = _edt_labels(labels, 'label_dist_trf')
    flags = (_lib.EDT_SIGNED if signed else 0) | (_lib.EDT_SQUARED if squared else 0)
    return _label_dist_trf(ids, labels, sampling, flags, 'label_dist_trf')


# --------------------------------------------------------------------------------------
# connected components and the mask clean-up built on them (csrc/ccl.hip)
# --------------------------------------------------------------------------------------

def _ccl_check_geometry(shape, connectivity, what):
    """the limits of csrc/ccl.hip for an input [B, *S], before the device is looked at"""
    batch, spatial = int(shape[0]), [int(v) for v in shape[1:]]
    if len(spatial) not in (2, 3):
        raise NotImplementedError('%s: 2 or 3 spatial axes, got %d (shape %s)' % (what, len(spatial), tuple(shape)))
    if batch < 1 or any(v < 1 for v in spatial):
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(shape)))
    if isinstance(connectivity, bool) or connectivity != int(connectivity) or not 1 <= int(connectivity) <= len(spatial):
        raise ValueError('%s: connectivity 1 to %d, got %r' % (what, len(spatial), connectivity))
    if batch > 65535 or batch * int(np.prod(spatial, dtype=np.int64)) >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 voxels, got shape %s' % (what, tuple(shape)))


def _ccl_source(x, labels, connectivity, batched, what, invert=False):
    """x (a mask, or with labels an id map) -> (dev, mask uint8 or None, ids int32 or None, label tensor or None, L, shape [B, *S])"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(x).__name__))
    x = materialize(x)
    if labels is not None:
        labels = _edt_labels(labels, what)
        if not 1 <= len(labels) <= _EDT_MAX_LABELS:
            raise NotImplementedError('%s: 1 to %d labels, got %d' % (what, _EDT_MAX_LABELS, len(labels)))
        if x.dtype.is_floating_point or x.dtype.is_complex:
            raise NotImplementedError('%s: an integer (or bool) label map, got %s' % (what, x.dtype))
    elif x.dtype.is_complex:
        raise NotImplementedError('%s: a real volume, got %s' % (what, x.dtype))
    vol = x if batched else x.unsqueeze(0)
    if vol.dim() < 2:
        raise ValueError('%s: expected [*spatial]%s, got shape %s' % (what, ' behind a batch axis' if batched else '', tuple(x.shape)))
    _ccl_check_geometry(vol.shape, connectivity, what)
    dev = _lib.require_device(vol)
    if labels is not None:
        return dev, None, vol.to(torch.int32).contiguous(), _edt_label_tensor(labels, dev), len(labels), tuple(vol.shape)
    if vol.dtype == torch.bool:
        vol = vol.contiguous().view(torch.uint8)
    elif vol.dtype != torch.uint8:
        vol = vol.ne(0).view(torch.uint8)                # (any other dtype: "nonzero" is decided here, one elementwise op)
    return dev, vol.contiguous(), None, None, 1, tuple(vol.shape)


def _ccl_workspace(dev, shape, nlabels):
    cshape = _lib.ints(shape[1:])
    nws = int(_lib.lib().nrt_ccl_workspace_bytes(shape[0], cshape, len(shape) - 1, nlabels))
    return cshape, _lib.workspace(dev, max(nws, 16)), nws


def _ccl_select(x, labels, connectivity, batched, what, mode=0, min_size=0, fill=0, want_table=False, want_out=True):
    """nrt_ccl_select -> (out or None: uint8 [B, *S] for a mask, int32 for an id map; table int32 [B, L, 2] or None)"""
    dev, mask, ids, lab, nlabels, shape = _ccl_source(x, labels, connectivity, batched, what)
    cshape, ws, nws = _ccl_workspace(dev, shape, nlabels)
    out = torch.empty(shape, dtype=torch.uint8 if ids is None else torch.int32, device=dev) if want_out else None
    table = torch.empty((shape[0], nlabels, 2), dtype=torch.int32, device=dev) if want_table else None
    _lib.call(dev, 'nrt_ccl_select', _lib.ptr(mask), _lib.ptr(ids), _lib.ptr(lab), nlabels, shape[0], cshape, len(shape) - 1,
              int(connectivity), int(mode), int(min_size), int(fill), _lib.ptr(table), _lib.ptr(out), _lib.ptr(ws), nws)
    return out, table


def _ccl_like(out, x, batched):
    """a uint8 0 / 1 mask [B, *S] as a mask of x's dtype and batching"""
    out = out.view(torch.bool) if x.dtype == torch.bool else out if x.dtype == torch.uint8 else out.to(x.dtype)
    return out if batched else out[0]


def _ccl_fill(fill, what):
    if isinstance(fill, bool) or fill != int(fill) or not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError('%s: fill must be an integer that int32 holds, got %r' % (what, fill))
    return int(fill)


def connected_components(x, connectivity=1, labels=None, batched=False):
    """
    Connected components of a mask or of every listed label of an id map at once: scipy.ndimage.label(x,
    generate_binary_structure(nd, connectivity)), computed on the device (csrc/ccl.hip) -- nothing travels to the host, so
    the call captures into a graph.

    x:            [*S], or [B, *S] with batched=True; len(S) in {2, 3}, B * prod(S) < 2^31.  Without `labels` a mask: bool and uint8 are
                  read as they are, any other real dtype goes through one `!= 0`.  With `labels` (1 to 256 distinct ids) an integer id
                  map: the listed ids are foreground, and two neighbours belong to one component when they carry the SAME id.
    connectivity: 1 .. len(S): neighbours differ in at most that many coordinates (4 / 8 in 2-D, 6 / 18 / 26 in 3-D).
    Returns (components, count): components int32 of x's shape, 0 on the background, numbered 1, 2, ... in raster order of each
    component's first voxel, per batch entry (scipy's numbering, bit for bit); count int32 [B] on the device, 0-d when not batched.
    Not differentiable: the input is a set.
    """
    what = 'connected_components'
    dev, mask, ids, lab, nlabels, shape = _ccl_source(x, labels, connectivity, batched, what)
    cshape, ws, nws = _ccl_workspace(dev, shape, nlabels)
    comp = torch.empty(shape, dtype=torch.int32, device=dev)
    count = torch.empty((shape[0],), dtype=torch.int32, device=dev)
    _lib.call(dev, 'nrt_ccl_label_i32', _lib.ptr(mask), _lib.ptr(ids), _lib.ptr(lab), nlabels, shape[0], cshape, len(shape) - 1,
              int(connectivity), _lib.ptr(comp), _lib.ptr(count), _lib.ptr(ws), nws)
    return (comp, count) if batched else (comp[0], count[0])


def largest_component(mask, connectivity=1, batched=False):
    """
    The largest connected component of a mask, per batch entry, as a mask of the input's dtype; of several of the largest size, the first
    in raster order (np.argmax of the bincount of scipy.ndimage.label).  An empty mask stays empty.  Arguments and limits as
    `connected_components`; on the device, graph-capturable, not differentiable.
    """
    out, _ = _ccl_select(mask, None, connectivity, batched, 'largest_component', mode=_lib.CCL_LARGEST)
    return _ccl_like(out, mask, batched)


def keep_largest_components(ids, labels, connectivity=1, fill=0, batched=False):
    """
    An integer id map with everything but the largest component of each listed label set to `fill` (ties: the first component in raster
    order); ids outside the list pass through unchanged.  One labelling pass serves all labels.  Returns int32 of ids' shape.
    Arguments and limits as `connected_components`; on the device, graph-capturable, not differentiable.
    """
    what = 'keep_largest_components'
    if labels is None:
        raise ValueError('%s: a label list is required' % what)
    out, _ = _ccl_select(ids, labels, connectivity, batched, what, mode=_lib.CCL_LARGEST, fill=_ccl_fill(fill, what))
    return out if batched else out[0]


def remove_small_components(x, min_size, connectivity=1, labels=None, fill=0, batched=False):
    """
    Drops the connected components of fewer than min_size voxels.  Without `labels`, x is a mask and the result a mask of its dtype; with
    `labels`, x is an integer id map and the result the int32 id map with the dropped voxels set to `fill` (ids outside the list pass
    through).  Arguments and limits as `connected_components`; on the device, graph-capturable, not differentiable.
    """
    what = 'remove_small_components'
    if isinstance(min_size, bool) or min_size != int(min_size) or not 0 <= int(min_size) < 2 ** 31:
        raise ValueError('%s: min_size must be an integer in [0, 2^31), got %r' % (what, min_size))
    out, _ = _ccl_select(x, labels, connectivity, batched, what, mode=_lib.CCL_MIN_SIZE, min_size=int(min_size), fill=_ccl_fill(fill, what))
    if labels is None:
        return _ccl_like(out, x, batched)
    return out if batched else out[0]


def fill_holes(mask, connectivity=1, batched=False):
    """
    scipy.ndimage.binary_fill_holes(mask, generate_binary_structure(nd, connectivity)): the mask together with every connected
    component of its complement (under that connectivity) that does not touch the border of the volume.  Returns a mask of the input's
    dtype.  Arguments and limits as `connected_components`; on the device, graph-capturable, not differentiable.
    """
    out, _ = _ccl_select(mask, None, connectivity, batched, 'fill_holes', mode=_lib.CCL_BORDER_FREE | _lib.CCL_INVERT)
    return _ccl_like(out, mask, batched)


# --------------------------------------------------------------------------------------
# percentiles and the percentile intensity normalisation (csrc/select.hip)
# --------------------------------------------------------------------------------------

_PCT_METHODS = {'linear': _lib.PCT_LINEAR, 'lower': _lib.PCT_LOWER, 'higher': _lib.PCT_HIGHER, 'midpoint': _lib.PCT_MIDPOINT}
_PCT_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
_PCT_MAX_Q = 8


def _pct_fractions(q, scale, what):
    """q (a scalar or a sequence of 1 .. 8 values in [0, scale]) -> (fractions in [0, 1] as Python floats, q was a scalar)"""
    if isinstance(q, torch.Tensor):
        raise TypeError('%s: q is read on the host: a number or a sequence of numbers, not a tensor' % what)
    scalar = np.ndim(q) == 0
    values = [q] if scalar else list(q)
    if np.ndim(q) > 1 or not values:
        raise ValueError('%s: q must be a scalar or a sequence of 1 to %d values, got %r' % (what, _PCT_MAX_Q, q))
    if len(values) > _PCT_MAX_Q:
        raise NotImplementedError('%s: up to %d percentiles in one call, got %d' % (what, _PCT_MAX_Q, len(values)))
    out = []
    for v in values:
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) <= scale:
            raise ValueError('%s: q must lie in [0, %g], got %r' % (what, scale, v))
        out.append(float(v) / 100.0 if scale == 100 else float(v))
    return out, scalar


def _pct_source(x, mask, batched, what):
    """x -> (x [B, V] contiguous, mask [B, V] uint8 or None); every check the host can make, before the device is looked at"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(x).__name__))
    x = materialize(x).detach()
    if x.dtype not in _PCT_DTYPES:
        raise NotImplementedError('%s: float32, bfloat16 or float16 tensors, got %s' % (what, x.dtype))
    if batched and x.dim() < 1:
        raise ValueError('%s: batched=True needs a batch axis, got a 0-d tensor' % what)
    if x.numel() == 0:
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(x.shape)))
    batch = int(x.shape[0]) if batched else 1
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError('%s: mask must be a torch.Tensor, got %s' % (what, type(mask).__name__))
        if mask.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError('%s: a bool or uint8 mask, got %s' % (what, mask.dtype))
        if tuple(mask.shape) != tuple(x.shape):
            raise ValueError('%s: the mask has shape %s, x has %s' % (what, tuple(mask.shape), tuple(x.shape)))
    if batch > 65535 or x.numel() >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 elements, got shape %s' % (what, tuple(x.shape)))
    _lib.require_device(x, mask)
    x = x.contiguous().view(batch, -1)
    if mask is not None:
        mask = mask.detach().contiguous().view(batch, -1)
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return x, mask


def _select_call(x, fractions, mask=None, method='linear', ignore_nan=False, what='percentile'):
    """nrt_percentile on x [B, V] -> (values, lower, upper: float32 [B, Q]; count: int32 [B]), all on the device"""
    dev = x.device
    batch, voxels, nq = int(x.shape[0]), int(x.shape[1]), len(fractions)
    nws = int(_lib.lib().nrt_select_workspace_bytes(batch, voxels, nq))
    ws = _lib.workspace(dev, max(nws, 16))
    out, lower, upper = [torch.empty((batch, nq), dtype=torch.float32, device=dev) for _ in range(3)]
    count = torch.empty((batch,), dtype=torch.int32, device=dev)
    positions = (C.c_double * nq)(*fractions)
    _lib.call(dev, 'nrt_percentile', _lib.ptr(x), _PCT_DTYPES[x.dtype], _lib.ptr(mask), batch, voxels, positions, nq,
              _PCT_METHODS[method], _lib.PCT_IGNORE_NAN if ignore_nan else 0, _lib.ptr(out), _lib.ptr(lower), _lib.ptr(upper),
              _lib.ptr(count), _lib.ptr(ws), nws, what=what)
    return out, lower, upper, count


def _percentile(x, q, scale, mask, batched, method, ignore_nan, what):
    fractions, scalar = _pct_fractions(q, scale, what)
    if method not in _PCT_METHODS:
        raise ValueError('%s: method must be one of %s, got %r' % (what, ', '.join(sorted(_PCT_METHODS)), method))
    x, mask = _pct_source(x, mask, batched, what)
    out = _select_call(x, fractions, mask, method, bool(ignore_nan), what)[0]
    out = out[:, 0] if scalar else out
    return out if batched else out[0]


def percentile(x, q, mask=None, batched=False, method='linear', ignore_nan=False):
    """
    The q-th percentiles of the elements of x (of every batch entry with batched=True): np.percentile(x.astype(float64), q, method=...)
    rounded to float32, exactly, by a radix select on the device (csrc/select.hip) -- no sort, no sorted copy, nothing
    travels to the host, so the call captures into a graph; bit-identical run to run.

    x:          float32, bfloat16 or float16, any shape; with batched=True the first axis is the batch.  Fewer than 2^31 elements,
                at most 65535 batch entries.
    q:          a number or a sequence of 1 to 8 numbers in [0, 100], read on the host.
    mask:       bool or uint8 of x's shape: the population is the selected elements.  An empty population gives NaN.
    method:     'linear' (NumPy's default: a + (b - a) t between the two bracketing order statistics, in float64), 'lower', 'higher',
                'midpoint'.
    ignore_nan: False: a NaN in the population makes the results NaN (np.percentile); True: NaNs leave the population
                (np.nanpercentile).
    Returns float32 of shape [] or [Q], with batched=True [B] or [B, Q].  Not differentiable: the result never requires grad.
    """
    return _percentile(x, q, 100, mask, batched, method, ignore_nan, 'percentile')


def quantile(x, q, mask=None, batched=False, method='linear', ignore_nan=False):
    """
    `percentile` with q in [0, 1]: q is the position itself, it is not multiplied by 100 and divided again.  On the device,
    graph-capturable, not differentiable.
    """
    return _percentile(x, q, 1, mask, batched, method, ignore_nan, 'quantile')


def median(x, mask=None, batched=False):
    """
    percentile(x, 50): the middle element, or the mean of the two middle elements (in float64, rounded to float32 once).  On the
    device, graph-capturable, not differentiable.
    """
    return _percentile(x, 50, 100, mask, batched, 'linear', False, 'median')


def percentile_norm(x, lower=0, upper=99, mask=None, clip=True, out_range=(0, 1), batched=False):
    """
    Percentile intensity normalisation: (x - lo) / (hi - lo) with lo, hi the `lower`-th and `upper`-th percentiles of x (of every batch
    entry with batched=True), both from ONE select call (lower=0 is the minimum, upper=100 the maximum), followed by one streaming
    kernel that reads the bounds on the device.  clip=True clips to [0, 1]; out_range=(a, b) other than (0, 1) maps the result to
    a + y (b - a).  Where hi == lo the result is 0 (mapped: a); where a bound is NaN (a NaN in x, an empty mask) it is NaN.
    lower=0, upper=99, clip=True is mri_synthstrip's intensity step; 0.5 / 99.5 the clipping of SynthSeg- and nnU-Net-style
    preprocessing.

    mask (bool or uint8 of x's shape) restricts where the bounds are MEASURED, not where the output is written.
    Returns float32 of x's shape.  Arguments and limits as `percentile`; on the device, graph-capturable, not differentiable.
    """
    what = 'percentile_norm'
    fractions, _ = _pct_fractions([lower, upper], 100, what)
    if fractions[0] > fractions[1]:
        raise ValueError('%s: lower must not exceed upper, got %r and %r' % (what, lower, upper))
    if np.ndim(out_range) != 1 or len(out_range) != 2 or not all(np.isfinite(float(v)) for v in out_range):
        raise ValueError('%s: out_range must be two finite numbers, got %r' % (what, out_range))
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else None
    x, mask = _pct_source(x, mask, batched, what)
    bounds = _select_call(x, fractions, mask, 'linear', False, what)[0]
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.call(x.device, 'nrt_rescale_clip_f32', _lib.ptr(x), _PCT_DTYPES[x.dtype], int(x.shape[0]), int(x.shape[1]), _lib.ptr(bounds),
              _lib.ptr(bounds[:, 1]), 2, int(bool(clip)), float(out_range[0]), float(out_range[1]), _lib.ptr(out), what=what)
    return out.view(shape)


# --------------------------------------------------------------------------------------
# per-label region statistics of an integer id map (csrc/labelstats.hip)
# --------------------------------------------------------------------------------------

_LS_MAX_CHANNELS = 4


def _ls_labels(labels, what):
    """labels (a list of distinct ids, or an int nb for the ids 0 .. nb - 1) -> (tuple of ids or None for 0 .. nb - 1, nlabels)"""
    if labels is None:
        raise ValueError('%s: give a label list, or the number of labels nb for the ids 0 .. nb - 1 (nothing is read back from the '
                         'id map to find them)' % what)
    if isinstance(labels, (bool, np.bool_)):
        raise ValueError('%s: labels must be a list of ids or their number, got %r' % (what, labels))
    if isinstance(labels, (int, np.integer)):
        ids, n = None, int(labels)
    else:
        ids = _edt_labels(labels, what)
        n = len(ids)
    if n < 1:
        raise ValueError('%s: at least one label, got %r' % (what, labels))
    if n > _EDT_MAX_LABELS:
        raise NotImplementedError('%s: 1 to %d labels, got %d' % (what, _EDT_MAX_LABELS, n))
    return ids, n


def _ls_check_geometry(shape, what, spatial_axes=(2, 3)):
    """the limits of csrc/labelstats.hip for an id map [B, *S], before the device is looked at"""
    batch, spatial = int(shape[0]), [int(v) for v in shape[1:]]
    if spatial_axes is not None and len(spatial) not in spatial_axes:
        raise NotImplementedError('%s: 2 or 3 spatial axes, got %d (shape %s)' % (what, len(spatial), tuple(shape)))
    if batch < 1 or not spatial or any(v < 1 for v in spatial):
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(shape)))
    if batch > 65535 or batch * int(np.prod(spatial, dtype=np.int64)) >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 voxels, got shape %s' % (what, tuple(shape)))


def _ls_voxel_volume(voxel_size, nd, what):
    """None, a scalar or nd voxel sizes -> the volume of a voxel as a Python float"""
    if voxel_size is None:
        return 1.0
    if isinstance(voxel_size, torch.Tensor):
        raise TypeError('%s: voxel_size is read on the host: a number or a sequence of numbers, not a tensor' % what)
    sizes = [voxel_size] * nd if np.ndim(voxel_size) == 0 else list(voxel_size)
    if np.ndim(voxel_size) > 1 or len(sizes) != nd:
        raise ValueError('%s: voxel_size must be a scalar or %d values, got %r' % (what, nd, voxel_size))
    for v in sizes:
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 < float(v) < np.inf:
            raise ValueError('%s: voxel sizes must be positive and finite, got %r' % (what, voxel_size))
    volume = 1.0
    for v in sizes:
        volume *= float(v)
    return volume


def _label_stats_call(ids, image, labels, nlabels, want_coords=True, what='label_stats'):
    """nrt_label_stats on ids [B, *S] int32 and image None or [B, *S, C], both contiguous on one device ->
    (counts [B, L] int64, coord_sums [B, L, nd] int64, bbox [B, L, 2, nd] int32, sums [B, L, C, 2] float64, minmax [B, L, C, 2]
    float32; None for what was not asked for)"""
    dev = ids.device
    batch, spatial = int(ids.shape[0]), [int(v) for v in ids.shape[1:]]
    nd = len(spatial)
    channels = 0 if image is None else int(image.shape[-1])
    cshape = _lib.ints(spatial)
    nws = int(_lib.lib().nrt_label_stats_workspace_bytes(batch, cshape, nd, nlabels, channels))
    ws = _lib.workspace(dev, max(nws, 16))
    counts = torch.empty((batch, nlabels), dtype=torch.int64, device=dev)
    coord_sums = torch.empty((batch, nlabels, nd), dtype=torch.int64, device=dev) if want_coords else None
    bbox = torch.empty((batch, nlabels, 2, nd), dtype=torch.int32, device=dev) if want_coords else None
    sums = torch.empty((batch, nlabels, channels, 2), dtype=torch.float64, device=dev) if channels else None
    minmax = torch.empty((batch, nlabels, channels, 2), dtype=torch.float32, device=dev) if channels else None
    lab = _edt_label_tensor(labels, dev) if labels is not None else None
    _lib.call(dev, 'nrt_label_stats', _lib.ptr(ids), _lib.ptr(lab), nlabels, _lib.ptr(image),
              _PCT_DTYPES[image.dtype] if channels else 0, channels, batch, cshape, nd, _lib.ptr(counts), _lib.ptr(coord_sums),
              _lib.ptr(bbox), _lib.ptr(sums), _lib.ptr(minmax), _lib.ptr(ws), nws, what=what)
    return counts, coord_sums, bbox, sums, minmax


def _label_stats_source(ids, image, labels, batched, what, voxel_size=None):
    """every check the host can make -> (ids [B, *S] int32 contiguous, image [B, *S, C] contiguous or None, label tuple or None, L,
    the volume of a voxel)"""
    labels, nlabels = _ls_labels(labels, what)
    ids = _edt_ids_checked(ids, what).detach()
    vol = ids if batched else ids.unsqueeze(0)
    if vol.dim() < 2:
        raise ValueError('%s: expected [*spatial]%s, got shape %s' % (what, ' behind a batch axis' if batched else '', tuple(ids.shape)))
    _ls_check_geometry(vol.shape, what)
    voxel = _ls_voxel_volume(voxel_size, vol.dim() - 1, what)
    if image is not None:
        if not isinstance(image, torch.Tensor):
            raise TypeError('%s: the image must be a torch.Tensor, got %s' % (what, type(image).__name__))
        image = materialize(image).detach()
        if image.dtype not in _PCT_DTYPES:
            raise NotImplementedError('%s: a float32, bfloat16 or float16 image, got %s' % (what, image.dtype))
        if tuple(image.shape) == tuple(ids.shape):
            image = image.unsqueeze(-1)                          # (no channel axis: one channel)
        if image.dim() != ids.dim() + 1 or tuple(image.shape[:-1]) != tuple(ids.shape):
            raise ValueError('%s: the image must have the id map\'s shape %s, with or without a channel axis behind it, got %s'
                             % (what, tuple(ids.shape), tuple(image.shape)))
        if not 1 <= int(image.shape[-1]) <= _LS_MAX_CHANNELS:
            raise NotImplementedError('%s: 1 to %d channels, got %d' % (what, _LS_MAX_CHANNELS, int(image.shape[-1])))
        image = image if batched else image.unsqueeze(0)
    _lib.require_device(vol, image)
    return vol.to(torch.int32).contiguous(), None if image is None else image.contiguous(), labels, nlabels, voxel


def label_stats(ids, image=None, labels=None, voxel_size=None, batched=False):
    """
    Per-label region statistics of an integer id map, and of an image under it, in one pass on the device (csrc/labelstats.hip;
    DESIGN 4.6n): what scipy.ndimage.sum / mean / center_of_mass / find_objects give label by label on the host.  No one-hot tensor
    exists, no float atomics are used (the float sums have a fixed partition and order: bit-identical run to run) and nothing travels
    to the host, so the call captures into a graph.

    ids:        an integer (or bool) id map [*S], or [B, *S] with batched=True; len(S) in {2, 3}, B * prod(S) < 2^31.
    image:      None, or float32 / bfloat16 / float16 of ids' shape (one channel) or of ids' shape + [C], 1 <= C <= 4.
    labels:     1 to 256 distinct ids of any int32 value, in any order: slot l collects the voxels with ids == labels[l]; or an int nb
                for the ids 0 .. nb - 1.  Other ids belong to no slot.  Required: the id map is not read back to find its ids.
    voxel_size: None (1), a scalar, or len(S) voxel sizes, read on the host.
    Returns a dict of device tensors (without batched=True the leading B axis is dropped):
      count [B, L] int64;  volume [B, L] float64 = count * prod(voxel_size);  centroid [B, L, nd] float64 in voxel coordinates ('ij';
      coord_sum / count, NaN for an empty label);  coord_sum [B, L, nd] int64;  bbox_min, bbox_max [B, L, nd] int32, both inclusive (an
      empty label holds shape and -1);
      with an image  sum, sumsq [B, L, C] float64;  mean = sum / n;  std = sqrt(max(0, sumsq / n - mean^2)) (the population std), both
      float64 and NaN where n == 0;  min, max [B, L, C] float32 (a NaN is skipped; an empty or all-NaN label holds +inf, -inf).
    The integers are exact.  sum is within (n + 2) 2^-24 sum|x| of the exact sum of the stored values, sumsq within (n + 3) 2^-24 sum x^2.
    Not differentiable: the results never require grad.
    """
    what = 'label_stats'
    vol, image, labels, nlabels, voxel = _label_stats_source(ids, image, labels, batched, what, voxel_size)
    counts, coord_sums, bbox, sums, minmax = _label_stats_call(vol, image, labels, nlabels, what=what)
    n = counts.to(torch.float64)
    out = {'count': counts, 'volume': n * voxel, 'centroid': coord_sums.to(torch.float64) / n.unsqueeze(-1), 'coord_sum': coord_sums,
           'bbox_min': bbox[:, :, 0], 'bbox_max': bbox[:, :, 1]}
    if image is not None:
        total, squares = sums[..., 0], sums[..., 1]
        mean = total / n.unsqueeze(-1)
        var = squares / n.unsqueeze(-1) - mean * mean
        out.update(sum=total, sumsq=squares, mean=mean, std=var.clamp_min(0.0).sqrt(), min=minmax[..., 0], max=minmax[..., 1])
    return out if batched else {k: v[0] for k, v in out.items()}


def label_volumes(ids, labels, voxel_size=None, batched=False):
    """
    The volume of every listed label of an integer id map: `label_stats(...)['volume']`, float64 [L] ([B, L] with batched=True), the
    voxel count times prod(voxel_size).  Arguments and limits as `label_stats`; on the device, graph-capturable, not differentiable.
    """
    what = 'label_volumes'
    vol, _, labels, nlabels, voxel = _label_stats_source(ids, None, labels, batched, what, voxel_size)
    out = _label_stats_call(vol, None, labels, nlabels, want_coords=False, what=what)[0].to(torch.float64) * voxel
    return out if batched else out[0]


def label_centroids(ids, labels, batched=False):
    """
    The centroid of every listed label of an integer id map in voxel coordinates ('ij'): `label_stats(...)['centroid']`, float64
    [L, nd] ([B, L, nd] with batched=True), NaN for a label that does not occur.  Arguments and limits as `label_stats`; on the device,
    graph-capturable, not differentiable.
    """
    what = 'label_centroids'
    vol, _, labels, nlabels, _ = _label_stats_source(ids, None, labels, batched, what)
    counts, coord_sums = _label_stats_call(vol, None, labels, nlabels, what=what)[:2]
    out = coord_sums.to(torch.float64) / counts.to(torch.float64).unsqueeze(-1)
    return out if batched else out[0]


# --------------------------------------------------------------------------------------
# index / grid helpers (host-side; the kernels never need the materialised grids)
# --------------------------------------------------------------------------------------

def volshape_to_ndgrid(volshape, **kwargs):
    """neurite/tf/utils/utils.py:333-353."""
    if not all(float(d).is_integer() for d in volshape):
        raise ValueError("volshape needs to be a list of integers")
    linvec = [torch.arange(0, int(d), dtype=torch.int32) for d in volshape]
    return ndgrid(*linvec, **kwargs)


def volshape_to_meshgrid(volshape, **kwargs):
    """neurite/tf/utils/utils.py:356-379 ('xy' default like tf.meshgrid)."""
    if not all(float(d).is_integer() for d in volshape):
        raise ValueError("volshape needs to be a list of integers")
    linvec = [torch.arange(0, int(d), dtype=torch.int32) for d in volshape]
    return meshgrid(*linvec, **kwargs)


def ndgrid(*args, **kwargs):
    """neurite/tf/utils/utils.py:382-395."""
    return meshgrid(*args, indexing='ij', **kwargs)


def meshgrid(*args, **kwargs):
    """neurite/tf/utils/utils.py:398-476."""
    indexing = kwargs.pop("indexing", "xy")
    kwargs.pop("name", None)
    if kwargs:
        key = list(kwargs.keys())[0]
        raise TypeError("'{}' is an invalid keyword argument for this function".format(key))
    if indexing not in ("xy", "ij"):
        raise ValueError("indexing parameter must be either 'xy' or 'ij'")
    args = [torch.as_tensor(a) for a in args]
    return [g.contiguous() for g in torch.meshgrid(*args, indexing=indexing)]


def sub2ind2d(siz, subs, **kwargs):
    """neurite/tf/utils/utils.py:1068-1082 (row-major flat index)."""
    assert len(siz) == len(subs), 'found inconsistent siz and subs: %d %d' % (len(siz), len(subs))
    k = np.cumprod(list(siz)[::-1])
    ndx = subs[-1]
    for i, v in enumerate(list(subs[:-1])[::-1]):
        ndx = ndx + v * int(k[i])
    return ndx


def prod_n(lst):
    """neurite/tf/utils/utils.py:1085-1092."""
    prod = lst[0]
    for p in lst[1:]:
        prod = prod * p
    return prod


def batch_channel_flatten(x):
    """neurite/tf/utils/utils.py:1175-1188: [B, ..., C] -> [B, V, C] (a view, never a copy)."""
    return flatten_axes(x, range(1, x.dim() - 1))


flatten_batch_channel = batch_channel_flatten


def flatten_axes(x, axes):
    """neurite/tf/utils/utils.py:1195-1226."""
    assert isinstance(axes, (list, tuple, range)), 'axes must be list or tuple of axes to be flattened'
    assert np.all(np.diff(axes) == 1), 'axes need to be contiguous'
    if axes[0] < 0:
        assert axes[-1] < 0, 'if one axis is negative, all have to be negative'
    assert axes[-1] < x.dim(), 'axis %d outside max axis %d' % (axes[-1], x.dim() - 1)
    shp = list(x.shape)
    new = shp[:axes[0]] + [-1]
    if axes[-1] < x.dim() - 1 and not (axes[-1] == -1):
        new += shp[axes[-1] + 1:]
    return x.reshape(new)


# --------------------------------------------------------------------------------------
# affine sampling helpers of voxelmorph that neurite's labels_to_image_new instantiates (neurite/tf/models.py:1068-1112:
# vxm.layers.DrawAffineParams, ParamsToAffineMatrix, vxm.utils.draw_flip_matrix / draw_swap_matrix).  voxelmorph is not
# vendored in the reference tree; these follow its published interface.  Host-side: a handful of numbers per batch entry.
# --------------------------------------------------------------------------------------

def _host_generator(seed):
    g = torch.Generator(device='cpu')
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed) % (2 ** 63 - 1))
    return g


def draw_affine_params(shift=None, rot=None, scale=None, shear=None, normal_shift=False, normal_rot=False,
                       normal_scale=False, normal_shear=False, shift_scale=False, ndims=3, batch_shape=None, concat=True,
                       dtype=torch.float32, seeds={}):
    """
    Draw translation, rotation, scaling and shearing parameters: uniformly in [-bound, bound] or, with normal_*, normally
    with the bound as SD (scaling: truncated at two SDs).  Returns [*batch_shape, M] with M = 12 (3-D) or 6 (2-D), ordered
    shift, rot, scale, shear; scaling parameters are deviations from 1 unless shift_scale.
    """
    assert ndims in (2, 3), 'only 2D and 3D supported'
    splits = dict(shift=ndims, rot=3 if ndims == 3 else 1, scale=ndims, shear=3 if ndims == 3 else 1)
    bounds = dict(shift=shift, rot=rot, scale=scale, shear=shear)
    normal = dict(shift=normal_shift, rot=normal_rot, scale=normal_scale, shear=normal_shear)
    batch_shape = [] if batch_shape is None else [int(b) for b in np.ravel(batch_shape)]
    par = {}
    for key, n in splits.items():
        lim = np.ravel(0 if bounds[key] is None else bounds[key]).astype(np.float64)
        if lim.size == 1:
            lim = np.repeat(lim, n)
        assert lim.size == n, f'unexpected number of {key} bounds {lim.size}, expected 1 or {n}'
        lim = torch.as_tensor(lim, dtype=torch.float64)
        gen = _host_generator(seeds.get(key) if isinstance(seeds, dict) else None)
        shp = batch_shape + [n]
        if normal[key]:
            draw = torch.randn(shp, generator=gen, dtype=torch.float64)
            if key == 'scale':                                  # tf.random.truncated_normal: re-draw beyond two SDs
                for _ in range(64):
                    bad = draw.abs() > 2
                    if not bool(bad.any()):
                        break
                    draw = torch.where(bad, torch.randn(shp, generator=gen, dtype=torch.float64), draw)
                draw = draw.clamp(-2, 2)
            draw = draw * lim
        else:
            draw = (torch.rand(shp, generator=gen, dtype=torch.float64) * 2 - 1) * lim
        par[key] = draw.to(dtype)
    if shift_scale:
        par['scale'] = par['scale'] + 1
    return torch.cat(list(par.values()), -1) if concat else par


def angles_to_rotation_matrix(ang, deg=True, ndims=3):
    """Rotation matrices [..., N, N] from angles [..., 1] (2-D) or [..., 3] (3-D, intrinsic R = Rx @ Ry @ Rz)."""
    assert ndims in (2, 3), 'only 2D and 3D supported'
    ang = torch.as_tensor(ang)
    if ang.dim() == 0:
        ang = ang.reshape(1)
    n = 1 if ndims == 2 else 3
    if ang.shape[-1] < n:
        ang = torch.cat([ang, ang.new_zeros(ang.shape[:-1] + (n - ang.shape[-1],))], -1)
    ang = ang[..., :n]
    if deg:
        ang = ang * (np.pi / 180)
    c, s = torch.cos(ang), torch.sin(ang)
    one, zero = torch.ones_like(c[..., 0]), torch.zeros_like(c[..., 0])

    def mat(rows):
        return torch.stack([torch.stack(r, -1) for r in rows], -2)
    if ndims == 2:
        return mat([[c[..., 0], -s[..., 0]], [s[..., 0], c[..., 0]]])
    rx = mat([[one, zero, zero], [zero, c[..., 0], -s[..., 0]], [zero, s[..., 0], c[..., 0]]])
    ry = mat([[c[..., 1], zero, s[..., 1]], [zero, one, zero], [-s[..., 1], zero, c[..., 1]]])
    rz = mat([[c[..., 2], -s[..., 2], zero], [s[..., 2], c[..., 2], zero], [zero, zero, one]])
    return rx @ ry @ rz


def params_to_affine_matrix(par, deg=True, shift_scale=False, last_row=False, ndims=3):
    """
    Affine matrices [..., N, N+1] (N+1 rows with last_row) from parameter vectors ordered shift, rot, scale, shear
    (missing trailing parameters are neutral): T @ R @ diag(scale) @ shear with an upper-triangular shear matrix.
    """
    assert ndims in (2, 3), 'only 2D and 3D supported'
    par = torch.as_tensor(par)
    if not par.dtype.is_floating_point:
        par = par.to(torch.float32)
    nrot = 3 if ndims == 3 else 1
    widths = (ndims, nrot, ndims, nrot)
    total = sum(widths)
    if par.shape[-1] > total:
        raise ValueError(f'number of params exceeds value {total} expected for dimensionality')
    if par.shape[-1] < total:
        pad = par.new_zeros(par.shape[:-1] + (total - par.shape[-1],))
        if par.shape[-1] <= ndims + nrot and not shift_scale:      # scaling parameters were not given at all: neutral = 1
            pad[..., ndims + nrot - par.shape[-1]:2 * ndims + nrot - par.shape[-1]] = 1
        par = torch.cat([par, pad], -1)
    shift, rot, scale, shear = torch.split(par, widths, -1)
    if shift_scale:
        scale = scale + 1
    m_rot = angles_to_rotation_matrix(rot, deg=deg, ndims=ndims)
    m_scale = torch.diag_embed(scale)
    m_shear = torch.eye(ndims, dtype=par.dtype, device=par.device).expand(par.shape[:-1] + (ndims, ndims)).clone()
    iu = np.triu_indices(ndims, k=1)
    for k, (i, j) in enumerate(zip(*iu)):
        m_shear[..., i, j] = shear[..., k]
    out = torch.cat([m_rot @ m_scale @ m_shear, shift[..., None]], -1)
    if last_row:
        row = out.new_zeros(out.shape[:-2] + (1, ndims + 1))
        row[..., -1] = 1
        out = torch.cat([out, row], -2)
    return out


def draw_flip_matrix(grid_shape, shift_center=True, last_row=True, dtype=torch.float32, seed=None):
    """Matrix that flips each axis of an N-D grid with probability 1/2 (about the grid centre unless shift_center)."""
    ndims = len(grid_shape)
    bit = (torch.randn(ndims, generator=_host_generator(seed)) > 0).to(dtype)
    out = torch.zeros(ndims, ndims + 1, dtype=dtype)
    out[:, :ndims] = torch.diag(1 - 2 * bit)
    if not shift_center:
        out[:, -1] = (torch.as_tensor(np.asarray(grid_shape), dtype=dtype) - 1) * bit
    if last_row:
        out = torch.cat([out, torch.tensor([[0.] * ndims + [1.]], dtype=dtype)], 0)
    return out


def draw_swap_matrix(ndims, last_row=True, dtype=torch.float32, seed=None):
    """Matrix that randomly permutes the axes of N-D space."""
    perm = torch.randperm(ndims, generator=_host_generator(seed))
    out = torch.zeros(ndims, ndims + 1, dtype=dtype)
    out[torch.arange(ndims), perm] = 1
    if last_row:
        out = torch.cat([out, torch.tensor([[0.] * ndims + [1.]], dtype=dtype)], 0)
    return out


def _axis_gather_launch(x, index, ax):
    dev = x.device
    idx = torch.as_tensor(np.asarray(index, dtype=np.int32)).to(dev)
    outer = int(np.prod(x.shape[:ax])) if ax else 1
    inner = int(np.prod(x.shape[ax + 1:]))
    y = torch.empty(tuple(x.shape[:ax]) + (idx.numel(),) + tuple(x.shape[ax + 1:]), dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_synth_axis_gather_f32', _lib.ptr(x), _lib.ptr(idx), _lib.ptr(y), outer, x.shape[ax], idx.numel(), inner)
    return y


class _AxisGatherFn(torch.autograd.Function):
    """tf.gather along one axis by a non-decreasing host-built index list; the gradient is a segmented sum (csrc/synth.hip)."""

    @staticmethod
    def forward(ctx, x, index, ax):
        index = np.asarray(index, dtype=np.int32)
        assert (np.diff(index) >= 0).all(), 'the index list must be non-decreasing'
        ctx.geom = (tuple(x.shape), ax, index)
        return _axis_gather_launch(x, index, ax)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        shape, ax, index = ctx.geom
        dev = grad_y.device
        g = grad_y.contiguous()
        if g.dtype != torch.float32:
            raise NotImplementedError('subsample_axis backward: float32 gradients, got %s' % g.dtype)
        run_start = np.searchsorted(index, np.arange(shape[ax] + 1), side='left').astype(np.int32)
        runs = torch.as_tensor(run_start).to(dev)
        outer = int(np.prod(shape[:ax])) if ax else 1
        inner = int(np.prod(shape[ax + 1:]))
        gx = torch.empty(shape, dtype=torch.float32, device=dev)
        if gx.numel():
            _lib.call(dev, 'nrt_synth_axis_gather_bwd_f32', _lib.ptr(g), _lib.ptr(runs), _lib.ptr(gx), outer, shape[ax], index.size, inner)
        return gx, None, None


def _axis_gather(x, index, ax):
    """y = tf.gather(x, index, axis=ax) of a float32 device tensor (csrc/synth.hip); recorded for autograd when x requires grad"""
    _lib.require_device(x)
    x = x.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _AxisGatherFn.apply(x, index, ax)
    return _axis_gather_launch(x, index, ax)


def subsample_axis_indices(width, thick):
    """index lists of utils.subsample_axis (utils.py:815-824): slices kept, and the map back to `width` samples"""
    num_slice = int(np.float32(width) / np.float32(thick) + np.float32(0.5))
    # tf.linspace re-casts integer end points to the dtype of its step, float64: the indices are truncations of doubles
    down = (np.linspace(0, width - 1, num_slice, dtype=np.float64) + 0.5).astype(np.int32)
    up = (np.linspace(0, num_slice - 1, width, dtype=np.float64) + 0.5).astype(np.int32)
    return down, up


def _subsample_draws(num_axes, stride_min, stride_max, prob, seed, draws=None):
    """(index into the axis list, slice thickness) of utils.subsample_axis (utils.py:801-813), in the reference's order of
    draws; `draws` (tests): uniform [0, 1) numbers to use instead of the generator's"""
    gen = _host_generator(seed)
    draws = None if draws is None else list(draws)

    def uniform():
        return np.float32(draws.pop(0)) if draws is not None else np.float32(float(torch.rand((), generator=gen)))
    ax = int(np.floor(np.float64(uniform()) * num_axes))
    thick = uniform() * np.float32(np.float32(stride_max) - np.float32(stride_min)) + np.float32(stride_min)
    assert 0 <= prob <= 1, f'{prob} not a probability'
    if prob < 1:
        bit = np.float32(uniform() < np.float32(prob))
        thick = thick * bit + (np.float32(1) - bit)
    return ax, thick


def subsample_axis(x, stride_min=1, stride_max=8, axes=None, prob=1, upsample=True, seed=None, _draws=None):
    """
    Symmetrically subsample a tensor by a random factor (stride) along one randomly drawn axis with nearest-neighbour
    interpolation and optionally up-sample it again (utils.py:754-826).  float32 device tensors.  Differentiable (once) with
    respect to x.
    """
    if x.dtype != torch.float32:
        raise NotImplementedError('subsample_axis: float32 tensors, got %s' % x.dtype)
    num_dim = x.dim()
    if axes is None:
        axes = range(num_dim)
    if np.isscalar(axes):
        axes = [axes]
    axes = list(axes)
    assert all(i in range(num_dim) for i in axes), 'invalid axis passed'
    assert 0 < stride_min and stride_min <= stride_max, 'invalid strides'
    ax, thick = _subsample_draws(len(axes), stride_min, stride_max, prob, seed, _draws)
    ax = axes[ax]
    width = x.shape[ax]
    down, up = subsample_axis_indices(width, thick)
    if upsample:
        return _axis_gather(x, down[up], ax)                 # the two gathers of the reference composed into one
    return _axis_gather(x, down, ax)
