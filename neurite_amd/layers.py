"""
neurite_amd.layers -- the layers of neurite's hot path as torch.nn.Modules over the HIP kernels.

Resize / Zoom           neurite/tf/layers.py:91-185
SpatialTransformer      voxelmorph.layers.SpatialTransformer as the reference calls it
                        (neurite/tf/models.py:806-807 and 1157-1159; not vendored in the reference)
LabelTransformer, LabelResize   the two above for integer label maps: linear interpolation + arg-max without a one-hot tensor
                        (an extension of this package; fused.warp_labels)
HyperConv* / HyperDense* neurite/tf/layers.py:2515-3033 (kernel and bias are inputs, one set per batch entry)
LocalBias, LocalLinear  neurite/tf/layers.py:746-808   (one bias / one linear map per voxel and feature)
LocalCrossLinear        :1535-1607                     (one Cin x Cout matrix per voxel; up to 64 features each way)
LocalParamLayer         :1711-1789                     (a learnable tensor without inputs; takes device= or .to())
LocalParamWithInput     :1792-1844                     (the same tensor once per batch entry of an otherwise ignored input)
MeanStream, CovStream   :1915-2073                     (running mean / covariance; `count` never leaves the device)
SampleNormalLogVar      :2261-2302                     (z = mu + exp(log_var / 2) * noise, the sampling step of models.single_ae)

The local and stream layers are float32 only (NotImplementedError otherwise, raised before any device is touched), know the
initializers 'RandomNormal', 'glorot_uniform' and 'zeros', refuse regularizers, and CovStream has no gradient.  The free function
LocalParam (:1847) is not provided: a bare tensor cannot own a registered parameter in torch -- use LocalParamLayer.

Same constructor arguments, defaults, lazy build on first call, get_config() keys and error
behaviour as the Keras layers.  Tensors are channels-last [B, *spatial, C] on a ROCm device.
The batch loop the reference runs serially with tf.map_fn (layers.py:171) is one batched kernel
launch here (blockIdx.y = batch entry).
"""

import numpy as np
import torch
from torch import nn

from . import _lib
from . import augment
from . import deferred
from . import utils

__all__ = ['Resize', 'Zoom', 'SpatialTransformer', 'LabelTransformer', 'LabelResize', 'LocallyConnected3D', 'VecInt', 'RescaleTransform',
           'ComposeTransform', 'AffineToDenseShift', 'GaussianBlur', 'Subsample', 'RandomCrop', 'GaussianNoise', 'PerlinNoise',
           'HyperConv', 'HyperConv2D', 'HyperConv3D', 'HyperConvFromDense', 'HyperConv2DFromDense', 'HyperConv3DFromDense',
           'HyperDense', 'HyperDenseFromDense', 'LocalBias', 'LocalLinear', 'LocalCrossLinear', 'LocalParamLayer',
           'LocalParamWithInput', 'MeanStream', 'CovStream', 'SampleNormalLogVar', 'Negate', 'RescaleValues']


class _Layer(nn.Module):
    """The slice of the Keras Layer protocol the reference's users touch."""

    def __init__(self, name=None, **kwargs):
        super().__init__()
        kwargs.pop('dtype', None)
        kwargs.pop('trainable', None)
        kwargs.pop('input_shape', None)
        if kwargs:
            raise TypeError('unexpected keyword arguments: %s' % sorted(kwargs))
        self._name = name or self.__class__.__name__.lower()
        self.built = False

    @property
    def name(self):
        return self._name

    def build(self, input_shape):
        self.built = True

    def get_config(self):
        return {'name': self._name}

    def _maybe_build(self, inputs):
        if not self.built:
            first = inputs[0] if isinstance(inputs, (list, tuple)) else inputs
            self._build_device, self._build_dtype = first.device, first.dtype    # weights are created where the data lives
            if isinstance(inputs, (list, tuple)):
                self.build([tuple(i.shape) for i in inputs])
            else:
                self.build(tuple(inputs.shape))
            self.built = True

    def forward(self, inputs, **kwargs):
        self._maybe_build(inputs)
        return self.call(inputs, **kwargs)


class Negate(_Layer):
    """The negative of the input (neurite/tf/layers.py:49-64); forward and gradient on the element-wise kernel."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    def compute_output_shape(self, input_shape):
        return input_shape

    def call(self, x):
        from .models import _scale_values
        if x.dtype != torch.float32:                  # refused before the device is looked at
            raise NotImplementedError('%s runs on the float32 element-wise kernel, got %s' % (self.__class__.__name__, x.dtype))
        _lib.require_device(x)
        return _scale_values(x, -1.0)


class RescaleValues(_Layer):
    """Rescale data values (e.g. intensities) by a fixed factor (neurite/tf/layers.py:67-88); forward and gradient on the
    element-wise kernel."""

    def __init__(self, resize, **kwargs):
        self.resize = resize
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'resize': self.resize})
        return config

    def compute_output_shape(self, input_shape):
        return input_shape

    def call(self, x):
        from .models import _scale_values
        if x.dtype != torch.float32:                  # refused before the device is looked at
            raise NotImplementedError('%s runs on the float32 element-wise kernel, got %s' % (self.__class__.__name__, x.dtype))
        _lib.require_device(x)
        return _scale_values(x, self.resize)


class Resize(_Layer):
    """
    N-D resize layer (neurite/tf/layers.py:91-181): align-corners linear (or nearest) zoom of
    every batch entry, e.g. the 2x deformation-field upsample at neurite/tf/models.py:804.
    """

    def __init__(self, zoom_factor, interp_method='linear', **kwargs):
        super().__init__(**kwargs)
        self.zoom_factor = zoom_factor
        self.interp_method = interp_method
        self.ndims = None
        self.inshape = None

    def get_config(self):
        config = super().get_config().copy()
        config.update({'zoom_factor': self.zoom_factor, 'interp_method': self.interp_method})
        return config

    def build(self, input_shape):
        if isinstance(input_shape[0], (list, tuple)) and len(input_shape) > 1:       # layers.py:133-134
            raise Exception('Resize must be called on a list of length 1.')
        if isinstance(input_shape[0], (list, tuple)):
            input_shape = input_shape[0]
        self.ndims = len(input_shape) - 2                                             # :140
        self.inshape = input_shape
        if not isinstance(self.zoom_factor, (list, tuple)):                           # :142-147
            self.zoom_factor = [self.zoom_factor] * self.ndims
        else:
            assert len(self.zoom_factor) == self.ndims, \
                'zoom factor length {} does not match number of dimensions {}'.format(
                    len(self.zoom_factor), self.ndims)
        self.built = True

    def compute_output_shape(self, input_shape):
        output_shape = [input_shape[0]]
        output_shape += [int(input_shape[1:-1][f] * self.zoom_factor[f]) for f in range(self.ndims)]
        output_shape += [input_shape[-1]]
        return tuple(output_shape)

    def call(self, inputs):
        if isinstance(inputs, (list, tuple)):                                         # :161-165
            assert len(inputs) == 1, "inputs has to be len 1. found: %d" % len(inputs)
            vol = inputs[0]
        else:
            vol = inputs
        _lib.require_device(vol)
        vol = vol.reshape([-1, *self.inshape[1:]])                                    # :168
        zf = list(self.zoom_factor)
        if all(z == 1 for z in zf):                                                   # utils.py:250-251
            return vol
        if self.interp_method != 'linear':
            assert self.interp_method == 'nearest', \
                'method should be linear or nearest, got: %s' % self.interp_method
        new_shape = utils._new_shape(list(vol.shape[1:-1]), zf)
        vol32, restore = utils._prepare_vol(vol, self.interp_method)

        out = utils._interp_op(vol32, None, new_shape, _lib.LOC_LINSPACE, utils._METHODS[self.interp_method],
                               None, batched=True)
        return out if restore is None else out.to(restore)


Zoom = Resize


class SpatialTransformer(_Layer):
    """
    N-D spatial transformer: out[b, x, :] = interpn(vol[b], x + trf[b, x, :]) (pull-back warp with a
    dense displacement field in voxel units), or an affine [B, D, D+1]: warped in one kernel
    (fused.affine_warp) or first converted to a dense shift, the same bits either way.  Accepts
    the union of voxelmorph's historical constructor arguments.

    call([vol, trf]):  vol [B, *S, C], trf [B, *S', D]  ->  [B, *S', C]
    """

    def __init__(self, interp_method='linear', indexing='ij', single_transform=False, fill_value=None,
                 shift_center=True, add_identity=True, shape=None, **kwargs):
        super().__init__(**kwargs)
        self.interp_method = interp_method
        assert indexing in ['ij', 'xy'], "indexing has to be 'ij' (matrix) or 'xy' (cartesian)"
        self.indexing = indexing
        self.single_transform = single_transform
        self.fill_value = fill_value
        self.shift_center = shift_center
        self.add_identity = add_identity
        self.shape = shape
        self.ndims = None
        self._variant, self._tune = 0, 0      # kernel selection override (tuning / tests); 0 = auto

    def get_config(self):
        config = super().get_config().copy()
        config.update({
            'interp_method': self.interp_method,
            'indexing': self.indexing,
            'single_transform': self.single_transform,
            'fill_value': self.fill_value,
            'shift_center': self.shift_center,
            'add_identity': self.add_identity,
            'shape': self.shape,
        })
        return config

    def build(self, input_shape):
        if len(input_shape) > 2:
            raise Exception('Spatial Transformer must be called on a list of length 2.')
        self.ndims = len(input_shape[0]) - 2
        self.built = True

    def _defers(self, vol, D, trf_requires_grad, inference):
        """Is the warp of non-empty tensors deferred for the fused Dice kernel (see call)?"""
        L = vol.shape[-1]
        return (deferred.is_enabled() and self.interp_method == 'linear' and D == 3 and vol.dtype == torch.float32
                and self._variant == 0 and self._tune == 0 and L % 4 == 0 and 4 <= L <= 256
                and not (torch.is_grad_enabled() and (vol.requires_grad or trf_requires_grad))
                # inference tensors carry no version counter: an in-place change could not be detected, so they warp eagerly
                and not (inference or torch.is_inference_mode_enabled()))

    def call(self, inputs):
        assert len(inputs) == 2, 'inputs has to be len 2, found: %d' % len(inputs)
        vol, trf = inputs
        _lib.require_device(vol, trf)
        D = vol.dim() - 2
        if D < 1 or D > 3:
            raise NotImplementedError('SpatialTransformer supports 1-, 2- and 3-D volumes')
        if self.interp_method != 'linear':
            assert self.interp_method == 'nearest', \
                'method should be linear or nearest, got: %s' % self.interp_method
        if not self.add_identity:
            raise NotImplementedError('add_identity=False (absolute coordinates): call utils.interpn directly')
        B = vol.shape[0]

        # affine [B, D, D+1] or [B, D+1, D+1] -> dense shift (a dense 1-D flow [B, X, 1] also has rank 3)
        if trf.dim() == 3 and trf.shape[-1] == D + 1 and trf.shape[-2] in (D, D + 1):
            out_spatial = list(self.shape) if self.shape is not None else list(vol.shape[1:-1])
            nb = 1 if self.single_transform else trf.shape[0]
            # one kernel, no dense field (fused.affine_warp, csrc/affine_warp.hip; the same bits), unless the warp is to be deferred for
            # the fused Dice kernel below, which consumes the field.  A linear 3-D warp of 32, 64 or 128 channels whose matrix needs no
            # gradient keeps the field as well: there the wave-cache and tile kernels of csrc/interpn.hip outrun the plain gather by
            # more than the field costs (4 x 160^3: 0.967 against 1.302 ms at 32 channels, 2.473 against 2.771 at 64, 5.149 against 5.941
            # at 128; at 256 the single kernel wins again, 5.115 against 6.021 for 2 x 160^3; tools/affine_warp_bench.py).  With a
            # gradient the single kernel and its reduction win tenfold at 32 channels.
            C = vol.shape[-1]
            needs_grad = torch.is_grad_enabled() and trf.requires_grad
            wide = D == 3 and self.interp_method == 'linear' and C in (32, 64, 128) and not needs_grad
            if (self.indexing == 'ij' and D in (2, 3) and vol.dtype == torch.float32 and trf.is_floating_point() and not wide
                    and self._variant == 0 and self._tune == 0 and vol.numel() > 0 and int(np.prod(out_spatial)) > 0
                    and (self.single_transform or trf.shape[0] == B)
                    and not self._defers(vol, D, needs_grad, vol.is_inference())):
                from . import fused
                return fused.affine_warp(vol, trf.to(torch.float32), shape=out_spatial, interp_method=self.interp_method,
                                         fill_value=self.fill_value, shift_center=self.shift_center,
                                         single_transform=self.single_transform)
            trf = utils.affine_to_dense_shift(trf[:nb].to(vol.device), out_spatial, shift_center=self.shift_center,
                                              indexing=self.indexing)                      # batched: one launch on the device
        else:
            if trf.dim() != D + 2 or trf.shape[-1] != D:
                raise Exception("Number of loc Tensors %d does not match volume dimension %d"
                                % (trf.shape[-1], D))
            trf = trf.to(torch.float32)
            if self.indexing == 'xy' and D > 1:
                # cartesian flows carry (x, y, ...) = (col, row, ...): swap the first two components
                trf = torch.cat([trf[..., 1:2], trf[..., 0:1], trf[..., 2:]], -1)
        if not self.single_transform and trf.shape[0] != B:
            raise ValueError('batch size of the transform (%d) does not match the volume (%d)'
                             % (trf.shape[0], B))
        shift = trf[:1] if self.single_transform else trf
        vol32, restore = utils._prepare_vol(vol, self.interp_method)

        def run():
            out = utils._interp_op(vol32, shift, shift.shape[1:-1], _lib.LOC_SHIFT,
                                   utils._METHODS[self.interp_method], self.fill_value, batched=True,
                                   single_transform=self.single_transform, variant=self._variant, tune=self._tune)
            return out if restore is None else out.to(restore)

        # SpatialTransformer -> Dice is the metric pipeline (models.py:806-807 + metrics.py:415-482): when nothing needs a
        # gradient the warp is deferred so that Dice can run the fused kernel and `warped` is never written
        # (neurite_amd/deferred.py); any other use of the result evaluates it with the stand-alone kernel, bit-identically
        L = vol.shape[-1]
        if (shift.numel() > 0 and vol.numel() > 0
                and self._defers(vol, D, shift.requires_grad, vol32.is_inference() or shift.is_inference())):
            vol_c, shift_c = vol32.contiguous(), shift.contiguous()
            return deferred.DeferredWarp([B] + list(shift.shape[1:-1]) + [L], vol.dtype, vol.device, run,
                                         dict(vol=vol_c, shift=shift_c, single_transform=self.single_transform,
                                              fill_value=self.fill_value))
        return run()


class LabelTransformer(_Layer):
    """
    SpatialTransformer for integer label maps: linear interpolation of the (never built) one-hot map + arg-max, in one kernel
    (fused.warp_labels, csrc/warp_argmax.hip).  An extension of this package.

    call([ids, trf]):  ids [B, *S] (or [B, *S, 1]) of any integer dtype, trf a dense field [B, *S', D] or an affine [B, 3, 4] / [B, 4, 4]
    ->  ids [B, *S'] in the dtype of the input (with the trailing axis of 1 if the input had it).  nb_labels=None: every int32 value is a
    label; nb_labels=L: ids outside [0, L) are background.  fill_label: None clamps the edge, an id marks what is sampled outside the
    volume.  No gradient flows through it.
    """

    def __init__(self, nb_labels=None, indexing='ij', single_transform=False, fill_label=None, shift_center=True, **kwargs):
        super().__init__(**kwargs)
        assert indexing in ['ij', 'xy'], "indexing has to be 'ij' (matrix) or 'xy' (cartesian)"
        self.nb_labels = nb_labels
        self.indexing = indexing
        self.single_transform = single_transform
        self.fill_label = fill_label
        self.shift_center = shift_center

    def get_config(self):
        config = super().get_config().copy()
        config.update({'nb_labels': self.nb_labels, 'indexing': self.indexing, 'single_transform': self.single_transform,
                       'fill_label': self.fill_label, 'shift_center': self.shift_center})
        return config

    def build(self, input_shape):
        if len(input_shape) > 2:
            raise Exception('LabelTransformer must be called on a list of length 2.')
        self.built = True

    def call(self, inputs):
        assert len(inputs) == 2, 'inputs has to be len 2, found: %d' % len(inputs)
        ids, trf = inputs
        from . import fused
        out = fused.warp_labels(ids, trf, nb_labels=self.nb_labels, indexing=self.indexing, single_transform=self.single_transform,
                                fill_label=self.fill_label, shift_center=self.shift_center)
        return out.unsqueeze(-1) if ids.dim() == out.dim() + 1 else out


class LabelResize(_Layer):
    """
    Resize for integer label maps: the align-corners linear zoom of the (never built) one-hot map + arg-max, in one kernel
    (utils.resize_labels on every batch entry in one launch).  An extension of this package.

    call(ids):  ids [B, *S] (or [B, *S, 1]), 2-D or 3-D, of any integer dtype  ->  [B, *S'] with S' = int(S * zoom_factor), same dtype.
    zoom_factor: a scalar or one factor per spatial axis.
    """

    def __init__(self, zoom_factor, nb_labels=None, **kwargs):
        super().__init__(**kwargs)
        self.zoom_factor = zoom_factor
        self.nb_labels = nb_labels

    def get_config(self):
        config = super().get_config().copy()
        config.update({'zoom_factor': self.zoom_factor, 'nb_labels': self.nb_labels})
        return config

    def call(self, inputs):
        if isinstance(inputs, (list, tuple)):
            assert len(inputs) == 1, "inputs has to be len 1. found: %d" % len(inputs)
            inputs = inputs[0]
        from . import fused
        if not isinstance(inputs, torch.Tensor):
            raise TypeError('LabelResize: expected a torch.Tensor, got %s' % type(inputs).__name__)
        zf = self.zoom_factor
        if isinstance(zf, (list, tuple)):
            nd = len(zf)
        else:                                       # [B, X, Y] is 2-D, [B, X, Y, Z] 3-D, a fifth axis the trailing 1
            nd = min(inputs.dim() - 1, 3)
            zf = [zf] * nd
        out = fused._resize_labels(inputs, list(zf), self.nb_labels, 'LabelResize')
        return out.unsqueeze(-1) if inputs.dim() == out.dim() + 1 else out


# ------------------------------------------------------------------------------------------
# VoxelMorph companions of SpatialTransformer: the layers neurite/tf/models.py instantiates right
# next to it (:802-804 RescaleTransform/VecInt in labels_to_image, :1131, :1149-1154).  voxelmorph is not
# vendored by the reference; constructor arguments follow its published layers.
# ------------------------------------------------------------------------------------------

class VecInt(_Layer):
    """
    Integrate a stationary velocity field [B, *S, D] into a displacement field by scaling and squaring
    (int_steps self-compositions, each one warp+add kernel pass) or by quadrature.
    """

    def __init__(self, indexing='ij', method='ss', int_steps=7, out_time_pt=1, ode_args=None, odeint_fn=None,
                 **kwargs):
        super().__init__(**kwargs)
        assert indexing in ['ij', 'xy'], "indexing has to be 'ij' (matrix) or 'xy' (cartesian)"
        self.indexing = indexing
        self.method = method
        self.int_steps = int_steps
        self.inshape = None
        self.out_time_pt = out_time_pt
        self.odeint_fn = odeint_fn
        self.ode_args = ode_args
        if ode_args is None:
            self.ode_args = {'rtol': 1e-6, 'atol': 1e-12}

    def get_config(self):
        config = super().get_config().copy()
        config.update({'indexing': self.indexing, 'method': self.method, 'int_steps': self.int_steps,
                       'out_time_pt': self.out_time_pt, 'ode_args': self.ode_args, 'odeint_fn': self.odeint_fn})
        return config

    def build(self, input_shape):
        self.built = True
        trf_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        self.inshape = trf_shape
        if trf_shape[-1] != len(trf_shape) - 2:
            raise Exception('transform ndims %d does not match expected ndims %d'
                            % (trf_shape[-1], len(trf_shape) - 2))

    def call(self, inputs):
        if isinstance(inputs, (list, tuple)):
            if len(inputs) > 1:
                raise NotImplementedError('VecInt: out_time_pt input is not implemented')
            inputs = inputs[0]
        loc_shift = inputs
        _lib.require_device(loc_shift)
        loc_shift = loc_shift.reshape([-1, *self.inshape[1:]])
        if self.indexing == 'xy' and loc_shift.shape[-1] > 1:          # cartesian: swap the first two components
            loc_shift = torch.cat([loc_shift[..., 1:2], loc_shift[..., 0:1], loc_shift[..., 2:]], -1)
        return utils.integrate_vec(loc_shift, method=self.method, nb_steps=self.int_steps, _batched=True)


class RescaleTransform(_Layer):
    """Rescale a transform: dense [B, *S, D] fields are resized and their vectors scaled; affines get a scaled translation."""

    def __init__(self, zoom_factor, interp_method='linear', **kwargs):
        super().__init__(**kwargs)
        self.zoom_factor = zoom_factor
        self.interp_method = interp_method

    def get_config(self):
        config = super().get_config().copy()
        config.update({'zoom_factor': self.zoom_factor, 'interp_method': self.interp_method})
        return config

    def compute_output_shape(self, input_shape):
        if utils.is_affine_shape(input_shape[1:]):
            return (input_shape[0], self.ndims, self.ndims + 1)
        shape = [int(d * self.zoom_factor) for d in input_shape[1:-1]]
        return (input_shape[0], *shape, self.ndims)

    def build(self, input_shape):
        self.ndims = (input_shape[-1] - 1) if utils.is_affine_shape(input_shape[1:]) else input_shape[-1]
        self.built = True

    def call(self, transform):
        _lib.require_device(transform)
        if utils.is_affine_shape(transform.shape[1:]):
            return utils.rescale_affine(transform, self.zoom_factor)
        return utils.rescale_dense_transform(transform, self.zoom_factor, interp_method=self.interp_method,
                                             _batched=True)


class ComposeTransform(_Layer):
    """
    Compose a list of affine [B, N, N+1] and/or dense [B, *S, N] transforms, T = T0 o T1 o ...; dense if any input is.
    """

    def __init__(self, interp_method='linear', shift_center=True, indexing='ij', **kwargs):
        super().__init__(**kwargs)
        self.interp_method = interp_method
        self.shift_center = shift_center
        self.indexing = indexing

    def get_config(self):
        config = super().get_config().copy()
        config.update({'interp_method': self.interp_method, 'shift_center': self.shift_center,
                       'indexing': self.indexing})
        return config

    def build(self, input_shape):
        if not isinstance(input_shape, (list, tuple)) or not isinstance(input_shape[0], (list, tuple)):
            raise Exception('ComposeTransform must be called for a list of transforms.')
        self.built = True

    def call(self, transforms):
        if len(transforms) == 1:
            raise ValueError('ComposeTransform must be called for a list of transforms.')
        _lib.require_device(*transforms)
        return utils.compose(list(transforms), interp_method=self.interp_method, shift_center=self.shift_center,
                             indexing=self.indexing, _batched=True)


class AffineToDenseShift(_Layer):
    """Affine [B, N, N+1] -> dense displacement field [B, *shape, N]."""

    def __init__(self, shape, shift_center=True, **kwargs):
        super().__init__(**kwargs)
        self.shape = shape
        self.ndims = len(shape)
        self.shift_center = shift_center

    def get_config(self):
        config = super().get_config().copy()
        config.update({'shape': self.shape, 'shift_center': self.shift_center})
        return config

    def compute_output_shape(self, input_shape):
        return (input_shape[0], *self.shape, self.ndims)

    def build(self, input_shape):
        utils.validate_affine_shape(input_shape)
        self.built = True

    def call(self, mat):
        _lib.require_device(mat)
        return utils.affine_to_dense_shift(mat, self.shape, shift_center=self.shift_center)      # batched: one launch


class GaussianBlur(_Layer):
    """
    Blur a tensor [B, *S, C] by convolving it with a Gaussian kernel, isotropic or anisotropic, randomised or not
    (neurite/tf/layers.py:251-364): `utils.gaussian_kernel(separate=True)` + `utils.separable_conv` -- one HIP pass per
    spatial axis, no transposes.  Differentiable with respect to the input (float32, once) through `utils.separable_conv`; the taps
    are host-built constants, so there is no gradient with respect to sigma.
    """

    def __init__(self, sigma=None, level=None, random=False, min_sigma=0, isotropic=False, seed=None, **kwargs):
        assert sigma is not None or level is not None, 'sigma or level must be provided'
        assert not (sigma is not None and level is not None), 'only sigma or level must be provided'
        if level is not None:
            import warnings
            warnings.warn('The `level` argument to ne.layers.GaussianBlur is deprecated and will '
                          'be removed in a future version. Please use `sigma` instead.')
            if level < 1:
                raise ValueError('Gaussian blur level must not be less than 1')
            if random:
                raise ValueError('level argument incompatible with random blurring')
            sigma = (level - 1) ** 2          # the reference computes this and then overwrites it with None (:297,303)
        if isotropic and not random:
            raise ValueError('For non-random blurring, isotropy is implicitly controlled by the '
                             'number of sigmas provided. Set `isotropic` only for random blur.')
        self.sigma = sigma
        self.random = random
        self.min_sigma = min_sigma
        self.isotropic = isotropic
        self.seed = seed
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'sigma': self.sigma, 'random': self.random, 'min_sigma': self.min_sigma,
                       'isotropic': self.isotropic, 'seed': self.seed})
        return config

    def _normalize_sigma(self, sigma, ndims):
        sigma = np.ravel(sigma).tolist()
        if len(sigma) not in (1, ndims):
            raise ValueError(f'1 or {ndims} sigmas expected in {ndims}D space, got {len(sigma)}')
        if any(s < 0 for s in sigma):
            raise ValueError('Gaussian blur sigma must not be less than 0')
        if len(sigma) > 1 and self.isotropic:
            raise ValueError(f'random isotropic blur requires a single sigma, got {len(sigma)}')
        if len(sigma) == 1:
            sigma = sigma * ndims
        return sigma

    def build(self, input_shape):
        ndims = len(input_shape) - 2
        self.sigma = self._normalize_sigma(self.sigma, ndims)
        self.min_sigma = self._normalize_sigma(self.min_sigma, ndims)
        if self.isotropic and self.random:           # the same random kernel along all axes
            self.sigma = self.sigma[:1]
            self.min_sigma = self.min_sigma[:1]
        self.built = True

    def call(self, x):
        if not any(s > 0 for s in self.sigma):
            return x
        if self.random:
            kernel = utils.gaussian_kernel(sigma=self.sigma, random=True, min_sigma=self.min_sigma, separate=True,
                                           dtype=x.dtype, seed=self.seed)
        else:
            # fixed sigmas: the taps are built once per device (a host-built kernel costs three blocking copies per call)
            key = (str(x.device), x.dtype, tuple(self.sigma))
            if getattr(self, '_taps_key', None) != key:
                kernel = utils.gaussian_kernel(sigma=self.sigma, separate=True, dtype=x.dtype)
                kernel = kernel if isinstance(kernel, (list, tuple)) else [kernel]
                self._taps = [k.to(x.device).contiguous() for k in kernel]
                self._taps_key = key
            kernel = self._taps
        return utils.separable_conv(x, kernel, batched=True)


class Subsample(_Layer):
    """
    Symmetrically subsample a tensor [B, *S, C] by a random stride along one random spatial axis with nearest-neighbour
    interpolation and (by default) up-sample it again, to create thick slices (layers.py:367-443).  Differentiable with respect to
    the input (float32, once) through `utils.subsample_axis`.
    """

    def __init__(self, stride_min=1, stride_max=8, axes=None, prob=1, upsample=True, seed=None, **kwargs):
        self.stride_min = stride_min
        self.stride_max = stride_max
        self.axes = axes
        self.prob = prob
        self.upsample = upsample
        self.seed = seed
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'stride_min': self.stride_min, 'stride_max': self.stride_max, 'axes': self.axes, 'prob': self.prob,
                       'upsample': self.upsample, 'seed': self.seed})
        return config

    def build(self, input_shape):
        ndims = len(input_shape) - 2
        assert ndims in (1, 2, 3), 'only 1D, 2D, or 3D supported'
        self.axes = augment.normalize_axes(self.axes, input_shape, range(1, ndims + 1), none_means_all=True)
        self._rand = np.random.default_rng(self.seed)
        self.built = True

    def call(self, x):
        if self.prob == 0 or self.stride_max == 1:
            return x
        return utils.subsample_axis(x, stride_min=self.stride_min, stride_max=self.stride_max, axes=self.axes, prob=self.prob,
                                    upsample=self.upsample, seed=int(self._rand.integers(2 ** 31 - 1)))


class RandomCrop(_Layer):
    """Randomly crop the content of a tensor [B, *S, C] along a spatial axis by multiplying with a binary mask
    (layers.py:446-519)."""

    def __init__(self, crop_min=0, crop_max=0.5, axis=None, prob=1, bilateral=False, seed=None, **kwargs):
        self.crop_min = crop_min
        self.crop_max = crop_max
        self.axis = axis
        self.prob = prob
        self.bilateral = bilateral
        self.seed = seed
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'crop_min': self.crop_min, 'crop_max': self.crop_max, 'axis': self.axis, 'prob': self.prob,
                       'bilateral': self.bilateral, 'seed': self.seed})
        return config

    def build(self, input_shape):
        ndims = len(input_shape) - 2
        self.axis = augment.normalize_axes(self.axis, input_shape, range(1, ndims + 1), none_means_all=True)
        self._rand = np.random.default_rng(self.seed)
        self.built = True

    def call(self, x):
        if self.prob == 0:
            return x
        dev = _lib.require_device(x)
        if x.dtype != torch.float32:
            raise NotImplementedError('RandomCrop: float32 tensors, got %s' % x.dtype)
        mask = augment.draw_crop_mask(x, crop_min=self.crop_min, crop_max=self.crop_max, axis=self.axis, prob=self.prob,
                                      bilateral=self.bilateral, seed=int(self._rand.integers(2 ** 31 - 1)))
        self.last_mask = mask
        ax = int(np.argmax([m > 1 for m in mask.shape])) if max(mask.shape) > 1 else self.axis[0]
        x = x.contiguous()
        y = torch.empty_like(x)
        outer = int(np.prod(x.shape[:ax])) if ax else 1
        inner = int(np.prod(x.shape[ax + 1:]))
        _lib.call(dev, 'nrt_synth_axis_mask_f32', _lib.ptr(x), _lib.ptr(mask.reshape(-1).contiguous()), _lib.ptr(y), outer, x.shape[ax],
                  inner)
        return y


class GaussianNoise(_Layer):
    """
    Sample and add (or return) Gaussian noise whose SD is drawn uniformly from [noise_min, noise_max) times the absolute
    maximum of the input (unless `absolute`), separately along `axes` (layers.py:2305-2403).  float32 [B, *S, C].
    """

    def __init__(self, noise_min=0.01, noise_max=0.10, noise_only=False, absolute=False, axes=(0, -1), seed=None, **kwargs):
        self.noise_min = noise_min
        self.noise_max = noise_max
        self.noise_only = noise_only
        self.absolute = absolute
        self.axes = axes
        self.seed = seed
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'noise_min': self.noise_min, 'noise_max': self.noise_max, 'noise_only': self.noise_only,
                       'absolute': self.absolute, 'axes': self.axes, 'seed': self.seed})
        return config

    def build(self, in_shape):
        num_dim = len(in_shape)
        self.axes = [int(ax) + num_dim if ax < 0 else int(ax) for ax in np.ravel(self.axes)]
        assert all(0 <= ax < num_dim for ax in self.axes), 'invalid axes'
        if any(ax not in (0, num_dim - 1) for ax in self.axes):
            raise NotImplementedError('neurite_amd GaussianNoise: a separate SD along the batch and / or feature axis only')
        self._gen = None
        self.built = True

    def call(self, x):
        if self.noise_max == 0 and not self.noise_only:
            return x
        dev = _lib.require_device(x)
        if x.dtype != torch.float32:
            raise NotImplementedError('GaussianNoise: float32 tensors, got %s' % x.dtype)
        if self._gen is None:
            self._gen = torch.Generator(device=dev)
            if self.seed is None:
                self._gen.seed()
            else:
                self._gen.manual_seed(int(self.seed))
        x = x.contiguous()
        B, C = x.shape[0], x.shape[-1]
        nb = B if 0 in self.axes else 1
        nc = C if (x.dim() - 1) in self.axes else 1
        lo = torch.as_tensor(self.noise_min, dtype=torch.float32, device=dev)
        hi = torch.as_tensor(self.noise_max, dtype=torch.float32, device=dev)
        sd = lo + (hi - lo) * torch.rand((nb, nc), generator=self._gen, device=dev)
        if not self.absolute:
            mm = utils._device_minmax(x)
            sd = sd * torch.maximum(mm[0].abs(), mm[1].abs())
        sd = sd.contiguous()
        noise = torch.randn(x.shape, generator=self._gen, device=dev)
        self.last_draws = dict(sd=sd, noise=noise)
        base = torch.zeros_like(x) if self.noise_only else x
        y = torch.empty_like(x)
        _lib.call(dev, 'nrt_synth_noise_add_f32', _lib.ptr(base), _lib.ptr(noise), _lib.ptr(sd), _lib.ptr(y), B, x[0].numel() // C, C,
                  nc if nb > 1 else 0, 1 if nc > 1 else 0)
        return y


class PerlinNoise(_Layer):
    """
    Sample Perlin noise of the input's shape (or `shape`, excluding the batch dimension) by drawing noise at full resolution
    and smoothing it randomly at several scales (layers.py:2406-2508); `reduce` is 'std' or 'max' (or tf / torch functions
    of those names).  Only the batch size (and possibly the shape) of the input is used.
    """

    def __init__(self, shape=None, noise_min=0.01, noise_max=1, fwhm_min=4, fwhm_max=32, isotropic=False, reduce='std',
                 out_type=torch.float32, axes=None, seed=None, **kwargs):
        self.shape = shape
        self.noise_min = noise_min
        self.noise_max = noise_max
        self.fwhm_min = fwhm_min
        self.fwhm_max = fwhm_max
        self.isotropic = isotropic
        self.reduce = reduce
        self.out_type = out_type
        self.axes = axes
        self.seed = seed
        super().__init__(**kwargs)

    def get_config(self):
        config = super().get_config().copy()
        config.update({'shape': self.shape, 'noise_min': self.noise_min, 'noise_max': self.noise_max, 'fwhm_min': self.fwhm_min,
                       'fwhm_max': self.fwhm_max, 'isotropic': self.isotropic, 'reduce': self.reduce, 'out_type': self.out_type,
                       'axes': self.axes, 'seed': self.seed})
        return config

    def build(self, input_shape):
        self._rand = np.random.default_rng(self.seed)
        shape = input_shape if self.shape is None else (input_shape[0],) + tuple(self.shape)
        self.axes = augment.normalize_axes(self.axes, shape, range(1, len(shape)), none_means_all=False)
        self.built = True

    def call(self, x):
        dev = _lib.require_device(x)
        shape = tuple(x.shape[1:]) if self.shape is None else tuple(int(s) for s in self.shape)
        return torch.stack([
            augment.draw_perlin_full(shape, noise_min=self.noise_min, noise_max=self.noise_max, isotropic=self.isotropic,
                                     fwhm_min=self.fwhm_min, fwhm_max=self.fwhm_max, batched=False, featured=True,
                                     dtype=torch.float32, seed=int(self._rand.integers(2 ** 31 - 1)),
                                     axes=[ax - 1 for ax in self.axes], reduce=self.reduce, device=dev)
            for _ in range(x.shape[0])], 0)


def _normalize_tuple(value, n, name):
    """keras conv_utils.normalize_tuple."""
    if isinstance(value, int):
        return (value,) * n
    try:
        value_tuple = tuple(value)
    except TypeError:
        raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' + str(value))
    if len(value_tuple) != n:
        raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' + str(value))
    for v in value_tuple:
        if not isinstance(v, int):
            raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' + str(value))
    return value_tuple


def _conv_output_length(input_length, filter_size, padding, stride):
    """keras conv_utils.conv_output_length for 'valid' / 'same' (used at neurite/tf/layers.py:963-968)"""
    if input_length is None:
        return None
    n = input_length if padding == 'same' else input_length - filter_size + 1
    return (n + stride - 1) // stride


def _lc3d_plan(ins, cin, ksize, strides, padding, outs, cout, implementation, data_format):
    """
    Host-side bookkeeping of LocallyConnected3D, built once per layer: how the layer's own kernel layout maps onto the
    streaming layout W1[o, (a, b, e, ci), co] of the HIP kernel, and the zero padding that turns 'same' into 'valid'.

    The window of output position p along axis d covers the inputs [p * s - left, p * s - left + k) clipped to the volume,
    left = k // 2 for 'same' and 0 for 'valid' (conv_connected_inputs, layers.py:1474-1482).
    gather[o, f, co]: flat index into the layer's kernel array of the weight of W1[o, f, co] (None = the kernel already is
    W1); mask: 0 where the tap lies outside the volume.  Implementation 3 ranks the connected (out_idx, in_idx) pairs in
    sorted order (the order of `kernel_idxs`, :1012-1022).
    """
    T3 = [int(k) for k in ksize]
    T = T3[0] * T3[1] * T3[2]
    O = int(np.prod(outs))
    F = T * cin
    cf = data_format == 'channels_first'
    left = [k // 2 if padding == 'same' else 0 for k in T3]
    need = [(outs[d] - 1) * strides[d] + T3[d] for d in range(3)]
    padded = [max(need[d], ins[d] + left[d]) for d in range(3)]
    plan = {'O': O, 'F': F, 'pad_before': tuple(left), 'padded': tuple(padded) if padding == 'same' else None,
            'gather': None, 'mask': None, 'nnz': None}
    if implementation == 1 and not cf:
        return plan
    # the table is built on the host from several int64 arrays of O * F * cout entries (~40 B per entry at the peak) and kept on
    # the device: 2^27 entries is ~5 GB of host memory; beyond that a promise of NotImplementedError is better than an opaque OOM
    if O * F * cout >= (1 << 27):
        raise NotImplementedError('LocallyConnected3D: the re-layout table of implementation %d (%s) would have %d entries; '
                                  'use implementation 1 / channels_last for layers of this size' % (implementation, data_format,
                                                                                                     O * F * cout))
    o_r, o_c, o_z = np.meshgrid(*[np.arange(n) for n in outs], indexing='ij')
    o_pos = np.stack([o_r.reshape(-1), o_c.reshape(-1), o_z.reshape(-1)], 1)               # [O, 3] row-major
    t_a, t_b, t_e = np.meshgrid(*[np.arange(k) for k in T3], indexing='ij')
    taps = np.stack([t_a.reshape(-1), t_b.reshape(-1), t_e.reshape(-1)], 1)                # [T, 3]
    ip = o_pos[:, None, :] * np.asarray(strides)[None, None, :] + taps[None, :, :] - np.asarray(left)[None, None, :]   # [O, T, 3]
    valid = np.all((ip >= 0) & (ip < np.asarray(ins)[None, None, :]), -1)                  # [O, T]
    ipc = np.clip(ip, 0, np.asarray(ins)[None, None, :] - 1)
    ipflat = (ipc[..., 0] * ins[1] + ipc[..., 1]) * ins[2] + ipc[..., 2]                   # [O, T]
    IN = int(np.prod(ins))
    o = np.arange(O, dtype=np.int64)[:, None, None, None]
    t = np.arange(T, dtype=np.int64)[None, :, None, None]
    ci = np.arange(cin, dtype=np.int64)[None, None, :, None]
    co = np.arange(cout, dtype=np.int64)[None, None, None, :]
    ipf = ipflat.astype(np.int64)[:, :, None, None]
    vmask = np.broadcast_to(valid[:, :, None, None], (O, T, cin, cout))
    if implementation == 1:                                    # channels_first: feature order (cin, kr, kc, kz)
        g = (o * F + ci * T + t) * cout + co
        g = np.broadcast_to(g, (O, T, cin, cout))
    elif implementation == 2:
        if cf:                                                 # (cin, in..., cout, out...)
            g = ((ci * IN + ipf) * cout + co) * O + o
        else:                                                  # (in..., cin, out..., cout)
            g = ((ipf * cin + ci) * O + o) * cout + co
    else:
        if cf:                                                 # concat_idxs = (filter,) + spatial   :1404-1405
            out_idx = co * O + o
            in_idx = ci * IN + ipf
        else:
            out_idx = o * cout + co
            in_idx = ipf * cin + ci
        out_idx = np.broadcast_to(out_idx, (O, T, cin, cout))
        in_idx = np.broadcast_to(in_idx, (O, T, cin, cout))
        keys = (out_idx * (IN * cin) + in_idx)[vmask]
        order = np.argsort(keys, kind='stable')
        rank = np.empty(order.size, np.int64)
        rank[order] = np.arange(order.size)
        g = np.zeros((O, T, cin, cout), np.int64)
        g[vmask] = rank
        plan['nnz'] = int(order.size)
        plan['pairs'] = (out_idx[vmask][order], in_idx[vmask][order])       # == sorted(conv_kernel_idxs(...)), for the tests
    plan['gather'] = np.ascontiguousarray(np.where(vmask, g, 0).reshape(O, F, cout))
    plan['mask'] = None if valid.all() else np.ascontiguousarray(vmask.reshape(O, F, cout).astype(np.float32))
    return plan


class _Pad3dFn(torch.autograd.Function):
    """zero padding of a channels-last volume (csrc/lc3d.hip: pad3d_rows); backward = the interior of the gradient"""

    @staticmethod
    def forward(ctx, x, before, padded):
        ctx.cfg = (tuple(x.shape[1:4]), tuple(before), tuple(padded))
        return _pad3d(x, ctx.cfg[0], before, padded, crop=False)

    @staticmethod
    def backward(ctx, g):
        ins, before, padded = ctx.cfg
        return _pad3d(g.contiguous(), ins, before, padded, crop=True), None, None


def _pad3d(t, ins, before, padded, crop):
    dev = _lib.require_device(t)
    B, C = t.shape[0], t.shape[-1]
    shape = [B] + list(ins if crop else padded) + [C]
    out = torch.empty(shape, dtype=t.dtype, device=dev)
    _lib.call(dev, 'nrt_pad3d', _lib.ptr(t), _lib.ptr(out), B, _lib.ints(ins), _lib.ints(before), _lib.ints(padded), C * t.element_size(),
              int(crop))
    return out


class _Lc3dFn(torch.autograd.Function):
    """LocallyConnected3D forward / backward on csrc/lc3d.hip (x channels-last, contiguous)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, run, run_backward):
        ctx.run_backward = run_backward
        with torch.no_grad():
            return run()

    @staticmethod
    def backward(ctx, g):
        dx, dk, db = ctx.run_backward(g, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return dx, dk, db, None, None


class LocallyConnected3D(_Layer):
    """
    Locally-connected layer for 3D inputs: a Conv3D whose weights are NOT shared between output positions
    (neurite/tf/layers.py:811-1532).  Implementation 1 semantics ('valid' padding): kernel
    [O, kr*kc*kz*Cin, filters] with the patch flattened in (kr, kc, kz, cin) order, O = output positions in
    row-major order, bias [or, oc, oz, filters].  Runs on the weight-streaming HIP kernel (csrc/lc3d.hip):
    every weight is read once, fp32 accumulation, bias + activation fused; float32 or bfloat16 tensors.
    """

    def __init__(self, filters, kernel_size, strides=(1, 1, 1), padding='valid', data_format=None, activation=None,
                 use_bias=True, kernel_initializer='glorot_uniform', bias_initializer='zeros',
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, implementation=1, **kwargs):
        super().__init__(**kwargs)
        self.filters = filters
        self.kernel_size = _normalize_tuple(kernel_size, 3, 'kernel_size')
        self.strides = _normalize_tuple(strides, 3, 'strides')
        self.padding = str(padding).lower()
        if self.padding not in ('valid', 'same'):
            raise ValueError('The `padding` argument must be a list/tuple or one of "valid", "same". Received: '
                             + str(padding))
        if self.padding != 'valid' and implementation == 1:                              # layers.py:934-936
            raise ValueError('Invalid border mode for LocallyConnected3D '
                             '(only "valid" is supported if implementation is 1): ' + padding)
        self.data_format = 'channels_last' if data_format is None else str(data_format).lower()
        if self.data_format not in ('channels_last', 'channels_first'):
            raise ValueError('The `data_format` argument must be one of "channels_first", "channels_last". Received: '
                             + str(data_format))
        if activation != 'softmax':
            from .models import _act_code
            _act_code(activation)                   # NotImplementedError for what the kernels do not know
        self.activation = activation
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.kernel_regularizer = kernel_regularizer
        self.bias_regularizer = bias_regularizer
        self.activity_regularizer = activity_regularizer
        self.kernel_constraint = kernel_constraint
        self.bias_constraint = bias_constraint
        if implementation not in (1, 2, 3):
            raise ValueError('Unrecognized implementation mode: %d.' % implementation)
        self.implementation = implementation
        self.kernel = None
        self.bias = None
        self._variant = 0
        self._stream_cache = None

    def build(self, input_shape):
        if self.data_format == 'channels_last':                                           # layers.py:952-958
            input_row, input_col, input_z = input_shape[1:-1]
            input_filter = input_shape[4]
        else:
            input_row, input_col, input_z = input_shape[2:]
            input_filter = input_shape[1]
        if input_row is None or input_col is None or input_z is None:
            raise ValueError('The spatial dimensions of the inputs to  a LocallyConnected3D layer should be '
                             'fully-defined, but layer received the inputs shape ' + str(input_shape))
        ins = (int(input_row), int(input_col), int(input_z))
        out = [_conv_output_length(n, k, self.padding, st) for n, k, st in zip(ins, self.kernel_size, self.strides)]
        self.output_row, self.output_col, self.output_z = out                              # :963-971
        T = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        F = T * input_filter
        O = out[0] * out[1] * out[2]
        IN = ins[0] * ins[1] * ins[2]
        cf = self.data_format == 'channels_first'
        if self.implementation == 1:                                                       # :973-984
            self.kernel_shape = (O, F, self.filters)
            fan_in, fan_out = F * O, self.filters * O          # Keras' fans of a rank-3 shape (receptive field = O)
        elif self.implementation == 2:                                                     # :986-1006
            self.kernel_shape = ((input_filter,) + ins + (self.filters,) + tuple(out)) if cf \
                else (ins + (input_filter,) + tuple(out) + (self.filters,))
            rf = int(np.prod(self.kernel_shape[:-2]))
            fan_in, fan_out = self.kernel_shape[-2] * rf, self.kernel_shape[-1] * rf
        else:                                                                              # :1008-1028
            self.dense_kernel_shape = (O * self.filters, IN * input_filter)
            fan_in = fan_out = None
        self.input_filter = int(input_filter)
        self.input_spatial = ins
        self._plan = _lc3d_plan(ins, int(input_filter), self.kernel_size, self.strides, self.padding, tuple(out),
                                self.filters, self.implementation, self.data_format)
        if self.implementation == 3:
            self.kernel_shape = (self._plan['nnz'],)
            fan_in = fan_out = int(np.sqrt(self._plan['nnz']))  # Keras' fans of a rank-1 shape: sqrt(n) each
        limit = (6.0 / max(1, fan_in + fan_out)) ** 0.5
        dev = getattr(self, '_build_device', None)
        dt = getattr(self, '_build_dtype', torch.float32)
        dt = dt if dt in (torch.float32, torch.bfloat16) else torch.float32
        if self.kernel_initializer == 'glorot_uniform':
            k = torch.empty(self.kernel_shape, dtype=dt, device=dev).uniform_(-limit, limit)
        elif self.kernel_initializer == 'zeros':
            k = torch.zeros(self.kernel_shape, dtype=dt, device=dev)
        else:
            raise NotImplementedError('kernel_initializer %r' % (self.kernel_initializer,))
        self.kernel = nn.Parameter(k)
        if self.use_bias:                                                                  # :1030-1039
            self.bias = nn.Parameter(torch.zeros(out[0], out[1], out[2], self.filters, dtype=dt, device=dev))
        self.built = True

    def compute_output_shape(self, input_shape):
        if self.data_format == 'channels_first':
            dims = input_shape[2:5]
        else:
            dims = input_shape[1:4]
        o = [_conv_output_length(n, k, self.padding, st) for n, k, st in zip(dims, self.kernel_size, self.strides)]
        if self.data_format == 'channels_first':
            return (input_shape[0], self.filters, o[0], o[1], o[2])
        return (input_shape[0], o[0], o[1], o[2], self.filters)

    def train(self, mode=True):
        self._stream_cache = None
        return super().train(mode)

    def _streaming_weights(self):
        """
        The un-shared weights in the layout the HIP kernel streams: [O, (kr, kc, kz, cin), filters] (= implementation 1,
        channels_last).  The other layouts hold the SAME numbers elsewhere -- implementation 1 channels_first flattens the
        patch channel-major (layers.py:1176-1186), 2 is a dense [in..., cin, out..., filters] array of which only the
        connected entries are used (:986-1006, 1300-1308), 3 the values of the sparse matrix in sorted (out_idx, in_idx)
        order (:1012-1028) -- and are re-laid out by ONE gather through an index table built at `build` time (a tap that
        'same' padding clips away gets weight 0).  Differentiable (torch indexing), so the kernel's weight gradient flows
        back into the layer's own parameter; cached while no gradient is being recorded.
        """
        plan = self._plan
        if plan['gather'] is None:
            return self.kernel
        track = torch.is_grad_enabled() and self.kernel.requires_grad
        key = (self.kernel._version, self.kernel.data_ptr(), self.kernel.device)
        if not track and self._stream_cache is not None and self._stream_cache[0] == key:
            return self._stream_cache[1]
        dev = self.kernel.device
        if plan.get('gather_dev') is None or plan['gather_dev'].device != dev:
            plan['gather_dev'] = torch.from_numpy(plan['gather']).to(dev)
            plan['mask_dev'] = None if plan['mask'] is None else torch.from_numpy(plan['mask']).to(dev)
        w = self.kernel.reshape(-1)[plan['gather_dev']]
        if plan['mask_dev'] is not None:
            w = w * plan['mask_dev'].to(w.dtype)
        w = w.reshape(plan['O'], plan['F'], self.filters)
        if not track:
            self._stream_cache = (key, w.detach())
        return w

    def _bias_channels_last(self):
        if self.bias is None:
            return None
        if self.data_format == 'channels_first':
            # K.bias_add on channels_first data RESHAPES the [or, oc, oz, filters] array to (1, filters, or, oc, oz)
            # (keras backend.bias_add); expressed for the channels-last kernel: element [co, r, c, z] of that view
            o = (self.output_row, self.output_col, self.output_z)
            return self.bias.reshape((self.filters,) + o).permute(1, 2, 3, 0).contiguous()
        return self.bias

    def get_config(self):
        config = {
            'filters': self.filters, 'kernel_size': self.kernel_size, 'strides': self.strides, 'padding': self.padding,
            'data_format': self.data_format, 'activation': self.activation, 'use_bias': self.use_bias,
            'kernel_initializer': self.kernel_initializer, 'bias_initializer': self.bias_initializer,
            'kernel_regularizer': self.kernel_regularizer, 'bias_regularizer': self.bias_regularizer,
            'activity_regularizer': self.activity_regularizer, 'kernel_constraint': self.kernel_constraint,
            'bias_constraint': self.bias_constraint, 'implementation': self.implementation,
        }
        base_config = super().get_config()
        return dict(list(base_config.items()) + list(config.items()))

    def call(self, inputs):
        dev = _lib.require_device(inputs, self.kernel)
        x = inputs
        if x.dim() != 5:
            raise ValueError('LocallyConnected3D expects a 5D input, got shape %s' % (tuple(x.shape),))
        if self.data_format == 'channels_first':
            x = x.permute(0, 2, 3, 4, 1)
        x = x.contiguous()
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError('LocallyConnected3D: float32 or bfloat16 tensors, got %s' % x.dtype)
        if self.kernel.dtype != x.dtype:
            raise TypeError('input dtype %s does not match the layer weights %s (use layer.to(dtype))'
                            % (x.dtype, self.kernel.dtype))
        B, cin = x.shape[0], x.shape[-1]
        if cin != self.input_filter:
            raise ValueError('expected %d input channels, got %d' % (self.input_filter, cin))
        if tuple(x.shape[1:4]) != tuple(self.input_spatial):
            raise ValueError('input spatial shape %s does not match the shape the layer was built for'
                             % (list(x.shape[1:4]),))
        plan = self._plan
        if plan['padded'] is not None:                      # padding='same': the 'valid' layer on the zero-padded input
            x = _Pad3dFn.apply(x, plan['pad_before'], plan['padded'])
        S = list(x.shape[1:4])
        O = [self.output_row, self.output_col, self.output_z]
        w1 = self._streaming_weights()
        bias_cl = self._bias_channels_last()
        y = torch.empty([B] + O + [self.filters], dtype=x.dtype, device=dev)
        from .models import _ACTS
        act = 0 if self.activation == 'softmax' else _ACTS[self.activation]       # softmax: linear epilogue + the softmax kernel below
        kact = act if act <= 2 else 0               # elu / relu are fused; the other activations run as an element-wise pass
        dt = _lib.DT_F32 if x.dtype == torch.float32 else _lib.DT_BF16
        k = w1.detach().contiguous()
        bias = None if bias_cl is None else bias_cl.detach().contiguous()
        xd = x.detach()

        def run():
            _lib.call(dev, 'nrt_lc3d_f', _lib.ptr(xd), _lib.ptr(k), _lib.ptr(bias), _lib.ptr(y), dt, B, _lib.ints(S), cin,
                      _lib.ints(self.kernel_size), _lib.ints(self.strides), self.filters, kact, int(self._variant))
            if act > 2:
                from .models import _elementwise
                y.copy_(_elementwise(y.float(), act=act))        # in place: the backward reads the activated output
            return y

        def run_backward(g, need_x, need_k, need_b):
            g = g.contiguous()
            dk = torch.empty_like(k) if need_k else None
            db = torch.empty((int(np.prod(O)), self.filters), dtype=xd.dtype, device=dev) if need_b else None
            dx = torch.zeros(xd.shape, dtype=torch.float32, device=dev) if need_x else None
            _lib.call(dev, 'nrt_lc3d_bwd_f', _lib.ptr(xd), _lib.ptr(k), _lib.ptr(y), _lib.ptr(g), _lib.ptr(dk), _lib.ptr(db), _lib.ptr(dx),
                      dt, B, _lib.ints(S), cin, _lib.ints(self.kernel_size), _lib.ints(self.strides), self.filters, act)
            return (None if dx is None else dx.to(xd.dtype)), dk, (None if db is None else db.reshape(bias.shape))

        needs = torch.is_grad_enabled() and (x.requires_grad or w1.requires_grad
                                             or (bias_cl is not None and bias_cl.requires_grad))
        if needs:
            out = _Lc3dFn.apply(x, w1, bias_cl, run, run_backward)
        else:
            out = run()
        if self.activation == 'softmax':            # Keras softmax: over the channel axis of the layer's data format
            from .models import _softmax, _SoftmaxFn
            sm = _SoftmaxFn.apply if (torch.is_grad_enabled() and out.requires_grad) else _softmax
            if self.data_format == 'channels_first':
                # layers.py:1100 applies self.activation to the channels_first tensor and Keras' softmax runs over ITS last axis: the
                # last spatial one, not the filters (a quirk of the reference, kept)
                out = out.permute(0, 4, 1, 2, 3).contiguous()
                return sm(out.float()).to(out.dtype) if out.dtype != torch.float32 else sm(out)
            out = sm(out.float()).to(out.dtype) if out.dtype != torch.float32 else sm(out)
        return out.permute(0, 4, 1, 2, 3) if self.data_format == 'channels_first' else out


# ---------------------------------------------------------------------------------------------------------------------------------
# Hyper-convolution / hyper-dense layers (neurite/tf/layers.py:2515-3033): the kernel and the bias are INPUTS, one set per batch
# entry.  The reference maps a single-entry convolution over the batch with tf.map_fn (:2587, :2860); here the whole batch is one
# launch of the conv kernels with the weight and bias base advanced by the batch entry (csrc/conv.hip: ConvArgs.wstride / bstride,
# nrt_hyperconv3d_f32), and the per-entry weight gradient one launch of the weight-gradient kernel with a grid slice per entry
# (nrt_hyperconv3d_wgrad_f32).  No packed-weight cache: the kernels change with every call.
# ---------------------------------------------------------------------------------------------------------------------------------
def _hyperconv_run(x, kernel, bias, ksize3, dilation, same, kact, flipped=False):
    """act(conv3d(x[b], W[b]) + bias[b]) for every b in one launch.  x [B, X, Y, Z, cin], kernel [B, kx, ky, kz, cin, cout], bias
    [B, cout] or None, all float32 and contiguous.  flipped: convolve with the kernels flipped in space and transposed in their
    channel axes instead (the input gradient: cout -> cin channels)."""
    lib = _lib.lib()
    dev = x.device
    B, S = x.shape[0], list(x.shape[1:4])
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    ci, co = (cout, cin) if flipped else (cin, cout)
    O = S if same else [S[d] - (ksize3[d] - 1) * dilation for d in range(3)]
    out = torch.empty([B] + O + [co], dtype=torch.float32, device=dev)
    weights = packed = None
    if lib.nrt_hyperconv3d_uses_packed(_lib.ints(S), _lib.ints(ksize3), ci, co, int(dilation), int(same)) == 1:
        n = lib.nrt_conv3d_packed_weight_floats(_lib.ints(ksize3), ci, co)
        packed = torch.empty(B * int(n), dtype=torch.float32, device=dev)
        _lib.call(dev, 'nrt_hyperconv3d_pack_weights_f32', _lib.ptr(kernel), B, _lib.ints(ksize3), cin, cout, int(flipped),
                  _lib.ptr(packed))
    else:
        # the direct and single-input-channel kernels read the Keras layout (one batched re-layout for the input gradient)
        weights = kernel.flip(1, 2, 3).transpose(4, 5).contiguous() if flipped else kernel
    if flipped:
        # the transpose of a 'same' convolution pads (k - 1) * dilation - (k - 1) * dilation // 2 before (even kernels: one more
        # than 'same' does)
        from .models import _dgrad_pad_before
        _lib.call(dev, 'nrt_hyperconv3d_pad_f32', _lib.ptr(x), ci, _lib.ptr(weights), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(out), B,
                  _lib.ints(S), _lib.ints(ksize3), co, int(dilation), _lib.ints(_dgrad_pad_before(ksize3, dilation)), int(kact), 0)
    else:
        _lib.call(dev, 'nrt_hyperconv3d_f32', _lib.ptr(x), ci, _lib.ptr(weights), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(out), B,
                  _lib.ints(S), _lib.ints(ksize3), co, int(dilation), int(same), int(kact), 0)
    return out


class _HyperConvFn(torch.autograd.Function):
    """Hyper-convolution with gradients wrt the features, the per-entry kernels and the per-entry biases."""

    @staticmethod
    def forward(ctx, x, kernel, bias, ksize3, dilation, same, act):
        from .models import _ACT_LAST_FUSED, _elementwise
        with torch.no_grad():
            out = _hyperconv_run(x, kernel, bias, ksize3, dilation, same, act if act <= _ACT_LAST_FUSED else 0)
            if act > _ACT_LAST_FUSED:             # activations beyond elu / relu: an element-wise pass over the layer output
                out = _elementwise(out, act=act)
        ctx.cfg = (tuple(ksize3), int(dilation), bool(same), int(act))
        ctx.save_for_backward(x, kernel, out)
        return out

    @staticmethod
    def backward(ctx, g):
        from .models import _act_bwd
        x, kernel, out = ctx.saved_tensors
        ksize3, dilation, same, act = ctx.cfg
        dev = g.device
        dpre = _act_bwd(g, out, act)
        B, S = x.shape[0], list(x.shape[1:4])
        cin, cout = kernel.shape[-2], kernel.shape[-1]
        if not same:
            # a 'valid' convolution is the 'same' one restricted to the outputs whose window lies inside the volume: its backward
            # is the 'same' backward of the output gradient embedded in zeros (as models._ConvFn does it)
            pb = [((ksize3[d] - 1) * dilation) // 2 for d in range(3)]
            dpre = _pad3d(dpre.contiguous(), tuple(dpre.shape[1:4]), pb, S, crop=False)
        need_x, need_k, need_b = ctx.needs_input_grad[:3]
        dx = dk = db = None
        if need_k or need_b:
            dk = torch.zeros_like(kernel)
            db = torch.zeros(B, cout, dtype=torch.float32, device=dev)
            _lib.call(dev, 'nrt_hyperconv3d_wgrad_f32', _lib.ptr(x), _lib.ptr(dpre), _lib.ptr(dk), _lib.ptr(db), B, _lib.ints(S), cin, cout,
                      _lib.ints(ksize3), dilation)
        if need_x:
            dx = _hyperconv_run(dpre, kernel, None, ksize3, dilation, True, 0, flipped=True)
        return dx, dk if need_k else None, db if need_b else None, None, None, None, None


def _hyperconv(x, kernel, bias, ksize3, dilation, same, act):
    """x [B, X, Y, Z, cin], kernel [B, kx, ky, kz, cin, cout], bias [B, cout] or None (float32, checked by the callers)."""
    _lib.require_device(x, kernel, bias)
    x, kernel = x.contiguous(), kernel.contiguous()
    bias = None if bias is None else bias.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or kernel.requires_grad or (bias is not None and bias.requires_grad)):
        return _HyperConvFn.apply(x, kernel, bias, ksize3, dilation, same, act)
    return _HyperConvFn.forward(_NoCtx(), x.detach(), kernel.detach(), None if bias is None else bias.detach(), ksize3, dilation,
                                same, act)


class _NoCtx:
    """stands in for the autograd context when nothing is recorded"""

    def save_for_backward(self, *tensors):
        pass


def _conv_output_length_dilated(n, k, padding, stride, dilation):
    """keras conv_utils.conv_output_length (neurite/tf/layers.py:2624-2630)"""
    if n is None:
        return None
    dk = k + (k - 1) * (dilation - 1)
    n = n if padding == 'same' else n - dk + 1
    return (n + stride - 1) // stride


def _keras_activation_name(activation):
    """what tf.keras.activations.serialize(tf.keras.activations.get(a)) gives for the names the project knows"""
    return 'linear' if activation is None else activation


_TORCH_ACTS = {
    None: lambda t: t, 'linear': lambda t: t, 'relu': torch.relu, 'elu': nn.functional.elu, 'sigmoid': torch.sigmoid,
    'tanh': torch.tanh, 'softplus': nn.functional.softplus, 'softsign': nn.functional.softsign, 'selu': torch.selu,
    'exponential': torch.exp, 'hard_sigmoid': lambda t: torch.clamp(0.2 * t + 0.5, 0.0, 1.0),
    'leaky_relu': lambda t: nn.functional.leaky_relu(t, 0.2),
}


def _require_f32(what, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError('%s: the hyper kernels are float32, got a %s tensor (non-float32 tensors are not implemented)'
                                      % (what, t.dtype))


class HyperConv(_Layer):
    """
    N-D hyper-convolution (neurite/tf/layers.py:2515-2647): a convolution without weights of its own -- called on
    [features, kernel, bias] (or [features, kernel] with use_bias=False), features [B, *space, cin], kernel
    [B, *kernel_size, cin, filters], bias [B, filters]: out[b] = activation(conv(features[b], kernel[b]) + bias[b]).
    One kernel launch for the whole batch (nrt_hyperconv3d_f32); rank 1 and 2 run on the 3-D kernels with leading singleton axes.
    Differentiable in all three inputs.  Limits (NotImplementedError): strides other than 1, tensors that are not float32,
    rank above 3, a dilation rate that differs between the axes.
    """

    def __init__(self, rank, filters, kernel_size, strides=1, padding='valid', dilation_rate=1, activation=None, use_bias=True,
                 name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.rank = rank
        self.filters = filters
        self.kernel_size = _normalize_tuple(kernel_size, rank, 'kernel_size')
        self.strides = _normalize_tuple(strides, rank, 'strides')
        padding = str(padding).lower()
        if padding not in ('valid', 'same', 'causal'):
            raise ValueError('The `padding` argument must be a list/tuple or one of "valid", "same" (or "causal", only for '
                             '`Conv1D). Received: ' + str(padding))
        self.padding = padding
        if self.padding == 'causal':                                                     # layers.py:2558-2559
            raise ValueError('Causal padding is not supported for HyperConv')
        self.dilation_rate = _normalize_tuple(dilation_rate, rank, 'dilation_rate')
        if activation != 'softmax':
            from .models import _act_code
            _act_code(activation)                   # NotImplementedError for what the kernels do not know
        else:
            raise NotImplementedError('activation softmax is not implemented by the hyper layers')
        self.activation = activation
        self.use_bias = use_bias

    def compute_output_shape(self, input_shape):
        input_shape = list(input_shape[0])                                               # the features' shape
        space = input_shape[1:-1]
        new_space = [_conv_output_length_dilated(space[i], self.kernel_size[i], self.padding, self.strides[i], self.dilation_rate[i])
                     for i in range(len(space))]
        return tuple([input_shape[0]] + new_space + [self.filters])

    def get_config(self):
        config = {
            'rank': self.rank, 'filters': self.filters, 'kernel_size': self.kernel_size, 'strides': self.strides,
            'padding': self.padding, 'dilation_rate': self.dilation_rate,
            'activation': _keras_activation_name(self.activation), 'use_bias': self.use_bias,
        }
        base_config = super().get_config()
        return dict(list(base_config.items()) + list(config.items()))

    def _check(self, inputs):
        """the refusals, on shapes and dtypes alone (nothing here touches a device)"""
        what = self.__class__.__name__
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError('%s is called on [features, kernel, bias] or [features, kernel]' % what)
        if self.use_bias and len(inputs) < 3:
            raise ValueError('%s: use_bias=True needs a bias input: [features, kernel, bias]' % what)
        x, kernel = inputs[0], inputs[1]
        bias = inputs[2] if self.use_bias else None
        if self.rank > 3:
            raise NotImplementedError('%s: rank %d is not implemented (the conv kernels are 3-D: rank <= 3)' % (what, self.rank))
        if any(s != 1 for s in self.strides):
            raise NotImplementedError('%s: strides %s are not implemented (the conv kernels are stride 1)' % (what, (self.strides,)))
        _require_f32(what, x, kernel, bias)
        if x.dim() != self.rank + 2:
            raise ValueError('%s: features must be [batch, %d spatial axes, channels], got shape %s' % (what, self.rank, tuple(x.shape)))
        B, cin = x.shape[0], x.shape[-1]
        if kernel.dim() != self.rank + 3 or kernel.shape[0] != B:
            raise ValueError('%s: the kernel input must be [batch = %d, *kernel_size, channels, filters], got shape %s'
                             % (what, B, tuple(kernel.shape)))
        if tuple(kernel.shape[1:1 + self.rank]) != tuple(self.kernel_size):
            raise ValueError('%s: kernel input of spatial size %s, layer kernel_size %s'
                             % (what, tuple(kernel.shape[1:1 + self.rank]), self.kernel_size))
        if kernel.shape[-2] != cin or kernel.shape[-1] != self.filters:
            raise ValueError('%s: channel mismatch: features have %d channels and the layer %d filters, the kernel input is [.., %d, %d]'
                             % (what, cin, self.filters, kernel.shape[-2], kernel.shape[-1]))
        if bias is not None and tuple(bias.shape) != (B, self.filters):
            raise ValueError('%s: the bias input must be [batch = %d, filters = %d], got shape %s' % (what, B, self.filters, tuple(bias.shape)))
        dil = [d for d, k in zip(self.dilation_rate, self.kernel_size) if k > 1]
        if any(d != dil[0] for d in dil):
            raise NotImplementedError('%s: a dilation rate that differs between the axes %s is not implemented'
                                      % (what, (self.dilation_rate,)))
        return x, kernel, bias, (dil[0] if dil else 1)

    def call(self, inputs):
        from .models import _act_code, _lift, _unlift
        x, kernel, bias, dilation = self._check(inputs)
        ksize3 = (1,) * (3 - self.rank) + tuple(self.kernel_size)
        x5 = _lift(x, self.rank)
        k6 = kernel
        for _ in range(3 - self.rank):
            k6 = k6.unsqueeze(1)
        out = _hyperconv(x5, k6, bias, ksize3, dilation, self.padding == 'same', _act_code(self.activation))
        return _unlift(out, self.rank)


class HyperConv2D(HyperConv):
    """2D hyper-convolution layer (neurite/tf/layers.py:2650-2656)."""

    def __init__(self, *args, **kwargs):
        super().__init__(2, *args, **kwargs)


class HyperConv3D(HyperConv):
    """3D hyper-convolution layer (neurite/tf/layers.py:2659-2665)."""

    def __init__(self, *args, **kwargs):
        super().__init__(3, *args, **kwargs)


class _FromDenseMixin:
    """The two 'pseudo dense layers' of the FromDense layers (neurite/tf/layers.py:2751-2794, 2980-3023): hyp @ kernel + bias ->
    activation -> reshape(-1, *target_shape).  A [B, H] x [H, units] product with B of a few entries: host plumbing (torch.addmm),
    differentiable through torch, so the parameters and `hyp` get their gradients from the layer's per-entry kernel / bias gradients."""

    def _init_from_dense(self, hyperkernel_use_bias, hyperbias_use_bias, hyperkernel_activation, hyperbias_activation):
        self.hyperkernel_use_bias = hyperkernel_use_bias
        self.hyperbias_use_bias = hyperbias_use_bias
        for a in (hyperkernel_activation, hyperbias_activation):
            if a not in _TORCH_ACTS:
                raise NotImplementedError('activation %r is not implemented for the hyper mappings (%s are)'
                                          % (a, ', '.join(sorted(str(k) for k in _TORCH_ACTS))))
        self.hyperkernel_activation = hyperkernel_activation
        self.hyperbias_activation = hyperbias_activation
        self.hyperkernel = self.hyperbias = None

    def _build_dense_pseudo_layer(self, name, last_dim, target_shape, use_bias, activation):
        target_shape = tuple(int(v) for v in target_shape)
        units = int(np.prod(target_shape))
        dev = getattr(self, '_build_device', None)
        # Keras' add_weight default for floating-point weights is glorot_uniform, for the bias vectors too (the reference passes no
        # initializer, :2760-2770); fans of a rank-1 shape are (n, n)
        limit = (6.0 / (last_dim + units)) ** 0.5
        kernel = nn.Parameter(torch.empty(last_dim, units, dtype=torch.float32, device=dev).uniform_(-limit, limit))
        setattr(self, '%s_kernel' % name, kernel)
        bias = None
        if use_bias:
            blimit = (6.0 / (2 * units)) ** 0.5
            bias = nn.Parameter(torch.empty(units, dtype=torch.float32, device=dev).uniform_(-blimit, blimit))
            setattr(self, '%s_bias' % name, bias)
        return (kernel, bias, activation, target_shape)

    def _call_dense_pseudo_layer(self, inputs, params):
        kernel, bias, activation, target_shape = params
        if inputs.layout != torch.strided:
            raise NotImplementedError('sparse hyper-network outputs are not implemented')
        inputs = inputs.to(torch.float32)                                                # tf.cast(inputs, self._compute_dtype)
        outputs = inputs @ kernel if bias is None else torch.addmm(bias, inputs, kernel)
        outputs = _TORCH_ACTS[activation](outputs)
        return outputs.reshape((-1,) + tuple(target_shape))

    def _from_dense_config(self):
        return {
            'hyperkernel_use_bias': self.hyperkernel_use_bias, 'hyperbias_use_bias': self.hyperbias_use_bias,
            'hyperkernel_activation': _keras_activation_name(self.hyperkernel_activation),
            'hyperbias_activation': _keras_activation_name(self.hyperbias_activation),
        }

    def _check_from_dense(self, inputs):
        what = self.__class__.__name__
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
            raise ValueError('%s is called on [features, last_hypernetwork_output]' % what)
        x, hyp = inputs
        if hyp.dim() != 2 or hyp.shape[0] != x.shape[0]:
            raise ValueError('%s: the hypernetwork output must be [batch = %d, features], got shape %s' % (what, x.shape[0], tuple(hyp.shape)))
        return x, hyp


class HyperConvFromDense(_FromDenseMixin, HyperConv):
    """
    N-D hyper-convolution with the dense mapping from the last hypernetwork layer to the kernel and bias inside
    (neurite/tf/layers.py:2668-2804).  Called on [features, hyp], hyp [B, H]; parameters (built on the first call):
    hyperkernel_kernel [H, prod(kernel_size) * cin * filters], hyperkernel_bias, hyperbias_kernel [H, filters], hyperbias_bias.
    """

    def __init__(self, rank, filters, kernel_size, hyperkernel_use_bias=True, hyperbias_use_bias=True, hyperkernel_activation=None,
                 hyperbias_activation=None, name=None, **kwargs):
        super().__init__(rank, filters, kernel_size, name=name, **kwargs)
        self._init_from_dense(hyperkernel_use_bias, hyperbias_use_bias, hyperkernel_activation, hyperbias_activation)

    def build(self, input_shape):
        last_dim = int(input_shape[1][-1])
        kernel_shape = tuple(self.kernel_size) + (int(input_shape[0][-1]), self.filters)
        self.hyperkernel = self._build_dense_pseudo_layer('hyperkernel', last_dim, kernel_shape, self.hyperkernel_use_bias,
                                                          self.hyperkernel_activation)
        if self.use_bias:
            self.hyperbias = self._build_dense_pseudo_layer('hyperbias', last_dim, [self.filters], self.hyperbias_use_bias,
                                                            self.hyperbias_activation)
        self.built = True

    def call(self, inputs):
        x, hyp = self._check_from_dense(inputs)
        kernel = self._call_dense_pseudo_layer(hyp, self.hyperkernel)
        if self.use_bias:
            return super().call([x, kernel, self._call_dense_pseudo_layer(hyp, self.hyperbias)])
        return super().call([x, kernel])

    def get_config(self):
        base_config = super().get_config()
        return dict(list(base_config.items()) + list(self._from_dense_config().items()))


class HyperConv2DFromDense(HyperConvFromDense):
    """2D hyper-convolution dense wrapping layer (neurite/tf/layers.py:2807-2813)."""

    def __init__(self, *args, **kwargs):
        super().__init__(2, *args, **kwargs)


class HyperConv3DFromDense(HyperConvFromDense):
    """3D hyper-convolution dense wrapping layer (neurite/tf/layers.py:2816-2822)."""

    def __init__(self, *args, **kwargs):
        super().__init__(3, *args, **kwargs)


class HyperDense(_Layer):
    """
    Hyper-dense layer (neurite/tf/layers.py:2825-2903): called on [x, kernel, bias] (or [x, kernel] with use_bias=False), x
    [B, ..., In] with any number of axes between the batch and the features, kernel [B, In, units], bias [B, units]:
    out[b] = activation(x[b] @ kernel[b] + bias[b]).  Runs as the 1x1x1 case of the hyper-convolution with the rows of x[b] as voxels,
    so it shares its kernels and its backward (matrix cores for In >= 8 and units <= 64, the direct kernel otherwise).  Those kernels
    decline no float32 shape, so there is no torch.baddbmm path; what they do not take is refused: tensors that are not float32 and
    sparse inputs (NotImplementedError).
    """

    def __init__(self, units, activation=None, use_bias=True, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units) if not isinstance(units, int) else units
        if activation == 'softmax':
            raise NotImplementedError('activation softmax is not implemented by the hyper layers')
        from .models import _act_code
        _act_code(activation)
        self.activation = activation
        self.use_bias = use_bias
        self.supports_masking = True

    def compute_output_shape(self, input_shape):
        input_shape = tuple(input_shape[0])
        if len(input_shape) < 2:
            raise ValueError('Shape %s must have rank at least 2' % (input_shape,))
        return input_shape[:-1] + (self.units,)

    def get_config(self):
        config = super().get_config()
        config.update({'units': self.units, 'activation': _keras_activation_name(self.activation), 'use_bias': self.use_bias})
        return config

    def _check(self, inputs):
        what = self.__class__.__name__
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError('%s is called on [x, kernel, bias] or [x, kernel]' % what)
        if self.use_bias and len(inputs) < 3:
            raise ValueError('%s: use_bias=True needs a bias input: [x, kernel, bias]' % what)
        x, kernel = inputs[0], inputs[1]
        bias = inputs[2] if self.use_bias else None
        _require_f32(what, x, kernel, bias)
        if x.layout != torch.strided:
            raise NotImplementedError('%s: sparse inputs are not implemented' % what)
        if x.dim() < 2:
            raise ValueError('%s: x must be [batch, ..., features], got shape %s' % (what, tuple(x.shape)))
        B, cin = x.shape[0], x.shape[-1]
        if kernel.dim() != 3 or kernel.shape[0] != B:
            raise ValueError('%s: the kernel input must be [batch = %d, features, units], got shape %s' % (what, B, tuple(kernel.shape)))
        if kernel.shape[1] != cin or kernel.shape[2] != self.units:
            raise ValueError('%s: channel mismatch: x has %d features and the layer %d units, the kernel input is [.., %d, %d]'
                             % (what, cin, self.units, kernel.shape[1], kernel.shape[2]))
        if bias is not None and tuple(bias.shape) != (B, self.units):
            raise ValueError('%s: the bias input must be [batch = %d, units = %d], got shape %s' % (what, B, self.units, tuple(bias.shape)))
        return x, kernel, bias

    def call(self, inputs):
        from .models import _act_code
        x, kernel, bias = self._check(inputs)
        B, cin = x.shape[0], x.shape[-1]
        rows = 1
        for n in x.shape[1:-1]:
            rows *= int(n)
        # the rows of x[b] as a volume of whole conv tiles where the row count allows it (a 1x1x1 kernel does not care which)
        sx = next(a for a in (4, 2, 1) if rows % a == 0)
        sy = next(a for a in (4, 2, 1) if (rows // sx) % a == 0)
        x5 = x.reshape(B, sx, sy, rows // (sx * sy), cin)
        out = _hyperconv(x5, kernel.reshape(B, 1, 1, 1, cin, self.units), bias, (1, 1, 1), 1, True, _act_code(self.activation))
        return out.reshape(tuple(x.shape[:-1]) + (self.units,))


class HyperDenseFromDense(_FromDenseMixin, HyperDense):
    """
    Hyper-dense layer with the dense mapping from the last hypernetwork layer to its kernel and bias inside
    (neurite/tf/layers.py:2906-3033).  Called on [x, hyp]; parameters: hyperkernel_kernel [H, In * units], hyperkernel_bias,
    hyperbias_kernel [H, units], hyperbias_bias.
    """

    def __init__(self, units, hyperkernel_use_bias=True, hyperbias_use_bias=True, hyperkernel_activation=None,
                 hyperbias_activation=None, **kwargs):
        super().__init__(units, **kwargs)
        self._init_from_dense(hyperkernel_use_bias, hyperbias_use_bias, hyperkernel_activation, hyperbias_activation)

    def build(self, input_shape):
        last_dim = int(input_shape[1][-1])
        self.hyperkernel = self._build_dense_pseudo_layer('hyperkernel', last_dim, [int(input_shape[0][-1]), self.units],
                                                          self.hyperkernel_use_bias, self.hyperkernel_activation)
        if self.use_bias:
            self.hyperbias = self._build_dense_pseudo_layer('hyperbias', last_dim, [self.units], self.hyperbias_use_bias,
                                                            self.hyperbias_activation)
        self.built = True

    def call(self, inputs):
        x, hyp = self._check_from_dense(inputs)
        kernel = self._call_dense_pseudo_layer(hyp, self.hyperkernel)
        if self.use_bias:
            return super().call([x, kernel, self._call_dense_pseudo_layer(hyp, self.hyperbias)])
        return super().call([x, kernel])

    def get_config(self):
        base_config = super().get_config()
        return dict(list(base_config.items()) + list(self._from_dense_config().items()))


# ---------------------------------------------------------------------------------------------------------------------------------
# "Local" layers (a parameter, or a small matrix, at each voxel: neurite/tf/layers.py:746-808, 1535-1607, 1711-1844) and the stream
# layers (:1915-2073) on csrc/local.hip.  Any spatial rank: the kernels see the flat views [B, n] / [B, V, C], a parameter is read
# once for all batch entries and its gradient summed over the batch by the thread that owns it (no atomics, bit-reproducible).
# ---------------------------------------------------------------------------------------------------------------------------------
def _require_f32_local(what, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError('%s: the local / stream kernels are float32, got a %s tensor (non-float32 tensors are not '
                                      'implemented)' % (what, t.dtype))


def _keras_fans(shape):
    """keras initializers _compute_fans"""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1:
        return 1, 1
    if len(shape) == 1:
        return shape[0], shape[0]
    if len(shape) == 2:
        return shape
    rf = int(np.prod(shape[:-2]))
    return shape[-2] * rf, shape[-1] * rf


def _check_initializer(what, initializer):
    if initializer not in ('RandomNormal', 'glorot_uniform', 'zeros'):
        raise NotImplementedError("%s: initializer %r is not implemented ('RandomNormal', 'glorot_uniform' and 'zeros' are)"
                                  % (what, initializer))


def _local_init(what, initializer, shape, device, normal=(0.0, 0.05)):
    """A float32 weight drawn the way Keras draws it: 'RandomNormal' is its default (mean 0, stddev 0.05); `normal` = (mean, stddev)
    replaces it where the reference passes an initializer object of its own (LocalCrossLinear, :1567-1582)."""
    shape = tuple(int(s) for s in shape)
    if initializer is None:
        return torch.empty(shape, dtype=torch.float32, device=device).normal_(normal[0], normal[1])
    _check_initializer(what, initializer)
    if initializer == 'RandomNormal':
        return torch.empty(shape, dtype=torch.float32, device=device).normal_(0.0, 0.05)
    if initializer == 'zeros':
        return torch.zeros(shape, dtype=torch.float32, device=device)
    fan_in, fan_out = _keras_fans(shape)
    limit = (6.0 / max(1, fan_in + fan_out)) ** 0.5
    return torch.empty(shape, dtype=torch.float32, device=device).uniform_(-limit, limit)


def _local_affine_launch(x, probe, mult, bias, bias_scale, B, n, dev):
    """nrt_local_affine_f32 on contiguous float32 tensors; probe: the tensor whose entries' first elements give the factors e[b]"""
    y = torch.empty((B, n), dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_local_affine_f32', _lib.ptr(x), _lib.ptr(probe), 0 if probe is None else probe.stride(0), _lib.ptr(mult),
              _lib.ptr(bias), float(bias_scale), _lib.ptr(y), B, n)
    return y


def _local_affine_bwd_launch(g, x, probe, mult, bias_scale, need_x, need_mult, need_bias, B, n, dev):
    gx = torch.empty((B, n), dtype=torch.float32, device=dev) if need_x else None
    gm = torch.empty(n, dtype=torch.float32, device=dev) if need_mult else None
    gb = torch.empty(n, dtype=torch.float32, device=dev) if need_bias else None
    _lib.call(dev, 'nrt_local_affine_bwd_f32', _lib.ptr(g), _lib.ptr(x), _lib.ptr(probe), 0 if probe is None else probe.stride(0),
              _lib.ptr(mult), float(bias_scale), _lib.ptr(gx), _lib.ptr(gm), _lib.ptr(gb), B, n)
    return gx, gm, gb


class _LocalAffineFn(torch.autograd.Function):
    """y = x * mult + bias * bias_scale (mult may be None), parameters of the shape of one batch entry."""

    @staticmethod
    def forward(ctx, x, mult, bias, bias_scale):
        B, n = x.shape[0], bias.numel()
        ctx.save_for_backward(x, mult)
        ctx.bias_scale = bias_scale
        return _local_affine_launch(x, None, mult, bias, bias_scale, B, n, x.device).view(x.shape)

    @staticmethod
    def backward(ctx, g):
        x, mult = ctx.saved_tensors
        need_x, need_m, need_b = ctx.needs_input_grad[:3]
        need_m = need_m and mult is not None
        g = g.contiguous()
        if mult is None and not need_b:
            return (g if need_x else None), None, None, None
        B, n = x.shape[0], x[0].numel()
        gx, gm, gb = _local_affine_bwd_launch(g, x, None, mult, ctx.bias_scale, need_x and mult is not None, need_m, need_b, B, n,
                                              g.device)
        if need_x:
            gx = g if mult is None else gx.view(x.shape)
        return gx, (gm.view(mult.shape) if need_m else None), (gb.view(x.shape[1:]) if need_b else None), None


class _LocalParamFn(torch.autograd.Function):
    """y[b] = e[b] * (kernel * mult), e[b] = probe[b, 0, ...] * 0 + 1 (1 without a probe); no gradient for the probe."""

    @staticmethod
    def forward(ctx, kernel, probe, mult, B):
        ctx.save_for_backward(probe)
        ctx.cfg = (mult, B)
        return _local_affine_launch(None, probe, None, kernel, mult, B, kernel.numel(), kernel.device).view((B,) + tuple(kernel.shape))

    @staticmethod
    def backward(ctx, g):
        probe, = ctx.saved_tensors
        mult, B = ctx.cfg
        g = g.contiguous()
        _, _, gk = _local_affine_bwd_launch(g, None, probe, None, mult, False, False, True, B, g[0].numel(), g.device)
        return gk.view(g.shape[1:]), None, None, None


def _local_affine(what, x, mult, bias, bias_scale):
    _require_f32_local(what, x, mult, bias)
    _lib.require_device(x, mult, bias)
    if tuple(x.shape[1:]) != tuple(bias.shape):
        raise ValueError('%s: input of shape %s, the layer was built for %s' % (what, tuple(x.shape[1:]), tuple(bias.shape)))
    if x.shape[0] < 1 or bias.numel() < 1:
        raise ValueError('%s: empty input of shape %s' % (what, tuple(x.shape)))
    x = x.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or bias.requires_grad or (mult is not None and mult.requires_grad)):
        return _LocalAffineFn.apply(x, mult, bias, bias_scale)
    return _LocalAffineFn.forward(_NoCtx(), x.detach(), None if mult is None else mult.detach(), bias.detach(), bias_scale)


class _LocalLayer(_Layer):
    """float32 is checked before the layer builds its weights (and before any device is touched)"""

    def forward(self, inputs, **kwargs):
        _require_f32_local(self.__class__.__name__, *(inputs if isinstance(inputs, (list, tuple)) else [inputs]))
        return super().forward(inputs, **kwargs)

    def compute_output_shape(self, input_shape):
        return input_shape


class LocalBias(_LocalLayer):
    """
    One bias per voxel and feature (neurite/tf/layers.py:746-774): `kernel` has the shape of one batch entry and
    call(x) = x + kernel * biasmult.  One kernel launch (nrt_local_affine_f32); the result equals the float32 evaluation of that
    expression bit for bit.  float32 only (NotImplementedError otherwise).
    """

    def __init__(self, my_initializer='RandomNormal', biasmult=1.0, **kwargs):
        self.initializer = my_initializer
        self.biasmult = biasmult
        super().__init__(**kwargs)
        self.kernel = None

    def build(self, input_shape):
        self.kernel = nn.Parameter(_local_init('LocalBias', self.initializer, input_shape[1:], getattr(self, '_build_device', None)))
        self.built = True

    def call(self, x):
        return _local_affine('LocalBias', x, None, self.kernel, self.biasmult)


class LocalLinear(_LocalLayer):
    """
    One linear map per voxel and feature (neurite/tf/layers.py:777-808): `mult` and `bias` have the shape of one batch entry and
    call(x) = x * mult + bias, product and sum rounded separately as the reference's two ops are.  float32 only.
    """

    def __init__(self, initializer='RandomNormal', **kwargs):
        self.initializer = initializer
        super().__init__(**kwargs)
        self.mult = None
        self.bias = None

    def build(self, input_shape):
        dev = getattr(self, '_build_device', None)
        self.mult = nn.Parameter(_local_init('LocalLinear', self.initializer, input_shape[1:], dev))
        self.bias = nn.Parameter(_local_init('LocalLinear', self.initializer, input_shape[1:], dev))
        self.built = True

    def call(self, x):
        return _local_affine('LocalLinear', x, self.mult, self.bias, 1.0)


class _CrossLinearFn(torch.autograd.Function):
    """y[b, v, :] = x[b, v, :] @ W[v] (+ bias[v]) and its three gradients (csrc/local.hip)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        dev = x.device
        cin, cout = w.shape[-2], w.shape[-1]
        B, V = x.shape[0], x[0].numel() // cin
        y = torch.empty(tuple(x.shape[:-1]) + (cout,), dtype=torch.float32, device=dev)
        _lib.call(dev, 'nrt_local_cross_linear_f32', _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), B, V, cin, cout)
        ctx.save_for_backward(x, w)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dev = g.device
        g = g.contiguous()
        cin, cout = w.shape[-2], w.shape[-1]
        B, V = x.shape[0], x[0].numel() // cin
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.bias_shape is not None
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w) if need_w else None
        gb = torch.empty(ctx.bias_shape, dtype=torch.float32, device=dev) if need_b else None
        _lib.call(dev, 'nrt_local_cross_linear_bwd_f32', _lib.ptr(g), _lib.ptr(x), _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), B,
                  V, cin, cout)
        return gx, gw, gb


class LocalCrossLinear(_LocalLayer):
    """
    A different linear map between the features at every voxel (neurite/tf/layers.py:1535-1607): x [B, *space, Cin] ->
    [B, *space, output_features], y[b, v] = x[b, v] @ mult[0, v] (+ bias[0, v]); mult [1, *space, Cin, output_features], bias
    [1, *space, output_features], both drawn from N(1 / Cin, 0.01) unless an initializer is named.  The batch loop the reference maps
    with tf.map_fn runs inside the kernel, so a voxel's matrix is read once.  Limits (NotImplementedError): tensors that are not
    float32, more than 64 input or output features, a regularizer (there is no Keras loss collection here; the arguments are kept
    for introspection).
    """

    def __init__(self, output_features, mult_initializer=None, bias_initializer=None, mult_regularizer=None, bias_regularizer=None,
                 use_bias=True, **kwargs):
        self.output_features = output_features
        self.mult_initializer = mult_initializer
        self.bias_initializer = bias_initializer
        self.mult_regularizer = mult_regularizer
        self.bias_regularizer = bias_regularizer
        self.use_bias = use_bias
        if mult_regularizer is not None or bias_regularizer is not None:
            raise NotImplementedError('LocalCrossLinear: regularizers are not implemented (no Keras loss collection)')
        super().__init__(**kwargs)
        self.mult = None
        self.bias = None

    def build(self, input_shape):
        dev = getattr(self, '_build_device', None)
        cin = int(input_shape[-1])
        normal = (1.0 / cin, 0.01)                                                        # :1567-1570, 1579-1582
        if cin > 64 or int(self.output_features) > 64:
            raise NotImplementedError('LocalCrossLinear: up to 64 input and output features, got %d -> %d'
                                      % (cin, self.output_features))
        mult_shape = [1] + list(input_shape)[1:] + [self.output_features]
        self.mult = nn.Parameter(_local_init('LocalCrossLinear', self.mult_initializer, mult_shape, dev, normal))
        if self.use_bias:
            bias_shape = [1] + list(input_shape)[1:-1] + [self.output_features]
            self.bias = nn.Parameter(_local_init('LocalCrossLinear', self.bias_initializer, bias_shape, dev, normal))
        self.built = True

    def compute_output_shape(self, input_shape):
        return tuple(list(input_shape)[:-1] + [self.output_features])

    def call(self, x):
        _require_f32_local('LocalCrossLinear', x, self.mult, self.bias)
        _lib.require_device(x, self.mult, self.bias)
        if tuple(x.shape[1:]) != tuple(self.mult.shape[1:-1]) or x.dim() < 2:
            raise ValueError('LocalCrossLinear: input of shape %s, the layer was built for %s'
                             % (tuple(x.shape[1:]), tuple(self.mult.shape[1:-1])))
        if x.numel() < 1:
            raise ValueError('LocalCrossLinear: empty input of shape %s' % (tuple(x.shape),))
        x = x.contiguous()
        if torch.is_grad_enabled() and (x.requires_grad or self.mult.requires_grad
                                        or (self.bias is not None and self.bias.requires_grad)):
            return _CrossLinearFn.apply(x, self.mult, self.bias)
        return _CrossLinearFn.forward(_NoCtx(), x.detach(), self.mult.detach(), None if self.bias is None else self.bias.detach())


_local_param_uid = [0]


class LocalParamLayer(_Layer):
    """
    A learnable tensor as a layer without inputs (neurite/tf/layers.py:1711-1789; in Keras a source layer): the parameter `kernel`
    of shape `shape` is created at construction and forward() returns kernel[None] * mult, shape [1, *shape].  There is no input to
    build on, so the device comes from a `device=` keyword or from .to().  float32 only.
    """

    def __init__(self, shape, my_initializer='RandomNormal', dtype=None, name=None, mult=1.0, **kwargs):
        device = kwargs.pop('device', None)
        if not name:
            _local_param_uid[0] += 1
            name = 'local_param_%d' % _local_param_uid[0]
        if dtype not in (None, 'float32', torch.float32, np.float32):
            raise NotImplementedError('LocalParamLayer: float32 only, got dtype %r' % (dtype,))
        super().__init__(name=name, **kwargs)
        self.shape = [1, *shape]
        self.my_initializer = my_initializer
        self.mult = mult
        self.kernel = nn.Parameter(_local_init('LocalParamLayer', my_initializer, shape, device))
        self.trainable = True
        self.built = True

    def get_config(self):
        return {'dtype': 'float32', 'sparse': False, 'name': self.name}

    def compute_output_shape(self, input_shape=None):
        return tuple(self.shape)

    def forward(self, inputs=None):
        _require_f32_local('LocalParamLayer', self.kernel)
        _lib.require_device(self.kernel)
        if torch.is_grad_enabled() and self.kernel.requires_grad:
            return _LocalParamFn.apply(self.kernel, None, self.mult, 1)
        return _LocalParamFn.forward(_NoCtx(), self.kernel.detach(), None, self.mult, 1)

    call = forward


class LocalParamWithInput(_LocalLayer):
    """
    The learnable tensor of LocalParamLayer, repeated for every batch entry of an input that is otherwise ignored
    (neurite/tf/layers.py:1792-1844; the learnable atlas of the conditional-template models): output [B, *shape], entry b =
    e[b] * (kernel * mult) with e[b] = x.flatten(1)[b, 0] * 0 + 1 as at :1837-1841 -- so a NaN or Inf in that one element makes
    entry b NaN, as in the reference.  x gets no gradient, `kernel` does.  float32 only.
    """

    def __init__(self, shape, initializer='RandomNormal', mult=1.0, **kwargs):
        self.shape = shape
        self.initializer = initializer
        self.biasmult = mult
        import warnings
        warnings.warn('LocalParamWithInput: Consider using LocalParamLayer')
        super().__init__(**kwargs)
        self.kernel = None

    def get_config(self):
        config = super().get_config().copy()
        config.update({'shape': self.shape})
        return config

    def build(self, input_shape):
        self.kernel = nn.Parameter(_local_init('LocalParamWithInput', self.initializer, self.shape, getattr(self, '_build_device', None)))
        self.built = True

    def compute_output_shape(self, input_shape):
        return (input_shape[0], *self.shape)

    def call(self, x):
        _require_f32_local('LocalParamWithInput', x, self.kernel)
        _lib.require_device(x, self.kernel)
        if x.dim() < 1 or x.numel() < 1 or self.kernel.numel() < 1:
            raise ValueError('LocalParamWithInput: empty input of shape %s' % (tuple(x.shape),))
        probe = x.detach()                      # only element [b, 0, ..., 0] of every entry is read, through the batch stride
        B = x.shape[0]
        if torch.is_grad_enabled() and self.kernel.requires_grad:
            return _LocalParamFn.apply(self.kernel, probe, self.biasmult, B)
        return _LocalParamFn.forward(_NoCtx(), self.kernel.detach(), probe, self.biasmult, B)


def _get_training_value(layer, training):
    """neurite/tf/layers.py:2076-2096 with the module's mode in the place of the Keras learning phase"""
    if training is None:
        training = layer.training
    if isinstance(training, int):
        training = bool(training)
    if layer.trainable is False:
        training = False
    return training


class _StreamMeanFn(torch.autograd.Function):
    """MeanStream in training mode: `run` updates the buffers in place and returns (y, coef); d y / d x = coef (the assigned
    variables are not differentiated through)."""

    @staticmethod
    def forward(ctx, x, run):
        y, coef = run(x)
        ctx.save_for_backward(coef)
        return y

    @staticmethod
    def backward(ctx, g):
        coef, = ctx.saved_tensors
        dev = g.device
        g = g.contiguous()
        gx = torch.empty_like(g)
        _lib.call(dev, 'nrt_stream_mean_bwd_f32', _lib.ptr(g), _lib.ptr(coef), _lib.ptr(gx), g.shape[0], g[0].numel())
        return gx, None


class _StreamLayer(_LocalLayer):
    """what MeanStream and CovStream share: cap, the `trainable` flag (a layer that is not trainable always runs the inference
    branch), the persistent buffers `mean` and `count` (saved with the model, not parameters)."""

    def __init__(self, cap=100, **kwargs):
        self.cap = float(cap)
        trainable = kwargs.get('trainable', True)
        super().__init__(**kwargs)
        self.trainable = trainable
        self.register_buffer('mean', None)
        self.register_buffer('count', None)

    def _build_stats(self, input_shape):
        dev = getattr(self, '_build_device', None)
        self.mean = torch.zeros(tuple(int(s) for s in input_shape[1:]), dtype=torch.float32, device=dev)
        self.count = torch.zeros(1, dtype=torch.float32, device=dev)

    def _prepare(self, x):
        what = self.__class__.__name__
        _require_f32_local(what, x)
        dev = _lib.require_device(x, self.mean, self.count)
        if tuple(x.shape[1:]) != tuple(self.mean.shape):
            raise ValueError('%s: input of shape %s, the layer was built for %s' % (what, tuple(x.shape[1:]), tuple(self.mean.shape)))
        if x.numel() < 1:
            raise ValueError('%s: empty input of shape %s' % (what, tuple(x.shape)))
        return dev


class MeanStream(_StreamLayer):
    """
    Running mean of a stream of batches (neurite/tf/layers.py:1915-1975, _mean_update :2059-2073): in training mode `mean` and
    `count` are updated in place (every new batch weighs at least 1 / cap) and the output is min(1, count / cap) * mean repeated
    for every batch entry; in inference mode the stored statistics are used and nothing is updated.  call(x, training=None): None
    is the module's mode (train() / eval()), trainable=False forces the inference branch.  `count` stays on the device (no host
    round trip; the layer captures into a hipGraph).  Differentiable in x in training mode.  float32 only.
    """

    def __init__(self, cap=100, **kwargs):
        super().__init__(cap=cap, **kwargs)

    def build(self, input_shape):
        self._build_stats(input_shape)
        self.built = True

    def _run(self, x, training, dev):
        B, n = x.shape[0], self.mean.numel()
        y = torch.empty(x.shape, dtype=torch.float32, device=dev)
        coef = torch.empty(1, dtype=torch.float32, device=dev) if training else None
        _lib.call(dev, 'nrt_stream_mean_f32', _lib.ptr(x), _lib.ptr(self.mean), _lib.ptr(self.count), self.cap, _lib.ptr(y), _lib.ptr(coef),
                  B, n, int(training))
        return y, coef

    def call(self, x, training=None):
        training = _get_training_value(self, training)
        dev = self._prepare(x)
        x = x.contiguous()
        if training and torch.is_grad_enabled() and x.requires_grad:
            return _StreamMeanFn.apply(x, lambda t: self._run(t.detach(), True, dev))
        return self._run(x.detach(), bool(training), dev)[0]


class CovStream(_StreamLayer):
    """
    Running covariance of a stream of batches (neurite/tf/layers.py:1978-2056): x [B, *feat] is flattened to [B, v]; in training mode
    cov <- (cov * (min(count, cap) - 1) + sum_b x_b x_b^T) / (min(count, cap) + B - 1), `mean` and `count` as in MeanStream, and the
    output is min(1, count / cap) * cov for every batch entry, [B, v, v]; plain IEEE division, so the first call with B = 1 gives
    Inf / NaN as the reference does.  Inference mode reads the stored `cov`.  The gradient is not implemented: a training-mode call
    on an x that requires grad raises NotImplementedError (detach it).  float32 only.
    """

    def __init__(self, cap=100, **kwargs):
        super().__init__(cap=cap, **kwargs)
        self.register_buffer('cov', None)

    def build(self, input_shape):
        self._build_stats(input_shape)
        v = int(np.prod(input_shape[1:]))
        self.cov = torch.zeros((v, v), dtype=torch.float32, device=getattr(self, '_build_device', None))
        self.built = True

    def compute_output_shape(self, input_shape):
        v = int(np.prod(input_shape[1:]))
        return (input_shape[0], v, v)

    def call(self, x, training=None):
        training = _get_training_value(self, training)
        if training and torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError('CovStream: the gradient with respect to the input is not implemented; detach the input')
        dev = self._prepare(x)
        _lib.require_device(x, self.cov)
        x = x.detach().contiguous()
        B, v = x.shape[0], self.cov.shape[0]
        y = torch.empty((B, v, v), dtype=torch.float32, device=dev)
        _lib.call(dev, 'nrt_stream_cov_f32', _lib.ptr(x), _lib.ptr(self.mean), _lib.ptr(self.cov), _lib.ptr(self.count), self.cap,
                  _lib.ptr(y), B, v, int(bool(training)))
        return y


class _SampleNormalFn(torch.autograd.Function):
    """z = mu + exp(log_var / 2) * noise on nrt_add_act_affine_f32; d z / d mu = 1, d z / d log_var = exp(log_var / 2) * noise / 2"""

    @staticmethod
    def forward(ctx, mu, log_var, noise):
        from .models import _ACTS, _elementwise
        dev = mu.device
        half = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
        zero = torch.zeros(1, dtype=torch.float32, device=dev)
        with torch.no_grad():
            flat = lambda t: t.contiguous().view(-1, 1)                                    # (one "channel": the affine is a scalar)
            h = _elementwise(flat(log_var), scale=half, shift=zero)                       # log_var / 2, exact
            p = _elementwise(h, flat(noise), act=_ACTS['exponential'], mul=True)           # exp(.) * noise
            z = _elementwise(flat(mu), p)
        ctx.save_for_backward(p, half, zero)
        return z.view(mu.shape)

    @staticmethod
    def backward(ctx, g):
        from .models import _elementwise
        p, half, zero = ctx.saved_tensors
        glv = None
        if ctx.needs_input_grad[1]:
            glv = _elementwise(g.contiguous().view(-1, 1), p, scale=half, shift=zero, mul=True).view(g.shape)
        return (g if ctx.needs_input_grad[0] else None), glv, None


class SampleNormalLogVar(_Layer):
    """
    Gaussian sample given mean and log-variance (neurite/tf/layers.py:2261-2302): call([mu, log_var]) = mu + exp(log_var / 2) * noise
    with noise ~ N(0, 1) drawn by torch.randn on the device.  float32, differentiable in both inputs.  The arithmetic runs on the
    existing element-wise kernel (nrt_add_act_affine_f32, three launches: the halving, exp(.) * noise, the sum); no kernel of its own.
    `_noise=` (a tensor of mu's shape) replaces the draw, for tests and replays; the noise of the last call is kept as
    `last_draws['noise']`, as GaussianNoise does.
    """

    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    def compute_output_shape(self, input_shape):
        return input_shape[0]

    def call(self, x, _noise=None):
        mu, log_var = x
        _require_f32_local('SampleNormalLogVar', mu, log_var, _noise)
        dev = _lib.require_device(mu, log_var, _noise)
        if tuple(mu.shape) != tuple(log_var.shape):
            raise ValueError('SampleNormalLogVar: mu %s and log_var %s differ in shape' % (tuple(mu.shape), tuple(log_var.shape)))
        noise = torch.randn(mu.shape, dtype=torch.float32, device=dev) if _noise is None else _noise
        if tuple(noise.shape) != tuple(mu.shape):
            raise ValueError('SampleNormalLogVar: _noise %s, expected %s' % (tuple(noise.shape), tuple(mu.shape)))
        self.last_draws = dict(noise=noise)
        if torch.is_grad_enabled() and (mu.requires_grad or log_var.requires_grad):
            return _SampleNormalFn.apply(mu, log_var, noise)
        return _SampleNormalFn.forward(_NoCtx(), mu.detach(), log_var.detach(), noise)
