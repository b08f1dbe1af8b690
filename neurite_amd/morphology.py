"""
neurite_amd.morphology -- binary morphology, flat grey morphology and box rank filters on the device (csrc/morph.hip):
scipy.ndimage.binary_erosion / binary_dilation / binary_opening / binary_closing, minimum_filter / maximum_filter / grey_erosion /
grey_dilation / grey_opening / grey_closing and median_filter / rank_filter / percentile_filter without the copy of the volume to the
host and back.  The functions are exported from neurite_amd.utils.

Every result is an exact integer or order statistic.  Nothing travels to the host, so the calls capture into a graph; there are no
atomics and the results are bit-identical from run to run.  Nothing is differentiable: the results never require grad.
"""

import numpy as np
import torch

from . import _lib
from .deferred import materialize

__all__ = ['binary_erosion', 'binary_dilation', 'binary_opening', 'binary_closing', 'minimum_filter', 'maximum_filter', 'grey_erosion',
           'grey_dilation', 'grey_opening', 'grey_closing', 'median_filter', 'rank_filter', 'percentile_filter']

_MAX_LAST_EXTENT = 1024                     # csrc/morph_core.h: 16 words of 64 voxels per row
_MAX_FIRST_EXTENT = 524280                  # csrc/morph.hip: 65535 tiles of 8 rows in the grid's second dimension
_MAX_BOX = 31                               # csrc/morph.hip: kMmMaxSize
_MAX_SAMPLES = 27                           # csrc/morph.hip: kRkMaxSamples
_BINARY_DTYPES = {torch.bool: _lib.DT_U8, torch.uint8: _lib.DT_U8, torch.int32: _lib.DT_I32, torch.float32: _lib.DT_F32}
_FILTER_DTYPES = {torch.float32: _lib.DT_F32, torch.int32: _lib.DT_I32}
_MODES = {'reflect': 0, 'mirror': 1, 'nearest': 2, 'constant': 3}


# --------------------------------------------------------------------------------------
# checks on the host, before the device is looked at
# --------------------------------------------------------------------------------------

def _volume(x, batched, dtypes, what):
    """the tensor as [B, *S], checked against the limits every kernel of csrc/morph.hip shares"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(x).__name__))
    x = materialize(x).detach()
    if x.dtype not in dtypes:
        raise NotImplementedError('%s: a %s tensor, got %s' % (what, ' / '.join(str(d).replace('torch.', '') for d in dtypes), x.dtype))
    vol = x if batched else x.unsqueeze(0)
    nd = vol.dim() - 1
    if nd not in (2, 3):
        raise NotImplementedError('%s: 2 or 3 spatial axes%s, got shape %s' % (what, ' behind a batch axis' if batched else '',
                                                                              tuple(x.shape)))
    if any(int(v) < 1 for v in vol.shape):
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(x.shape)))
    if int(vol.shape[0]) > 65535 or int(np.prod(vol.shape, dtype=np.int64)) >= 2 ** 31:
        raise NotImplementedError('%s: up to 65535 batch entries and fewer than 2^31 voxels, got shape %s' % (what, tuple(vol.shape)))
    return vol


def _structure_bits(structure, nd, what):
    """None, a connectivity or a (3,) * nd array -> the 27-bit mask of csrc/morph_core.h (a 2-D structure in the plane dz = 0)"""
    if structure is None:
        structure = 1
    if isinstance(structure, (bool, np.bool_, str)):
        raise ValueError('%s: structure must be None, a connectivity 1 .. %d, an array of shape %s or \'ball\', got %r'
                         % (what, nd, (3,) * nd, structure))
    if isinstance(structure, (int, np.integer)):
        if not 1 <= int(structure) <= nd:
            raise ValueError('%s: a connectivity must be in 1 .. %d, got %d' % (what, nd, int(structure)))
        set_ = np.abs(np.indices((3,) * nd) - 1).sum(0) <= int(structure)          # scipy's generate_binary_structure
    else:
        if isinstance(structure, torch.Tensor):
            if structure.device.type != 'cpu':
                raise TypeError('%s: the structure is read on the host: an array-like or a CPU tensor, not a device tensor' % what)
            structure = structure.numpy()
        set_ = np.asarray(structure)
        if set_.shape != (3,) * nd:
            raise ValueError('%s: a structure for this input has shape %s, got %s' % (what, (3,) * nd, set_.shape))
        set_ = set_ != 0
    if nd == 2:
        full = np.zeros((3, 3, 3), dtype=bool)
        full[1] = set_
        set_ = full
    return int(sum(1 << i for i, v in enumerate(set_.reshape(-1)) if v))


def _iterations(iterations, what):
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)):
        raise ValueError('%s: iterations must be an int, got %r' % (what, iterations))
    if iterations < 1:
        raise NotImplementedError('%s: iterations >= 1; iterations < 1 (repeat until nothing changes) is not built, got %d'
                                  % (what, iterations))
    return int(iterations)


def _border(border_value, what):
    if isinstance(border_value, (bool, np.bool_, int, np.integer)) and int(border_value) in (0, 1):
        return int(border_value)
    raise ValueError('%s: border_value must be 0 or 1, got %r' % (what, border_value))


def _box(size, nd, what, max_samples=None):
    """an int or nd ints -> a tuple of nd odd sizes within the limits"""
    sizes = [size] * nd if np.ndim(size) == 0 else list(size)
    if np.ndim(size) > 1 or len(sizes) != nd:
        raise ValueError('%s: size must be an int or %d ints, got %r' % (what, nd, size))
    for v in sizes:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('%s: sizes must be positive ints, got %r' % (what, size))
        if v % 2 == 0:
            raise ValueError('%s: sizes must be odd (an even size shifts scipy\'s origin between erosion and dilation), got %r'
                             % (what, size))
    sizes = tuple(int(v) for v in sizes)
    if max_samples is None:
        if any(v > _MAX_BOX for v in sizes):
            raise NotImplementedError('%s: sizes up to %d, got %r' % (what, _MAX_BOX, size))
    elif int(np.prod(sizes, dtype=np.int64)) > max_samples:
        raise NotImplementedError('%s: a box of at most %d samples, got %r (%d samples)'
                                  % (what, max_samples, size, int(np.prod(sizes, dtype=np.int64))))
    return sizes


def _mode(mode, cval, dtype, what):
    if mode == 'wrap':
        raise NotImplementedError('%s: mode \'wrap\' is not built (reflect, mirror, nearest, constant)' % what)
    if not isinstance(mode, str) or mode not in _MODES:
        raise ValueError('%s: mode must be one of %s, got %r' % (what, ', '.join(sorted(_MODES)), mode))
    if isinstance(cval, (bool, str, torch.Tensor)) or not isinstance(cval, (int, float, np.integer, np.floating)) or cval != cval:
        raise ValueError('%s: cval must be a number (read on the host) and not NaN, got %r' % (what, cval))
    if dtype == torch.int32 and not -2 ** 31 <= cval < 2 ** 31:
        raise ValueError('%s: cval must fit the int32 input, got %r' % (what, cval))
    return _MODES[mode], float(cval)


# --------------------------------------------------------------------------------------
# binary morphology
# --------------------------------------------------------------------------------------

def _binary_pass(vol, bits, iterations, border, dilate, what):
    """nrt_binary_morph on vol [B, *S] (contiguous, on a device) -> bool [B, *S]"""
    dev = vol.device
    batch, spatial = int(vol.shape[0]), [int(v) for v in vol.shape[1:]]
    cshape = _lib.ints(spatial)
    out = torch.empty(vol.shape, dtype=torch.bool, device=dev)
    nws = int(_lib.lib().nrt_binary_morph_workspace_bytes(batch, cshape, len(spatial), iterations))
    ws = _lib.workspace(dev, nws) if nws else None
    _lib.call(dev, 'nrt_binary_morph', _lib.ptr(vol), _BINARY_DTYPES[vol.dtype], batch, cshape, len(spatial), bits, iterations, border,
              dilate, _lib.ptr(out), _lib.ptr(ws), nws, what=what)
    return out


def _ball_pass(vol, radius, dilate, what):
    """the Euclidean ball through the exact distance transform: a voxel is set by a dilation when a set voxel lies within `radius`,
    and kept by an erosion when no unset voxel does"""
    from .utils import _dist_trf
    r2 = float(radius) * float(radius)
    if dilate:
        return _dist_trf(vol, None, True, True, False, what) <= r2
    return _dist_trf(vol == 0, None, True, True, False, what) > r2


def _binary(x, structure, iterations, border_value, batched, radius, stages, what):
    vol = _volume(x, batched, _BINARY_DTYPES, what)
    nd = vol.dim() - 1
    ball = isinstance(structure, str) and structure == 'ball'
    if ball:
        if isinstance(radius, (bool, str)) or not isinstance(radius, (int, float, np.integer, np.floating)) or not 0 <= radius < np.inf:
            raise ValueError('%s: structure=\'ball\' needs a finite radius >= 0, got %r' % (what, radius))
        if _iterations(iterations, what) != 1:
            raise NotImplementedError('%s: structure=\'ball\' takes iterations=1 (a ball of radius r applied n times is not the ball of '
                                      'radius n r on a grid), got %d' % (what, iterations))
        if _border(border_value, what) != 0:
            raise NotImplementedError('%s: structure=\'ball\' does not look outside the volume (a dilation sees nothing set there, an '
                                      'erosion nothing unset): leave border_value at 0' % what)
    else:
        if radius is not None:
            raise ValueError('%s: radius goes with structure=\'ball\' only' % what)
        bits = _structure_bits(structure, nd, what)
        iterations, border = _iterations(iterations, what), _border(border_value, what)
        if int(vol.shape[-1]) > _MAX_LAST_EXTENT:
            raise NotImplementedError('%s: a last axis of up to %d voxels, got shape %s' % (what, _MAX_LAST_EXTENT, tuple(x.shape)))
        if nd == 3 and int(vol.shape[1]) > _MAX_FIRST_EXTENT:
            raise NotImplementedError('%s: a first spatial axis of up to %d voxels, got shape %s' % (what, _MAX_FIRST_EXTENT, tuple(x.shape)))
    _lib.require_device(vol)
    out = vol.contiguous()
    for dilate in stages:
        out = _ball_pass(out, radius, dilate, what) if ball else _binary_pass(out, bits, iterations, border, dilate, what)
    return out if batched else out[0]


def binary_erosion(input, structure=None, iterations=1, border_value=0, batched=False, radius=None):      # noqa: A002 (scipy's name)
    """
    scipy.ndimage.binary_erosion on the device: out[p] = AND over the set entries o of `structure` of m[p + o], m = (input != 0),
    applied `iterations` times; every voxel outside the volume holds `border_value`.  One voxel is one bit in the kernel
    (csrc/morph.hip): rows are packed by wave ballots straight into LDS and nothing packed reaches global memory.

    input:        bool, uint8, int32 or float32, [*S], or [B, *S] with batched=True; len(S) in {2, 3}; the last axis up to 1024 voxels
                  (the first of three up to 524280), B <= 65535, B * prod(S) < 2^31.  `!= 0` is evaluated in the kernel.
    structure:    None (connectivity 1), an int c in 1 .. len(S) (scipy's generate_binary_structure(len(S), c)), or an array-like of
                  shape (3,) * len(S) taken as it is (asymmetric, without its centre ...), read on the host; or 'ball' with
                  radius=r: the Euclidean ball, computed from the exact distance transform (`dist_trf`), which does not look outside
                  the volume and takes iterations=1, border_value=0.
    iterations:   an int >= 1.  scipy's iterations < 1 (until nothing changes) is not built: NotImplementedError.
    border_value: 0 or 1.
    Returns a bool tensor of input's shape.  scipy's origin, mask and output are not offered.
    """
    return _binary(input, structure, iterations, border_value, batched, radius, (0,), 'binary_erosion')


def binary_dilation(input, structure=None, iterations=1, border_value=0, batched=False, radius=None):     # noqa: A002
    """
    scipy.ndimage.binary_dilation on the device: out[p] = OR over the set entries o of `structure` of m[p - o] (the reflected
    structure).  Arguments, limits and result as `binary_erosion`.
    """
    return _binary(input, structure, iterations, border_value, batched, radius, (1,), 'binary_dilation')


def binary_opening(input, structure=None, iterations=1, border_value=0, batched=False, radius=None):      # noqa: A002
    """
    scipy.ndimage.binary_opening: `iterations` erosions, then `iterations` dilations, both with `border_value`.  Arguments, limits and
    result as `binary_erosion`.
    """
    return _binary(input, structure, iterations, border_value, batched, radius, (0, 1), 'binary_opening')


def binary_closing(input, structure=None, iterations=1, border_value=0, batched=False, radius=None):      # noqa: A002
    """
    scipy.ndimage.binary_closing: `iterations` dilations, then `iterations` erosions, both with `border_value`.  Arguments, limits and
    result as `binary_erosion`.
    """
    return _binary(input, structure, iterations, border_value, batched, radius, (1, 0), 'binary_closing')


# --------------------------------------------------------------------------------------
# flat grey morphology: the minimum / maximum over a box
# --------------------------------------------------------------------------------------

def _minmax(x, size, mode, cval, batched, stages, what):
    vol = _volume(x, batched, _FILTER_DTYPES, what)
    nd = vol.dim() - 1
    sizes = _box(size, nd, what)
    cmode, cval = _mode(mode, cval, vol.dtype, what)
    dev = _lib.require_device(vol)
    batch, spatial = int(vol.shape[0]), [int(v) for v in vol.shape[1:]]
    cshape, csize = _lib.ints(spatial), _lib.ints(sizes)
    nws = int(_lib.lib().nrt_minmax_filter_workspace_bytes(batch, cshape, nd, csize))
    ws = _lib.workspace(dev, nws) if nws else None
    out = vol.contiguous()
    for want_max in stages:
        src, out = out, torch.empty_like(out)
        _lib.call(dev, 'nrt_minmax_filter', _lib.ptr(src), _FILTER_DTYPES[vol.dtype], batch, cshape, nd, csize, cmode, cval, want_max,
                  _lib.ptr(out), _lib.ptr(ws), nws, what=what)
    return out if batched else out[0]


def minimum_filter(input, size=3, mode='reflect', cval=0.0, batched=False):                               # noqa: A002
    """
    scipy.ndimage.minimum_filter over a box, on the device: one running-minimum pass per axis whose size is above 1 (csrc/morph.hip).

    input: float32 or int32, [*S], or [B, *S] with batched=True; len(S) in {2, 3}, B <= 65535, B * prod(S) < 2^31.
    size:  an int or one int per spatial axis, each odd and in 1 .. 31 (an even size: ValueError).
    mode:  'reflect' (scipy's default: d c b a | a b c d | d c b a), 'mirror' (d c b | a b c d | c b a), 'nearest' or 'constant'
           (`cval`, converted to the input's dtype by truncation); 'wrap' is not built.  The fold is scipy's for a window wider than
           the axis too.
    Returns a tensor of input's shape and dtype.  +-inf and both zeros are ordinary values compared by value (-0.0 == 0.0: either may
    come back); the result at a window that holds a NaN is unspecified (scipy's own depends on the order of its visit).
    """
    return _minmax(input, size, mode, cval, batched, (0,), 'minimum_filter')


def maximum_filter(input, size=3, mode='reflect', cval=0.0, batched=False):                               # noqa: A002
    """scipy.ndimage.maximum_filter over a box.  Arguments, limits and result as `minimum_filter`."""
    return _minmax(input, size, mode, cval, batched, (1,), 'maximum_filter')


def grey_erosion(input, size=3, mode='reflect', cval=0.0, batched=False):                                 # noqa: A002
    """scipy.ndimage.grey_erosion by a flat box of odd sizes, which is `minimum_filter`.  Arguments, limits and result as there."""
    return _minmax(input, size, mode, cval, batched, (0,), 'grey_erosion')


def grey_dilation(input, size=3, mode='reflect', cval=0.0, batched=False):                                # noqa: A002
    """scipy.ndimage.grey_dilation by a flat box of odd sizes, which is `maximum_filter`.  Arguments, limits and result as there."""
    return _minmax(input, size, mode, cval, batched, (1,), 'grey_dilation')


def grey_opening(input, size=3, mode='reflect', cval=0.0, batched=False):                                 # noqa: A002
    """scipy.ndimage.grey_opening by a flat box: the erosion, then the dilation.  Arguments, limits and result as `minimum_filter`."""
    return _minmax(input, size, mode, cval, batched, (0, 1), 'grey_opening')


def grey_closing(input, size=3, mode='reflect', cval=0.0, batched=False):                                 # noqa: A002
    """scipy.ndimage.grey_closing by a flat box: the dilation, then the erosion.  Arguments, limits and result as `minimum_filter`."""
    return _minmax(input, size, mode, cval, batched, (1, 0), 'grey_closing')


# --------------------------------------------------------------------------------------
# order statistics over a box
# --------------------------------------------------------------------------------------

def _rank_call(x, size, which, mode, cval, batched, what):
    """which: the box's sample count N -> the rank"""
    vol = _volume(x, batched, _FILTER_DTYPES, what)
    nd = vol.dim() - 1
    sizes = _box(size, nd, what, max_samples=_MAX_SAMPLES)
    rank = which(int(np.prod(sizes)))
    cmode, cval = _mode(mode, cval, vol.dtype, what)
    dev = _lib.require_device(vol)
    src = vol.contiguous()
    out = torch.empty_like(src)
    _lib.call(dev, 'nrt_rank_filter', _lib.ptr(src), _FILTER_DTYPES[vol.dtype], int(vol.shape[0]), _lib.ints(vol.shape[1:]), nd,
              _lib.ints(sizes), rank, cmode, cval, _lib.ptr(out), what=what)
    return out if batched else out[0]


def median_filter(input, size=3, mode='reflect', cval=0.0, batched=False):                                # noqa: A002
    """
    scipy.ndimage.median_filter over a box of N = prod(size) <= 27 samples (3 x 3 x 3, 1 x 3 x 3, 3 x 3, 5 x 5, 1 x 5 x 5 ...), on the
    device: the sample of rank N // 2.  A block stages its tile and halo in LDS and every thread sorts its samples in registers by a
    fixed network of compare-exchanges (csrc/morph.hip).

    input: float32 or int32, [*S], or [B, *S] with batched=True; len(S) in {2, 3}, B <= 65535, B * prod(S) < 2^31.
    size:  an int or one int per spatial axis, each odd; more than 27 samples: NotImplementedError.
    mode, cval, zeros, infinities and NaNs: as `minimum_filter`.
    Returns a tensor of input's shape and dtype.
    """
    return _rank_call(input, size, lambda n: n // 2, mode, cval, batched, 'median_filter')


def rank_filter(input, rank, size=3, mode='reflect', cval=0.0, batched=False):                            # noqa: A002
    """
    scipy.ndimage.rank_filter over a box: the sample of rank `rank` (0 the smallest; a negative rank counts from the end, -1 the
    largest).  Other arguments, limits and result as `median_filter`.
    """
    what = 'rank_filter'
    if isinstance(rank, (bool, np.bool_)) or not isinstance(rank, (int, np.integer)):
        raise ValueError('%s: rank must be an int, got %r' % (what, rank))

    def which(n):
        k = int(rank) + n if rank < 0 else int(rank)
        if not 0 <= k < n:
            raise ValueError('%s: rank %d is outside the box of %d samples' % (what, rank, n))
        return k
    return _rank_call(input, size, which, mode, cval, batched, what)


def percentile_filter(input, percentile, size=3, mode='reflect', cval=0.0, batched=False):                # noqa: A002
    """
    scipy.ndimage.percentile_filter over a box of N samples: the sample of rank int(N * p / 100.0) for 0 <= p < 100 and N - 1 for
    p = 100, a negative percentile meaning p + 100 (scipy's rule: no interpolation).  Other arguments, limits and result as
    `median_filter`.
    """
    what = 'percentile_filter'
    if isinstance(percentile, (bool, str, torch.Tensor)) or not isinstance(percentile, (int, float, np.integer, np.floating)):
        raise ValueError('%s: percentile must be a number (read on the host), got %r' % (what, percentile))
    p = float(percentile)
    if p < 0.0:
        p += 100.0
    if not 0.0 <= p <= 100.0:
        raise ValueError('%s: percentile must be in -100 .. 100, got %r' % (what, percentile))
    return _rank_call(input, size, lambda n: n - 1 if p == 100.0 else int(n * p / 100.0), mode, cval, batched, what)
