"""
Segmentation tools (neurite/tf/utils/seg.py:41-374): from the probability maps of overlapping patches to one label volume, on the four
kernels of csrc/seg.hip.

    labels = ne.seg.predict_volume(net, scan, (64, 64, 64), (32, 32, 32), batch_size=4)       # scan [X, Y, Z, C] on the device

The reference keeps every patch's probability map on the host in float64 and takes the arg-max and the vote at the end.  Here a
batch's probabilities are read once, straight after the network wrote them: what is kept per patch voxel is one int32 label (and one
float32 probability where it is asked for), and the vote is one gather pass over those (`quilt`).  Only `predict_volume_stack`, whose
contract is the stack itself, stores probabilities, in float32.

Tensors live on a ROCm device; CPU tensors are refused like everywhere else in the package.  Nothing but `prob_of_label` (its label
range check) and `recode` (its lookup table is built on the host and uploaded) touches the host: `pred_to_label`, `extract_patches` and
`quilt` capture into a graph.

The quilt semantics are a restatement: the reference calls pystrum's `patchlib.quilt`, which is not part of the reference tree
(DESIGN.md section 4.6e).  A volume element is the `nan_func` of the values of the patches that cover it, NaN where none does.
"""

import numpy as np
import torch

from . import _lib

__all__ = ['predict_volumes', 'predict_volume_stack', 'predict_volume', 'prob_of_label', 'pred_to_label', 'recode', 'extract_patches',
           'quilt']

_PRED_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16}
QUILT_MEAN, QUILT_MEDIAN = 0, 1


def _prod(values):
    return int(np.prod([int(v) for v in values], dtype=np.int64))


def _as_pred(x):
    """a probability map the kernels read as stored: float32 or bfloat16, contiguous; anything else is cast to float32"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(x).__name__)
    _lib.require_device(x)
    if x.dtype not in _PRED_DTYPES:
        x = x.to(torch.float32)
    return x.contiguous()


def _as_labels(x):
    """a label map the kernels read as stored: int32 or int64, contiguous"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(x).__name__)
    _lib.require_device(x)
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise IndexError('labels must be integers, got %s' % x.dtype)
    if x.dtype not in (torch.int32, torch.int64):
        x = x.to(torch.int64)
    return x.contiguous()


def _argmax(pred, labels=None, of=None, prob=None):
    """nrt_seg_argmax on pred [..., C]: fills `labels` (int32 / int64) and / or `prob` (float32), both of pred.shape[:-1] elements and
    contiguous; `of`: the labels whose probability is wanted (None: the arg-max's own)."""
    dev = pred.device
    C = int(pred.shape[-1])
    n = pred.numel() // max(C, 1)
    if n == 0 or C == 0:
        if C == 0:
            raise ValueError('attempt to get argmax of an empty sequence')
        return
    _lib.call(dev, 'nrt_seg_argmax', _lib.ptr(pred), _PRED_DTYPES[pred.dtype], n, C, _lib.ptr(labels),
              int(labels is not None and labels.dtype == torch.int64), _lib.ptr(of), int(of is not None and of.dtype == torch.int64),
              _lib.ptr(prob))


def pred_to_label(*y):
    """
    seg.py:296-301.  One int64 label tensor per argument: the index of the maximum over the last axis of a [..., C] map, with
    np.argmax's rules (the first index wins a tie, a NaN counts as the maximum, so the first NaN wins).
    """
    out = ()
    for f in y:
        f = _as_pred(f)
        lab = torch.empty(f.shape[:-1], dtype=torch.int64, device=f.device)
        _argmax(f, labels=lab)
        out += (lab,)
    return out


def prob_of_label(vol, labelvol):
    """
    seg.py:230-260.  vol [..., C] holds non-normalised probabilities, labelvol [...] one integer label per voxel; returns the float32
    tensor vol[v, labelvol[v]] / sum_c vol[v, c] in labelvol's shape (one pass over vol, float32 sum).

    The label range is checked once on the host (one aminmax, one synchronisation): a label outside [0, C) raises IndexError, negative
    labels included (NumPy would count those from the end).
    """
    vol, labelvol = _as_pred(vol), _as_labels(labelvol)
    _lib.require_device(vol, labelvol)
    nb_dims = labelvol.dim()
    if vol.dim() != nb_dims + 1:
        raise ValueError('prob_of_label: vol has %d axes, labelvol %d; vol needs one more (the labels)' % (vol.dim(), nb_dims))
    if tuple(vol.shape[:-1]) != tuple(labelvol.shape):
        raise IndexError('shape mismatch: vol %s and labelvol %s' % (tuple(vol.shape), tuple(labelvol.shape)))
    nb_labels = int(vol.shape[-1])
    out = torch.empty(labelvol.shape, dtype=torch.float32, device=vol.device)
    if labelvol.numel() == 0:
        return out
    lo, hi = (int(v) for v in torch.aminmax(labelvol))
    if lo < 0 or hi >= nb_labels:
        raise IndexError('index %d is out of bounds for axis 1 with size %d' % (lo if lo < 0 else hi, nb_labels))
    _argmax(vol, of=labelvol, prob=out)
    return out


def _recode_table(mapping, max_label):
    """the float32 lookup of recode (seg.py:338-352) from its three mapping forms"""
    if hasattr(mapping, 'mapping') and not isinstance(mapping, dict):
        mapping = mapping.mapping                       # a FreeSurfer-style table object carries its dict
    if isinstance(mapping, dict):
        keys = np.fromiter(mapping.keys(), dtype=np.int64, count=len(mapping))
        values = np.fromiter(mapping.values(), dtype=np.float32, count=len(mapping))
    elif isinstance(mapping, (list, tuple, np.ndarray)):
        keys = np.asarray(mapping, dtype=np.int64).reshape(-1)
        values = np.arange(1, keys.size + 1, dtype=np.float32)          # label l -> its place in the list, counted from 1
    else:
        raise ValueError('recode: mapping must be a list, a dict or an object with .mapping, got %s' % type(mapping).__name__)
    if keys.size == 0 and max_label is None:
        raise ValueError('recode: an empty mapping needs max_label')
    size = int(keys.max() if max_label is None else max_label) + 1
    table = np.zeros(size, dtype=np.float32)
    table[keys] = values                                # a key past max_label is an IndexError, as in the reference
    return table


def recode(seg, mapping, max_label=None):
    """
    seg.py:322-356.  out[v] = lookup[seg[v]] for an integer label tensor on the device; the result is float32 like the lookup.

    mapping:   {source label: target value}, an object whose `.mapping` is such a dict, or a sequence of source labels, the i-th of
               which maps to i + 1.  Labels the mapping does not name recode to 0.
    max_label: the lookup has max_label + 1 entries; None: the largest source label + 1.  A label of seg beyond the lookup (or
               negative) recodes to 0, which is what tf.gather gives on a GPU, and is never used as an index.

    The lookup is built on the host and uploaded (one small copy per call).
    """
    lookup = _recode_table(mapping, max_label)
    seg = _as_labels(seg)
    dev = seg.device
    out = torch.empty(seg.shape, dtype=torch.float32, device=dev)
    if seg.numel() == 0:
        return out
    table = torch.from_numpy(lookup).to(dev)
    _lib.call(dev, 'nrt_seg_recode', _lib.ptr(seg), int(seg.dtype == torch.int64), seg.numel(), _lib.ptr(table), table.numel(),
              _lib.ptr(out))
    return out


def _sizes(value, ndims, what):
    if isinstance(value, (int, np.integer)):
        value = (value,) * ndims
    value = tuple(int(v) for v in value)
    if len(value) != ndims:
        raise ValueError('%s has %d entries for %d dimensions' % (what, len(value), ndims))
    if any(v < 1 for v in value):
        raise ValueError('%s must be positive, got %s' % (what, (value,)))
    return value


def extract_patches(vol, patch_size, patch_stride, grid_size=None, start=0, count=None):
    """
    Patches of a channels-last volume.

    vol [*vol_shape, C] (1 to 3 spatial axes; float32 and bfloat16 are read as stored, anything else is cast to float32) ->
    [count, *patch_size, C]: the patches start .. start + count - 1 of the grid, patch n at unravel_index(n, grid_size) * patch_stride.
    grid_size None: every patch that fits, (vol_shape - patch_size) // patch_stride + 1 per axis.  count None: up to the last patch.
    """
    vol = _as_pred(vol)
    ndims = vol.dim() - 1
    if not 1 <= ndims <= 3:
        raise ValueError('extract_patches takes [*vol_shape, C] with 1 to 3 spatial axes, got %s' % (tuple(vol.shape),))
    shape = tuple(int(v) for v in vol.shape[:-1])
    patch, stride = _sizes(patch_size, ndims, 'patch_size'), _sizes(patch_stride, ndims, 'patch_stride')
    if any(p > v for p, v in zip(patch, shape)):
        raise ValueError('patch_size %s exceeds the volume %s' % (patch, shape))
    grid = tuple((v - p) // s + 1 for v, p, s in zip(shape, patch, stride)) if grid_size is None else _sizes(grid_size, ndims, 'grid_size')
    if any((g - 1) * s + p > v for g, s, p, v in zip(grid, stride, patch, shape)):
        raise ValueError('a grid of %s patches of %s at stride %s does not fit inside %s' % (grid, patch, stride, shape))
    total = _prod(grid)
    start = int(start)
    count = total - start if count is None else int(count)
    if start < 0 or count < 1 or start + count > total:
        raise ValueError('patches %d .. %d of a grid of %d' % (start, start + count - 1, total))
    C = int(vol.shape[-1])
    out = torch.empty((count,) + patch + (C,), dtype=vol.dtype, device=vol.device)
    if out.numel() == 0:
        return out
    dev = vol.device
    _lib.call(dev, 'nrt_patch_extract', _lib.ptr(vol), _PRED_DTYPES[vol.dtype], ndims, _lib.ints(shape), C, _lib.ints(patch),
              _lib.ints(stride), _lib.ints(grid), start, count, _lib.ptr(out))
    return out


def _reducer(nan_func):
    if nan_func is np.nanmean or nan_func == 'mean':
        return QUILT_MEAN
    if nan_func is np.nanmedian or nan_func == 'median':
        return QUILT_MEDIAN
    raise ValueError("nan_func must be np.nanmean, np.nanmedian, 'mean' or 'median', got %r" % (nan_func,))


def quilt(patches, patch_size, grid_size, patch_stride, nan_func=np.nanmean):
    """
    The inverse of extract_patches: a volume from the patches of a grid, overlapping patches reduced by `nan_func`.

    patches [N, *patch_size, C] with N = prod(grid_size) gives [*vol_shape, C]; [N, *patch_size], [N, prod(patch_size)] and
    [N, prod(patch_size), 1] are single-channel and give [*vol_shape]; vol_shape = (grid_size - 1) * patch_stride + patch_size.
    float32 and int32 are read as stored (int64 is narrowed to int32, anything else cast to float32; integers are exact below 2^23).
    The result is float32.

    nan_func: np.nanmean / 'mean' or np.nanmedian / 'median'.  An element is the reducer of the non-NaN values of the patches that
    cover it (read in ascending patch index; the mean is a float32 sum in that order, the median an exact selection with (a + b) / 2
    for an even count); NaN where no patch covers it (a stride larger than the patch) or every value is NaN.  The median takes up to
    64 covering patches per voxel, prod(ceil(patch_size / patch_stride)) <= 64.
    """
    if not isinstance(patches, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(patches).__name__)
    reduce = _reducer(nan_func)
    _lib.require_device(patches)
    patch = tuple(int(v) for v in np.atleast_1d(patch_size))
    ndims = len(patch)
    if not 1 <= ndims <= 3:
        raise ValueError('quilt takes patches of 1 to 3 spatial axes, got patch_size %s' % (patch,))
    patch, grid, stride = _sizes(patch, ndims, 'patch_size'), _sizes(grid_size, ndims, 'grid_size'), _sizes(patch_stride, ndims, 'patch_stride')
    N, pv = _prod(grid), _prod(patch)
    if patches.dim() < 1 or int(patches.shape[0]) != N:
        raise ValueError('quilt needs %d patches (grid %s), got a tensor of shape %s' % (N, grid, tuple(patches.shape)))
    with_channels = tuple(patches.shape[1:-1]) == patch and patches.dim() == ndims + 2
    C = int(patches.shape[-1]) if with_channels else 1
    if patches.numel() != N * pv * C:
        raise ValueError('patches of shape %s are not %d patches of %s' % (tuple(patches.shape), N, patch))
    if patches.dtype == torch.int64:
        patches = patches.to(torch.int32)
    elif patches.dtype not in (torch.float32, torch.int32):
        patches = patches.to(torch.float32)
    patches = patches.contiguous()
    if reduce == QUILT_MEDIAN and _prod(-(-p // s) for p, s in zip(patch, stride)) > 64:
        raise NotImplementedError('quilt: the median takes up to 64 covering patches per voxel; patch_size %s at patch_stride %s can '
                                  'reach %d' % (patch, stride, _prod(-(-p // s) for p, s in zip(patch, stride))))
    shape = tuple((g - 1) * s + p for g, s, p in zip(grid, stride, patch))
    dev = patches.device
    out = torch.empty(shape + ((C,) if with_channels else ()), dtype=torch.float32, device=dev)
    code = _lib.DT_F32 if patches.dtype == torch.float32 else _lib.DT_I32
    _lib.call(dev, 'nrt_patch_quilt', _lib.ptr(patches), code, ndims, _lib.ints(patch), _lib.ints(stride), _lib.ints(grid), C, reduce,
              _lib.ptr(out))
    return out


def _quilt(patches, patch_size, grid_size, patch_stride, verbose=False, **kwargs):
    """seg.py:363-374 in the reference's argument order: single-channel patches [N, ...] (flattened per patch) -> [*vol_shape].
    kwargs: nan_func_layers / nan_func_K, the names under which the reference hands its reducer to patchlib.quilt (there is one
    reducer here, so they must agree), or nan_func; the mean by default.  verbose is accepted and ignored."""
    if patches.dim() < 2:
        raise ValueError('_quilt takes [N, ...] patches, got shape %s' % (tuple(patches.shape),))
    known = ('nan_func_layers', 'nan_func_K', 'nan_func')
    unknown = sorted(set(kwargs) - set(known))
    if unknown:
        raise TypeError('_quilt got unexpected keyword arguments %s' % unknown)
    codes = {_reducer(kwargs[k]) for k in known if k in kwargs}
    if len(codes) > 1:
        raise NotImplementedError('_quilt: nan_func_layers and nan_func_K must name the same reducer')
    return quilt(patches.reshape(patches.shape[0], -1), patch_size, grid_size, patch_stride,
                 nan_func='median' if codes == {QUILT_MEDIAN} else 'mean')


def _run(model, inputs):
    """model.predict(inputs) where there is one, else model(inputs); an nn.Module runs under eval() and no_grad()"""
    if hasattr(model, 'predict'):
        return model.predict(inputs)
    if isinstance(model, torch.nn.Module):
        was = model.training
        if was:
            model.eval()
        try:
            with torch.no_grad():
                return model(inputs)
        finally:
            if was:
                model.train(True)
    return model(inputs)


def _patch_labels(pred, into, of=None, prob=None):
    """arg-max of pred [b, ..., C] into the int32 rows `into` [b, nb_vox] (and the probability of `of`, or of the arg-max, into prob)"""
    pred = _as_pred(pred)
    if pred.numel() // int(pred.shape[-1]) != into.numel():
        raise ValueError('a prediction of shape %s for %d patch voxels' % (tuple(pred.shape), into.numel()))
    _argmax(pred, labels=into, of=of, prob=prob)


def _to_int(vol):
    return vol.to(torch.int64)          # truncation, as .astype('int')


def _model_list(models):
    return tuple(models) if isinstance(models, (list, tuple)) else (models,)


def _generator_batches(models, data_generator, batch_size, grid_size):
    """Draws ceil(prod(grid_size) / batch_size) samples (inputs, y_true) and runs every model on each.  Yields
    (rows, used, vol_batch, prior_batch or None, y_true, [prediction per model]): `rows` is the slice of patch indices the batch fills
    and `used` its length -- the last batch may be only partly used, as in seg.py:197-201."""
    nb_patches = _prod(np.atleast_1d(grid_size))
    batch_size = int(batch_size)
    for start in range(0, nb_patches, batch_size):
        inputs, y_true = next(data_generator)[:2]
        with_prior = isinstance(inputs, (list, tuple))
        _lib.require_device(y_true)
        preds = []
        for model in models:
            pred = _run(model, inputs)
            if int(pred.shape[0]) != batch_size:
                raise ValueError('the model returned %d patches for a batch_size of %d' % (int(pred.shape[0]), batch_size))
            preds.append(pred)
        used = min(batch_size, nb_patches - start)
        yield (slice(start, start + used), used, inputs[0] if with_prior else inputs, inputs[1] if with_prior else None, y_true, preds)


def predict_volumes(models,
                    data_generator,
                    batch_size,
                    patch_size,
                    patch_stride,
                    grid_size,
                    nan_func=np.nanmedian,
                    do_extra_vol=False,
                    do_prob_of_true=False,
                    verbose=False):
    """
    seg.py:41-135: label volumes from a generator of patch batches.

    models:          one model or a list of them (a callable, or an object with .predict; a ConvNet runs under eval() and no_grad());
                     every model sees the same samples.
    data_generator:  yields (inputs, y_true): inputs [batch_size, *patch_size, 1], or [inputs, prior] with a prior
                     [batch_size, *patch_size, nb_labels]; y_true [batch_size, *patch_size, nb_labels]; device tensors, the patches of
                     the grid in C order.
    nan_func:        np.nanmedian / np.nanmean / 'median' / 'mean': how the labels (and probabilities) of overlapping patches are
                     reduced (`quilt`).
    do_extra_vol:    also return the quilted input (always a mean) and, with a prior, the prior's label volume.
    do_prob_of_true: with do_extra_vol, also return the quilted probability of the true label under the prediction (and the prior).
    verbose:         accepted and ignored.

    Returns, per model, the tuple (true_label, pred_label[, vol[, prior_label]][, pred_prob_of_true[, prior_prob_of_true]]); one such
    tuple for a single model, a tuple of them for several.  Label volumes are int64 (the float32 votes truncated, as .astype('int')
    does), the others float32.

    No probability stack is kept: per batch the arg-max -- and, where asked for, the probability of the true label in the same pass
    -- is taken while the probabilities are still the network's output; one int32 label (one float32 probability) per patch voxel is
    stored until the quilt.  What does not depend on the model (truth, input, prior) is computed once and shared by the entries.
    """
    models = _model_list(models)
    _reducer(nan_func)
    nb_patches = _prod(np.atleast_1d(grid_size))
    want_prob = bool(do_extra_vol and do_prob_of_true)
    shared, per_model = {}, [{} for _ in models]

    def rows(table, key, dtype, like, nb_vox):
        if key not in table:
            table[key] = torch.empty((nb_patches, nb_vox), dtype=dtype, device=like.device)
        return table[key]

    with_prior = False
    for sl, used, vol_batch, prior_batch, y_true, preds in _generator_batches(models, data_generator, batch_size, grid_size):
        y_true = _as_pred(y_true)
        nb_vox = _prod(y_true.shape[1:-1])
        with_prior = prior_batch is not None
        truth = rows(shared, 'true', torch.int32, y_true, nb_vox)[sl]
        _patch_labels(y_true[:used], truth)
        if do_extra_vol:
            rows(shared, 'vol', torch.float32, y_true, nb_vox)[sl] = vol_batch[:used].reshape(used, -1)
            if with_prior:
                _patch_labels(_as_pred(prior_batch)[:used], rows(shared, 'prior', torch.int32, y_true, nb_vox)[sl], of=truth if want_prob else None,
                              prob=rows(shared, 'prior_pp', torch.float32, y_true, nb_vox)[sl] if want_prob else None)
        for table, pred in zip(per_model, preds):
            _patch_labels(_as_pred(pred)[:used], rows(table, 'pred', torch.int32, y_true, nb_vox)[sl], of=truth if want_prob else None,
                          prob=rows(table, 'pp', torch.float32, y_true, nb_vox)[sl] if want_prob else None)

    def vote(patches, func=nan_func):
        return _quilt(patches, patch_size, grid_size, patch_stride, nan_func=func)

    common = {'true': _to_int(vote(shared['true']))}
    if do_extra_vol:
        common['vol'] = vote(shared['vol'], np.nanmean)
        if with_prior:
            common['prior'] = _to_int(vote(shared['prior']))
            if want_prob:
                common['prior_pp'] = vote(shared['prior_pp'])
    out = []
    for table in per_model:
        entry = [common['true'], _to_int(vote(table['pred']))]
        entry += [common[k] for k in ('vol', 'prior') if k in common]
        if want_prob:
            entry.append(vote(table['pp']))
            if with_prior:
                entry.append(common['prior_pp'])
        out.append(tuple(entry))
    return out[0] if len(out) == 1 else tuple(out)


def predict_volume_stack(models,
                         data_generator,
                         batch_size,
                         grid_size,
                         verbose=False):
    """
    seg.py:138-227: every patch of a grid through every model, kept as stacks.  Arguments as predict_volumes; batch_size need not
    divide the number of patches (the last batch is then partly used).

    Returns, per model, (all_true, all_pred, all_vol[, all_prior]): all_true / all_pred / all_prior [nb_patches, nb_vox, nb_labels]
    and all_vol [nb_patches, nb_vox], float32 on the device (the reference's are float64 on the host); one tuple for a single model,
    a tuple of them for several (all_true, all_vol and all_prior are then the same tensors in every entry).  This is the one contract
    that stores probabilities; predict_volumes does not go through it.
    """
    models = _model_list(models)
    nb_patches = _prod(np.atleast_1d(grid_size))
    stacks = {}

    def stack(key, like, width):
        if key not in stacks:
            stacks[key] = torch.zeros((nb_patches, width), dtype=torch.float32, device=like.device)
        return stacks[key]

    nb_vox = nb_labels = 0
    with_prior = False
    for sl, used, vol_batch, prior_batch, y_true, preds in _generator_batches(models, data_generator, batch_size, grid_size):
        nb_vox, nb_labels = _prod(y_true.shape[1:-1]), int(y_true.shape[-1])
        with_prior = prior_batch is not None
        stack('vol', y_true, nb_vox)[sl] = vol_batch[:used].reshape(used, -1)
        stack('true', y_true, nb_vox * nb_labels)[sl] = y_true[:used].reshape(used, -1)
        if with_prior:
            stack('prior', y_true, nb_vox * nb_labels)[sl] = prior_batch[:used].reshape(used, -1)
        for idx, pred in enumerate(preds):
            stack(('pred', idx), y_true, nb_vox * nb_labels)[sl] = pred[:used].reshape(used, -1)

    def maps(t):
        return t.view(nb_patches, nb_vox, nb_labels)
    out = []
    for idx in range(len(models)):
        entry = (maps(stacks['true']), maps(stacks[('pred', idx)]), stacks['vol'])
        out.append(entry + ((maps(stacks['prior']),) if with_prior else ()))
    return out[0] if len(out) == 1 else tuple(out)


def predict_volume(model, vol, patch_size, patch_stride, batch_size=1, nan_func=np.nanmedian, return_prob=False):
    """
    The label volume of a scan larger than the network's input.

    vol [*vol_shape, C] on the device (1 to 3 spatial axes); model: a callable (or an object with .predict) that maps a batch of patches
    [b, *patch_size, C] to probabilities [b, *patch_size, nb_labels] (float32 or bfloat16); a ConvNet runs under eval() and no_grad().
    patch_stride must tile the volume exactly, (vol_shape - patch_size) % patch_stride == 0 per axis, else ValueError.

    Per batch the patches are extracted on the device, the model runs, and one pass over its output leaves an int32 label per patch
    voxel (and, with return_prob, the probability of that label: its value over the sum of the voxel's channels).  The labels of
    overlapping patches are then reduced by nan_func (np.nanmedian / np.nanmean / 'median' / 'mean').

    Returns the int64 label volume [*vol_shape]; with return_prob, (labels, float32 probabilities [*vol_shape], reduced the same way).
    """
    if not isinstance(vol, torch.Tensor):
        raise TypeError('expected a torch.Tensor, got %s' % type(vol).__name__)
    _lib.require_device(vol)
    _reducer(nan_func)
    vol = _as_pred(vol)
    ndims = vol.dim() - 1
    if not 1 <= ndims <= 3:
        raise ValueError('predict_volume takes [*vol_shape, C] with 1 to 3 spatial axes, got %s' % (tuple(vol.shape),))
    shape = tuple(int(v) for v in vol.shape[:-1])
    patch, stride = _sizes(patch_size, ndims, 'patch_size'), _sizes(patch_stride, ndims, 'patch_stride')
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be positive, got %d' % batch_size)
    if any(p > v or (v - p) % s for v, p, s in zip(shape, patch, stride)):
        raise ValueError('patches of %s at stride %s do not tile a volume of %s exactly' % (patch, stride, shape))
    grid = tuple((v - p) // s + 1 for v, p, s in zip(shape, patch, stride))
    nb_patches, nb_vox = _prod(grid), _prod(patch)
    dev = vol.device
    labels = torch.empty((nb_patches, nb_vox), dtype=torch.int32, device=dev)
    probs = torch.empty((nb_patches, nb_vox), dtype=torch.float32, device=dev) if return_prob else None
    for start in range(0, nb_patches, batch_size):
        nb = min(batch_size, nb_patches - start)
        pred = _run(model, extract_patches(vol, patch, stride, grid, start, nb))
        _patch_labels(pred, labels[start:start + nb], prob=probs[start:start + nb] if return_prob else None)
    out = _to_int(_quilt(labels, patch, grid, stride, nan_func=nan_func))
    if return_prob:
        return out, _quilt(probs, patch, grid, stride, nan_func=nan_func)
    return out
