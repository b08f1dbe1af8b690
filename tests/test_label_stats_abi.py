"""
CPU tests of the per-label statistics and the label confusion matrix (no kernel is launched): the entry points of csrc/labelstats.hip
are declared, typed and exported, and their section of the header brought no enumerator and no #define; every invalid argument is
refused with NRT_ERR_INVALID_ARG and every limit with NRT_ERR_UNSUPPORTED before any launch, the workspace check coming last; the
Python entry points (utils.label_stats, label_volumes, label_centroids, metrics.LabelOverlap, synthesis.intensity_priors) validate on
the host and refuse CPU tensors; and the restatement the GPU tests compare against (tests/label_stats_restatement.py, the definition
in NumPy) agrees with np.bincount and, where scipy imports, with scipy.ndimage.sum / center_of_mass / find_objects.
"""

import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import label_stats_restatement as R

ENTRY_POINTS = ['nrt_label_stats_workspace_bytes', 'nrt_label_stats', 'nrt_label_confusion_workspace_bytes', 'nrt_label_confusion_i32']
D = 16                                             # a non-NULL, 16-byte aligned "pointer"; nothing is launched on an argument error
BIG = 1 << 40


def _L():
    from neurite_amd import _lib
    return _lib


def _stats(ids=D, labels=D, nlabels=3, image=D, dtype=0, channels=2, batch=2, shape=(5, 6, 7), nd=None, counts=D, coord_sums=D, bbox=D,
           sums=D, minmax=D, ws=D, nws=BIG, shape_null=False):
    L = _L()
    return L.lib().nrt_label_stats(ids, labels, nlabels, image, dtype, channels, batch, None if shape_null else L.ints(shape),
                                   len(shape) if nd is None else nd, counts, coord_sums, bbox, sums, minmax, ws, nws, None)


def _conf(a=D, b=D, labels=D, nlabels=3, batch=2, voxels=210, counts=D, ws=D, nws=BIG):
    return _L().lib().nrt_label_confusion_i32(a, b, labels, nlabels, batch, voxels, counts, ws, nws, None)


def _bytes(batch=2, shape=(5, 6, 7), nd=None, nlabels=3, channels=2):
    L = _L()
    return L.lib().nrt_label_stats_workspace_bytes(batch, L.ints(shape), len(shape) if nd is None else nd, nlabels, channels)


def _conf_bytes(batch=2, voxels=210, nlabels=3):
    return _L().lib().nrt_label_confusion_workspace_bytes(batch, voxels, nlabels)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
    sigs = L.signatures()
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    assert sigs['nrt_label_stats'][2] == ['ids', 'labels', 'nlabels', 'image', 'dtype', 'channels', 'batch', 'shape', 'nd', 'counts',
                                          'coord_sums', 'bbox', 'sums', 'minmax', 'workspace', 'workspace_bytes', 'stream']
    args = dict(zip(sigs['nrt_label_stats'][2], sigs['nrt_label_stats'][1]))
    assert args['shape'] is ip and all(args[k] is vp for k in ('ids', 'labels', 'image', 'counts', 'coord_sums', 'bbox', 'sums', 'minmax'))
    assert args['workspace_bytes'] is C.c_size_t and sigs['nrt_label_stats'][0] is C.c_int
    assert sigs['nrt_label_stats_workspace_bytes'] == (C.c_size_t, [C.c_int, ip, C.c_int, C.c_int, C.c_int],
                                                       ['batch', 'shape', 'nd', 'nlabels', 'channels'])
    assert sigs['nrt_label_confusion_workspace_bytes'] == (C.c_size_t, [C.c_int, C.c_longlong, C.c_int], ['batch', 'voxels', 'nlabels'])
    assert sigs['nrt_label_confusion_i32'] == (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_longlong, vp, vp, C.c_size_t, vp],
                                               ['a', 'b', 'labels', 'nlabels', 'batch', 'voxels', 'counts', 'workspace',
                                                'workspace_bytes', 'stream'])


def test_the_header_gained_no_enumerator_and_no_define():
    L = _L()
    with open(L.HEADER_PATH) as f:
        text = f.read()
    start = text.index('Per-label region statistics')
    section = text[start:]
    assert all(name in section for name in ENTRY_POINTS)
    assert not re.search(r'^[ \t]*#[ \t]*define', section, flags=re.M) and 'enum' not in section
    names = re.findall(r'\bNRT_[A-Z0-9_]+', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert not [n for n in names if 'LABEL' in n or n.startswith('NRT_LS')]
    # options are plain ints and the image dtypes are the existing enumerators
    assert not any(hasattr(L, n) for n in ('LS_WANT_SUMS', 'LABEL_STATS', 'LS_DIRECT')) and (L.DT_F32, L.DT_BF16, L.DT_F16) == (0, 1, 2)


INVALID = ({'ids': None}, {'counts': None}, {'shape_null': True}, {'image': None}, {'image': None, 'minmax': None},
           {'image': None, 'sums': None}, {'dtype': 3}, {'dtype': 4}, {'dtype': -1}, {'dtype': 7}, {'batch': 0}, {'batch': -3},
           {'shape': (5, 0, 7)}, {'shape': (-1, 6)}, {'shape': (5, 6, 7, 8)}, {'shape': (9,)}, {'nd': 1}, {'nd': 4}, {'nd': 0},
           {'channels': 0}, {'channels': 5}, {'channels': -1}, {'nlabels': 0}, {'nlabels': 257}, {'nlabels': -4})


def test_invalid_arguments_are_refused_before_any_launch():
    L = _L()
    inv = L.NRT_ERR_INVALID_ARG
    for kw in INVALID:
        assert _stats(**kw) == inv, kw
        assert _stats(ws=None, nws=0, **kw) == inv, kw                                        # an argument error wins over the workspace
    # ... and over a limit
    assert _stats(batch=65536, nlabels=0) == inv
    assert _stats(shape=(1 << 30, 4), channels=9, ws=None, nws=0) == inv
    assert _stats(batch=0, shape=(1 << 20, 1 << 20), ws=None, nws=0) == inv
    assert _stats(shape=(1 << 20, 1 << 20, 0)) == inv
    # without an image the dtype and the channel count are not looked at
    ok = dict(image=None, sums=None, minmax=None, ws=None, nws=0)
    assert _stats(dtype=9, channels=77, **ok) == L.NRT_ERR_WORKSPACE
    for kw in ({'a': None}, {'b': None}, {'counts': None}, {'batch': 0}, {'batch': -1}, {'voxels': 0}, {'voxels': -5}, {'nlabels': 0},
               {'nlabels': 257}):
        assert _conf(**kw) == inv, kw
        assert _conf(ws=None, nws=0, **kw) == inv, kw
    assert _conf(batch=65536, voxels=4, nlabels=300) == inv
    for kw in ({'batch': 0}, {'shape': (5, 0, 7)}, {'shape': (5,)}, {'nd': 4}, {'nlabels': 0}, {'nlabels': 257}, {'channels': 5},
               {'channels': -1}):
        assert _bytes(**kw) == 0, kw
    for kw in ({'batch': 0}, {'voxels': 0}, {'nlabels': 0}, {'nlabels': 257}):
        assert _conf_bytes(**kw) == 0, kw


def test_limits_are_unsupported_and_the_workspace_comes_last():
    L = _L()
    unsup, ws = L.NRT_ERR_UNSUPPORTED, L.NRT_ERR_WORKSPACE
    limits = ({'batch': 65536, 'shape': (2, 1)}, {'batch': 2, 'shape': (1 << 10, 1 << 10, 1 << 10)}, {'batch': 1, 'shape': (1 << 16, 1 << 15)},
              {'batch': 2048, 'shape': (1 << 10, 1 << 10)}, {'batch': 3, 'shape': (1 << 30, 1 << 30, 4)})     # (the product does not wrap)
    for kw in limits:
        assert _stats(**kw) == unsup, kw
        assert _stats(ws=None, nws=0, **kw) == unsup, kw
        assert _stats(image=None, sums=None, minmax=None, labels=None, **kw) == unsup, kw
        assert _bytes(**kw) == 0, kw
        voxels = int(np.prod(kw['shape'], dtype=object))
        assert _conf(batch=kw['batch'], voxels=voxels) == unsup, kw
        assert _conf(batch=kw['batch'], voxels=voxels, ws=None, nws=0) == unsup, kw
        assert _conf_bytes(batch=kw['batch'], voxels=voxels) == 0, kw
    # just inside: every check but the workspace's passes, and nothing was launched
    inside = ({'batch': 1, 'shape': ((1 << 31) - 1, 1)}, {'batch': 65535, 'shape': (2, 1)}, {'batch': 1, 'shape': (1, 1, 1)},
              {'batch': 2, 'shape': (1 << 10, 1 << 10, (1 << 10) - 1)})
    for kw in inside:
        for dtype in (0, 1, 2):
            for channels in (1, 2, 3, 4):
                assert _stats(ws=None, nws=0, dtype=dtype, channels=channels, **kw) == ws, kw
        for nlabels in (1, 256):
            assert _stats(ws=None, nws=0, nlabels=nlabels, labels=None, coord_sums=None, bbox=None, sums=None, **kw) == ws, kw
            assert _conf(batch=kw['batch'], voxels=int(np.prod(kw['shape'], dtype=object)), nlabels=nlabels, ws=None, nws=0) == ws, kw


def test_missing_or_short_workspace_is_refused():
    L = _L()
    ws = L.NRT_ERR_WORKSPACE
    need = _bytes()
    # the sorted label list (256 ids and their slots) and per (entry, block) a float64 row of nlabels * channels * 2 partial sums
    assert need >= 2 * 256 * 4 + 2 * 3 * 2 * 2 * 8 and need % 16 == 0
    assert _bytes(channels=0) == 2 * 256 * 4 < _bytes(channels=1) < need < _bytes(channels=4)
    assert _bytes(batch=3) > need > _bytes(batch=1) and _bytes(nlabels=256) > _bytes(nlabels=4) > need
    assert _bytes(batch=1, shape=(160, 160, 160), nlabels=256, channels=4) > 100 * _bytes(batch=1, nlabels=256, channels=4)   # one row per block
    for kw in ({'ws': None, 'nws': 0}, {'ws': None, 'nws': BIG}, {'ws': 256, 'nws': need - 1}, {'ws': 24, 'nws': BIG}):
        assert _stats(**kw) == ws, kw
    assert _stats(channels=4, ws=256, nws=need) == ws
    need = _conf_bytes()
    assert need == 2 * 256 * 4 == _conf_bytes(batch=7, voxels=1 << 20, nlabels=256)
    for kw in ({'ws': None, 'nws': 0}, {'ws': None, 'nws': BIG}, {'ws': 256, 'nws': need - 1}, {'ws': 24, 'nws': BIG}):
        assert _conf(**kw) == ws, kw


def test_python_entry_points_are_public():
    import neurite_amd as ne
    for name in ('label_stats', 'label_volumes', 'label_centroids'):
        assert name in ne.utils.__all__ and callable(getattr(ne.utils, name))
        assert 'not differentiable' in getattr(ne.utils, name).__doc__.lower()
    assert 'LabelOverlap' in ne.metrics.__all__ and 'intensity_priors' in ne.synthesis.__all__
    assert list(inspect.signature(ne.utils.label_stats).parameters) == ['ids', 'image', 'labels', 'voxel_size', 'batched']
    assert list(inspect.signature(ne.utils.label_volumes).parameters) == ['ids', 'labels', 'voxel_size', 'batched']
    assert list(inspect.signature(ne.utils.label_centroids).parameters) == ['ids', 'labels', 'batched']
    assert list(inspect.signature(ne.synthesis.intensity_priors).parameters) == ['pairs', 'labels', 'channel']
    assert inspect.signature(ne.synthesis.intensity_priors).parameters['channel'].default == 0
    overlap = ne.metrics.LabelOverlap([0, 2035, 41, -7])
    assert overlap.labels == (0, 2035, 41, -7) and overlap.nb_labels == 4 and callable(overlap.confusion) and callable(overlap.scores)
    assert ne.metrics.LabelOverlap(5).labels is None and ne.metrics.LabelOverlap(5).nb_labels == 5


def _calls():
    import neurite_amd as ne
    u = ne.utils
    return (lambda t, **kw: u.label_stats(t, labels=4, **kw), lambda t, **kw: u.label_stats(t, labels=[3, 0, -7], **kw),
            lambda t, **kw: u.label_volumes(t, [1, 2], **kw), lambda t, **kw: u.label_centroids(t, 3, **kw))


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    ids = torch.zeros((5, 6, 7), dtype=torch.int32)
    for fn in _calls():
        for dtype in (torch.int32, torch.int64, torch.uint8, torch.bool):
            with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                fn(ids.to(dtype))
            with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                fn(ids.to(dtype), batched=True)
    for image in (torch.zeros((5, 6, 7)), torch.zeros((5, 6, 7, 3), dtype=torch.bfloat16), torch.zeros((5, 6, 7, 1), dtype=torch.float16)):
        with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
            ne.utils.label_stats(ids, image, labels=4)
    overlap = ne.metrics.LabelOverlap(4)
    for fn in (overlap.confusion, overlap.scores):
        with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
            fn(ids[None], ids[None].to(torch.int64))
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        ne.synthesis.intensity_priors([(torch.zeros((5, 6, 7)), ids)], [0, 1])


def test_host_side_argument_errors():
    import neurite_amd as ne
    u = ne.utils
    meta = torch.zeros((2, 5, 6, 7), dtype=torch.int32, device='meta')
    for fn in _calls():
        with pytest.raises(TypeError):
            fn(np.zeros((5, 6), np.int32))
        for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.complex64):
            with pytest.raises(NotImplementedError):
                fn(torch.zeros((5, 6), dtype=dtype, device='meta'))
        for shape in ((0, 4), (3, 0, 4)):
            with pytest.raises(ValueError):
                fn(torch.zeros(shape, dtype=torch.int32, device='meta'))
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 0, 4), dtype=torch.int32, device='meta'), batched=True)
        with pytest.raises(ValueError):
            fn(torch.zeros((), dtype=torch.int32, device='meta'), batched=True)
        for shape, batched in (((7,), False), ((2, 7), True), ((2, 3, 4, 5), False), ((2, 3, 4, 5, 6), True)):     # 1 or 4 spatial axes
            with pytest.raises(NotImplementedError):
                fn(torch.zeros(shape, dtype=torch.int32, device='meta'), batched=batched)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((65536, 2, 2), dtype=torch.int32, device='meta'), batched=True)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((2, 1 << 10, 1 << 10, 1 << 10), dtype=torch.int32, device='meta'), batched=True)         # 2^31 voxels
    # the label list
    for labels in (None, [], 0, -3, [1, 1], [0.5, 1], [2 ** 31], True):
        with pytest.raises(ValueError):
            u.label_stats(meta, labels=labels, batched=True)
    for labels in (257, list(range(257))):
        with pytest.raises(NotImplementedError):
            u.label_stats(meta, labels=labels, batched=True)
    # the image: a tensor of the id map's shape, with or without a channel axis of 1 to 4
    with pytest.raises(TypeError):
        u.label_stats(meta, np.zeros((2, 5, 6, 7), np.float32), labels=3, batched=True)
    for dtype in (torch.float64, torch.int32, torch.uint8):
        with pytest.raises(NotImplementedError):
            u.label_stats(meta, torch.zeros((2, 5, 6, 7), dtype=dtype, device='meta'), labels=3, batched=True)
    for shape in ((2, 5, 6), (2, 5, 6, 8), (5, 6, 7), (2, 5, 6, 7, 1, 1), (1, 2, 5, 6, 7)):
        with pytest.raises(ValueError):
            u.label_stats(meta, torch.zeros(shape, device='meta'), labels=3, batched=True)
    for channels in (0, 5, 32):
        with pytest.raises((NotImplementedError, ValueError)):
            u.label_stats(meta, torch.zeros((2, 5, 6, 7, channels), device='meta'), labels=3, batched=True)
    # the voxel size
    for voxel_size in (0, -1.0, float('nan'), float('inf'), [1, 2], [1, 2, 3, 4], [[1, 1, 1]], '1', [1, None, 1], True):
        with pytest.raises(ValueError):
            u.label_stats(meta, labels=3, voxel_size=voxel_size, batched=True)
        with pytest.raises(ValueError):
            u.label_volumes(meta, 3, voxel_size=voxel_size, batched=True)
    with pytest.raises(TypeError):
        u.label_stats(meta, labels=3, voxel_size=torch.ones(3), batched=True)
    # LabelOverlap
    for labels in (None, [], 0, [1, 1], [0.5]):
        with pytest.raises(ValueError):
            ne.metrics.LabelOverlap(labels)
    with pytest.raises(NotImplementedError):
        ne.metrics.LabelOverlap(257)
    overlap = ne.metrics.LabelOverlap([4, 2])
    for fn in (overlap.confusion, overlap.scores):
        with pytest.raises(TypeError):
            fn(np.zeros((2, 5), np.int32), np.zeros((2, 5), np.int32))
        for dtype in (torch.float32, torch.float64, torch.bfloat16):
            with pytest.raises(TypeError):
                fn(meta, meta.to(dtype))
            with pytest.raises(TypeError):
                fn(meta.to(dtype), meta)
        with pytest.raises(ValueError):
            fn(meta, meta[:, :4])
        with pytest.raises(ValueError):
            fn(meta[:, :0], meta[:, :0])
        with pytest.raises(ValueError):
            fn(meta[0, 0, 0], meta[0, 0, 0])
        big = torch.zeros((2, 1 << 10, 1 << 10, 1 << 10), dtype=torch.int32, device='meta')
        with pytest.raises(NotImplementedError):
            fn(big, big)
    # intensity_priors
    for kw in ({'labels': []}, {'labels': [1, 1]}, {'channel': -1}, {'channel': 0.5}, {'channel': True}):
        args = dict(pairs=[], labels=[0, 1], channel=0)
        args.update(kw)
        with pytest.raises(ValueError):
            ne.synthesis.intensity_priors(**args)
    with pytest.raises(ValueError):
        ne.synthesis.intensity_priors([], [0, 1])


# ---- the restatement against NumPy and scipy ---------------------------------------------------------------------------------------------
def test_restatement_equals_bincount_and_scipy():
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for shape in R.SHAPES[:4]:
        for kind in ('blobs', 'outside'):
            n = 7
            slots, ids, want = R.case(kind, shape, n, False)
            image = R.make_image(shape, 2, 'normal')
            full = R.stats(ids, image, slots)
            for key in ('count', 'coord_sums', 'bbox_min', 'bbox_max'):
                assert np.array_equal(full[key], want[key])
            for e in range(shape[0]):
                flat = ids[e].reshape(-1).astype(np.int64)
                inside = (flat >= 0) & (flat < n)
                assert np.array_equal(np.bincount(flat[inside], minlength=n)[:n], want['count'][e])
                for c in range(2):
                    x = image[e, ..., c].reshape(-1).astype(np.float64)
                    assert np.allclose(np.bincount(flat[inside], weights=x[inside], minlength=n)[:n], full['sum'][e, :, c], rtol=1e-12)
                if ndimage is None:
                    continue
                safe = np.where((ids[e] >= 0) & (ids[e] < n), ids[e], n).astype(np.int64)         # (scipy indexes with the ids)
                index = np.arange(n)
                assert np.allclose(ndimage.sum(image[e, ..., 0].astype(np.float64), safe, index), full['sum'][e, :, 0], rtol=1e-12)
                with np.errstate(invalid='ignore'):                                                # (an absent label: 0 / 0)
                    centres = np.asarray(ndimage.center_of_mass(np.ones(shape[1:]), safe, index))
                present = want['count'][e] > 0
                assert np.allclose(centres[present], want['coord_sums'][e][present] / want['count'][e][present, None], rtol=1e-12)
                boxes = ndimage.find_objects(safe + 1, max_label=n)                                # (label 0 is scipy's background)
                for l in range(n):
                    if not present[l]:
                        assert boxes[l] is None and tuple(want['bbox_min'][e, l]) == shape[1:] and np.all(want['bbox_max'][e, l] == -1)
                    else:
                        assert [s.start for s in boxes[l]] == list(want['bbox_min'][e, l])
                        assert [s.stop - 1 for s in boxes[l]] == list(want['bbox_max'][e, l])
            # the confusion matrix against bincount(a * (L + 1) + b)
            other = R.case('blobs' if kind == 'outside' else 'iid', shape, n, False)[1]
            table = R.confusion(ids, other, slots)
            for e in range(shape[0]):
                ia = np.where((ids[e] >= 0) & (ids[e] < n), ids[e], n).astype(np.int64).reshape(-1)
                ib = np.where((other[e] >= 0) & (other[e] < n), other[e], n).astype(np.int64).reshape(-1)
                assert np.array_equal(np.bincount(ia * (n + 1) + ib, minlength=(n + 1) ** 2).reshape(n + 1, n + 1), table[e])
                assert table[e].sum() == np.prod(shape[1:])


def test_restatement_conventions():
    ids = np.array([[[0, 0, 5], [2, 2, -7]]], np.int32)                                         # [1, 2, 3]
    image = np.array([[[1, np.nan, 4], [np.nan, np.nan, -0.0]]], np.float32)[..., None]
    got = R.stats(ids, image, [0, 2, 9, -7])
    assert got['count'].tolist() == [[2, 2, 0, 1]]
    assert got['coord_sums'].tolist() == [[[0, 1], [2, 1], [0, 0], [1, 2]]]
    assert got['bbox_min'].tolist() == [[[0, 0], [1, 0], [2, 3], [1, 2]]] and got['bbox_max'].tolist() == [[[0, 1], [1, 1], [-1, -1], [1, 2]]]
    assert np.isnan(got['sum'][0, 0, 0]) and np.isnan(got['sum'][0, 1, 0]) and got['sum'][0, 2, 0] == 0 and got['sum'][0, 3, 0] == 0
    assert got['min'][0, :, 0].tolist() == [1.0, np.inf, np.inf, 0.0] and got['max'][0, :, 0].tolist() == [1.0, -np.inf, -np.inf, 0.0]
    table = R.confusion(ids, ids[:, ::-1], [0, 2])
    assert table.tolist() == [[[0, 2, 0], [2, 0, 0], [0, 0, 2]]]
    for dtype in ('bfloat16', 'float16'):
        stored, back = R.store(R.make_image((1, 5, 13), None, 'normal'), dtype)
        assert stored.dtype.itemsize == 2 and back.dtype == np.float32 and np.abs(back - R.make_image((1, 5, 13), None, 'normal')).max() < 1.0
    assert R.slot_ids(4, True) == [0, 2035, 41, -7] and len(set(R.slot_ids(256, True))) == 256
    assert not set(R.slot_ids(256, True)) & set(R.OUTSIDE) and R.slot_ids(3, False) == [0, 1, 2]
