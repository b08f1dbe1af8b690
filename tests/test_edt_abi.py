"""
CPU tests of the distance transforms and surface distances (no kernel is launched): the entry points of csrc/edt.hip are declared,
typed and exported, refuse bad arguments before any launch and answer every limit with NRT_ERR_UNSUPPORTED; the Python entry points
(utils.dist_trf, signed_dist_trf, vol_to_sdt, vol_to_sdt_batch, label_dist_trf, metrics.SurfaceDistance, losses.SignedDistanceMSE)
validate on the host and refuse CPU tensors; and the restatement the GPU tests compare against (tests/edt_restatement.py, brute force by
definition) agrees bit for bit with scipy.ndimage where scipy imports: np.sqrt of the integer squared distance with
distance_transform_edt, and the neighbour-comparison surface with m & ~binary_erosion(m).
"""

import ctypes as C

import numpy as np
import pytest
import torch

import edt_restatement as R

ENTRY_POINTS = ['nrt_edt_workspace_bytes', 'nrt_edt_f32', 'nrt_surface_stats_workspace_bytes', 'nrt_surface_stats_f32']
D = 16                                             # a non-NULL, 8-byte aligned "pointer"; nothing is launched on an argument error
BIG = 1 << 40
# the fixed list of tests/test_gpu_edt.py; the scipy cross-checks take those with at least two axes longer than one voxel
SHAPES = [(1, 1, 1), (1, 7, 1), (5, 6, 7), (3, 65, 66), (130, 3, 5), (2, 2, 129), (17, 65), (64, 64), (1, 130)]
SCIPY_SHAPES = [s for s in SHAPES if sum(n > 1 for n in s) >= 2]


def _L():
    from neurite_amd import _lib
    return _lib


def _edt(mask=D, ids=None, labels=None, nlabels=1, batch=2, shape=(5, 6, 7), nd=None, sampling=None, flags=0, out=D, ws=D, nws=BIG,
         shape_null=False):
    L = _L()
    samp = (C.c_float * len(sampling))(*sampling) if sampling is not None else None
    return L.lib().nrt_edt_f32(mask, ids, labels, nlabels, batch, None if shape_null else L.ints(shape), len(shape) if nd is None else nd,
                               samp, flags, out, ws, nws, None)


def _ids(**kw):
    kw.setdefault('nlabels', 3)
    kw.setdefault('labels', D)
    return _edt(mask=None, ids=D, **kw)


def _stats(t=D, labels=D, nlabels=3, d2=D, batch=2, shape=(5, 6, 7), nd=None, stats=D, hist=D, nbins=78, ws=D, nws=BIG, shape_null=False):
    L = _L()
    return L.lib().nrt_surface_stats_f32(t, labels, nlabels, d2, batch, None if shape_null else L.ints(shape),
                                         len(shape) if nd is None else nd, stats, hist, nbins, ws, nws, None)


def _bytes(fn, batch=2, shape=(5, 6, 7), nd=None, channels=3):
    L = _L()
    return getattr(L.lib(), fn)(batch, L.ints(shape), len(shape) if nd is None else nd, channels)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
    assert (L.EDT_SURFACE, L.EDT_INVERT, L.EDT_SIGNED, L.EDT_SQUARED, L.EDT_ANY_OF) == (1, 2, 4, 8, 16)
    with open(L.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('SURFACE', 1), ('INVERT', 2), ('SIGNED', 4), ('SQUARED', 8), ('ANY_OF', 16)):
        assert '#define NRT_EDT_%s %d\n' % (name, value) in text


def test_invalid_arguments_are_refused_before_any_launch():
    L = _L()
    inv = L.NRT_ERR_INVALID_ARG
    for kw in ({'out': None}, {'shape_null': True}, {'mask': None}, {'ids': D, 'labels': D}, {'labels': D}, {'nlabels': 2},
               {'flags': L.EDT_SURFACE}, {'flags': L.EDT_ANY_OF}, {'flags': 32}, {'flags': -1}, {'batch': 0}, {'batch': -2},
               {'shape': (5, 0, 7)}, {'shape': (5, -6, 7)}, {'shape': (0, 6)}, {'sampling': (1.0, 0.0, 1.0)}, {'sampling': (1.0, -2.0, 1.0)},
               {'sampling': (1.0, float('nan'), 1.0)}, {'sampling': (float('inf'), 1.0, 1.0)}):
        assert _edt(**kw) == inv, kw
    for kw in ({'out': None}, {'labels': None}, {'flags': L.EDT_SURFACE | L.EDT_SIGNED}, {'batch': 0}, {'shape': (5, 0, 7)}):
        assert _ids(**kw) == inv, kw
    for kw in ({'t': None}, {'labels': None}, {'d2': None}, {'stats': None}, {'stats': 20}, {'shape_null': True}, {'nbins': 0},
               {'nbins': -3}, {'batch': 0}, {'shape': (5, 0, 7)}):
        assert _stats(**kw) == inv, kw
    for fn in ENTRY_POINTS[::2]:
        for kw in ({'batch': 0}, {'shape': (5, 0, 7)}):
            assert _bytes(fn, **kw) == 0, (fn, kw)
    # every flag combination that is allowed gets as far as the workspace check, which comes last: nothing was launched
    ws = L.NRT_ERR_WORKSPACE
    assert _edt(flags=L.EDT_SIGNED | L.EDT_SQUARED | L.EDT_INVERT, ws=None, nws=0) == ws
    assert _ids(flags=L.EDT_SIGNED | L.EDT_ANY_OF, ws=None, nws=0) == ws
    assert _stats(hist=None, nbins=0, ws=None, nws=0) == ws


def test_limits_are_unsupported():
    L = _L()
    unsup = L.NRT_ERR_UNSUPPORTED
    geometry = ({'shape': (7,), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 4}, {'shape': (5, 6, 7), 'nd': 0},
                {'shape': (1025, 2)}, {'shape': (2, 1025)}, {'shape': (2, 3, 1025)}, {'shape': (1 << 20, 2)},
                {'batch': 65536, 'shape': (2, 2)},
                {'batch': 2, 'shape': (1 << 10, 1 << 10, 1 << 10)},                        # 2^31 elements
                {'batch': 2048, 'shape': (1 << 10, 1 << 10)})                              # 2^31 elements
    for kw in geometry:
        assert _edt(**kw) == unsup, kw
        assert _ids(**kw) == unsup, kw
        assert _stats(**kw) == unsup, kw
        for fn in ENTRY_POINTS[::2]:
            assert _bytes(fn, **kw) == 0, (fn, kw)
    for n in (0, -1, 257, 1 << 20):
        assert _ids(nlabels=n) == unsup and _stats(nlabels=n) == unsup, n
        for fn in ENTRY_POINTS[::2]:
            assert _bytes(fn, channels=n) == 0
    # the label count is part of the element count: 2^22 voxels x 256 labels x 2 entries
    assert _ids(nlabels=256, batch=2, shape=(1 << 10, 1 << 10, 4)) == unsup
    # (with ANY_OF the output has one channel: the same call gets as far as the workspace check)
    assert _ids(nlabels=256, batch=2, shape=(1 << 10, 1 << 10, 4), flags=L.EDT_ANY_OF | L.EDT_SIGNED, ws=None, nws=0) == L.NRT_ERR_WORKSPACE
    # the histogram: more than 2^24 bins per label, or 2^31 bins in all
    assert _stats(nbins=(1 << 24) + 1) == unsup and _stats(batch=64, nlabels=256, nbins=1 << 17) == unsup
    # just inside
    assert _bytes(ENTRY_POINTS[0], batch=65535, shape=(2, 2), channels=1) == 65535 * 4 * 4
    assert _bytes(ENTRY_POINTS[0], batch=1, shape=(1024, 1024, 1024), channels=1) == 1 << 32
    assert _bytes(ENTRY_POINTS[0], batch=1, shape=(1024, 1024), channels=256) > 0
    assert _bytes(ENTRY_POINTS[2], batch=65535, shape=(2, 2), channels=1) > 0


def test_missing_or_short_workspace_is_refused():
    L = _L()
    ws = L.NRT_ERR_WORKSPACE
    need = _bytes(ENTRY_POINTS[0], channels=1)
    assert need == 2 * 5 * 6 * 7 * 4 and _bytes(ENTRY_POINTS[0], channels=3) == 3 * need
    for kw in ({'ws': None, 'nws': 0}, {'ws': None, 'nws': BIG}, {'ws': 256, 'nws': need - 1}, {'ws': 18, 'nws': BIG}):
        assert _edt(flags=L.EDT_SIGNED, **kw) == ws, kw
    assert _ids(flags=L.EDT_SIGNED, ws=256, nws=3 * need - 1) == ws
    need = _bytes(ENTRY_POINTS[2])
    assert need > 0
    for kw in ({'ws': None, 'nws': 0}, {'ws': None, 'nws': BIG}, {'ws': 256, 'nws': need - 1}):
        assert _stats(**kw) == ws, kw
    assert _bytes(ENTRY_POINTS[2], batch=3, shape=(9, 33, 34)) >= 3 * _bytes(ENTRY_POINTS[2], batch=1, shape=(9, 33, 34)) > 0


def test_python_entry_points_are_public():
    import neurite_amd as ne
    for name in ('dist_trf', 'signed_dist_trf', 'vol_to_sdt', 'vol_to_sdt_batch', 'label_dist_trf'):
        assert name in ne.utils.__all__ and callable(getattr(ne.utils, name))
    assert 'SurfaceDistance' in ne.metrics.__all__ and 'SignedDistanceMSE' in ne.losses.__all__
    sd = ne.metrics.SurfaceDistance([1, 2, 7])
    assert sd.labels == (1, 2, 7) and sd.percentile == 95.0 and sd.voxel_size is None
    assert all(callable(getattr(sd, k)) for k in ('distances', 'hausdorff', 'assd', 'hd95'))
    assert ne.losses.SignedDistanceMSE(1).foreground == (1,) and ne.losses.SignedDistanceMSE([1, 2], max_dist=5).max_dist == 5.0


def _entry_points():
    import neurite_amd as ne
    sd = ne.metrics.SurfaceDistance([1, 2])
    mse = ne.losses.SignedDistanceMSE([1])
    binary = (ne.utils.dist_trf, ne.utils.signed_dist_trf, ne.utils.vol_to_sdt, lambda t: ne.utils.dist_trf(t[None], batched=True),
              lambda t: ne.utils.vol_to_sdt_batch(t[None, ..., None]))
    labelled = (lambda t: ne.utils.label_dist_trf(t[None], [1, 2]), lambda t: ne.utils.label_dist_trf(t[None], [1], signed=True),
                lambda t: sd.distances(t[None], t[None]), lambda t: sd.hausdorff(t[None], t[None]), lambda t: sd.hd95(t[None], t[None]),
                lambda t: mse.loss(t[None], torch.zeros(t[None].shape + (1,))),
                lambda t: mse.loss(None, torch.stack([t.float(), t.float()], -1)[None] if isinstance(t, torch.Tensor) else t))
    return binary, labelled


def test_cpu_tensors_are_refused():
    L = _L()
    binary, labelled = _entry_points()
    for shape in ((5, 6, 7), (17, 65)):
        for fn in binary:
            for dtype in (torch.bool, torch.uint8, torch.int32, torch.float32):
                with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                    fn(torch.ones(shape).to(dtype))
        for fn in labelled:
            with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                fn(torch.ones(shape, dtype=torch.int32))
    import neurite_amd as ne
    both = ne.losses.multiple_losses_decorator([ne.losses.SignedDistanceMSE([1]).loss, ne.losses.SignedDistanceMSE([2], 3.0).loss], [1, 0.1])
    with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
        both(torch.ones(2, 5, 6, 7, dtype=torch.int32), torch.zeros(2, 5, 6, 7, 1))


def test_host_side_argument_errors():
    import neurite_amd as ne
    binary, labelled = _entry_points()
    for fn in binary + labelled:
        for shape in ((9,), (2, 3, 4, 5), (1025, 2), (2, 3, 1025)):                         # 1-D, 4-D, an extent above 1024
            with pytest.raises(NotImplementedError):
                fn(torch.zeros(shape, dtype=torch.int32))
        with pytest.raises(ValueError):
            fn(torch.zeros((5, 0, 7), dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(np.zeros((5, 6, 7), np.int32))
    for fn in labelled[:5]:
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((5, 6, 7), dtype=torch.float32))                                # ids are integers
    for fn in (ne.utils.dist_trf, ne.utils.signed_dist_trf):
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((65536, 2, 2), dtype=torch.uint8, device='meta'), batched=True)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((2048, 1024, 1024), dtype=torch.uint8, device='meta'), batched=True)        # 2^31 elements
        for sampling in ((1, 2), (1, 2, 3, 4), 0, -1.0, (1, float('nan'), 1), (1, float('inf'), 1)):
            with pytest.raises(ValueError):
                fn(torch.zeros((5, 6, 7), dtype=torch.uint8), sampling=sampling)
    meta = torch.zeros((2, 1024, 1024, 4), dtype=torch.int32, device='meta')
    with pytest.raises(NotImplementedError):
        ne.utils.label_dist_trf(meta, list(range(256)))                                    # 2^31 elements through the label count
    for labels in ([], list(range(257))):
        with pytest.raises(NotImplementedError):
            ne.utils.label_dist_trf(torch.zeros((2, 5, 6, 7), dtype=torch.int32), labels)
        with pytest.raises(NotImplementedError):
            ne.metrics.SurfaceDistance(labels)
    for labels in ([1, 1], [1.5], [1 << 31]):
        with pytest.raises(ValueError):
            ne.utils.label_dist_trf(torch.zeros((2, 5, 6, 7), dtype=torch.int32), labels)
        with pytest.raises(ValueError):
            ne.metrics.SurfaceDistance(labels)
        with pytest.raises(ValueError):
            ne.losses.SignedDistanceMSE(labels)
    for fn in (ne.utils.vol_to_sdt, ne.utils.vol_to_sdt_batch):
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((2, 5, 6, 1)), sdt_vol_resize=2)
    with pytest.raises(ValueError):
        ne.utils.vol_to_sdt_batch(torch.zeros((2, 5, 6, 7)))
    sd = ne.metrics.SurfaceDistance([1])
    with pytest.raises(ValueError):
        sd.distances(torch.zeros((2, 5, 6), dtype=torch.int32), torch.zeros((2, 5, 7), dtype=torch.int32))
    with pytest.raises(NotImplementedError):                                               # 5 x 256 x (2 x 1023^2 + 1) bins
        ne.metrics.SurfaceDistance(list(range(256))).distances(torch.zeros((5, 1024, 1024), dtype=torch.int32, device='meta'),
                                                               torch.zeros((5, 1024, 1024), dtype=torch.int32, device='meta'))
    for p in (-1, 101):
        with pytest.raises(ValueError):
            ne.metrics.SurfaceDistance([1], percentile=p)
    mse = ne.losses.SignedDistanceMSE([1])
    ids = torch.zeros((2, 5, 6, 7), dtype=torch.int32)
    for y_true, y_pred in ((None, torch.zeros(2, 5, 6, 7, 1)), (None, torch.zeros(2, 5, 6, 7, 3)), (ids, torch.zeros(2, 5, 6, 7, 2)),
                           (ids, torch.zeros(2, 5, 6, 8, 1)), (ids[..., None].expand(2, 5, 6, 7, 2), torch.zeros(2, 5, 6, 7, 1))):
        with pytest.raises(ValueError):
            mse.loss(y_true, y_pred)
    with pytest.raises(NotImplementedError):
        mse.loss(ids, torch.zeros(2, 5, 6, 7, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        ne.losses.SignedDistanceMSE([1], max_dist=0)
    # the missing key of an anisotropic result raises; any other missing key is a KeyError
    d = ne.metrics._SurfaceDistances(assd=1)
    with pytest.raises(NotImplementedError):
        d['hd_percentile']
    with pytest.raises(KeyError):
        d['nothing']


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------------
def test_restatement_equals_scipy_bit_for_bit():
    """executed wherever scipy imports (it does where this suite is developed); the definition needs no scipy"""
    ndi = pytest.importorskip('scipy.ndimage')
    checked = 0
    for shape in SCIPY_SHAPES:
        for density in (0.5, 0.02):
            m = R.feature_set(density, shape, seed=5)
            if not m.any():
                m[(0,) * len(shape)] = True
            d2 = R.sq_dist(m)
            want = ndi.distance_transform_edt(~m)                                          # VoxelMorph's dist_trf
            assert np.array_equal(np.sqrt(d2), want)
            assert np.array_equal(R.root32(d2), want.astype(np.float32))
            assert np.array_equal(R.surface(m), m & ~ndi.binary_erosion(m))
            # VoxelMorph's signed_dist_trf (on the balanced set: the complement of the sparse one costs the brute force most)
            if density == 0.5:
                assert not m.all()
                neg = ndi.distance_transform_edt(m)
                signed = np.where(m, -R.sq_dist(~m), d2)
                assert np.array_equal(R.root32(signed), (want * ~m - neg * m).astype(np.float32))
            if density == 0.02:                                                            # (and the sampling, on the cheaper set)
                for sampling in ((1.5, 1, 2)[:len(shape)], 0.75):
                    want = ndi.distance_transform_edt(~m, sampling=sampling)
                    assert np.allclose(np.sqrt(R.sq_dist(m, sampling)), want, rtol=1e-14, atol=0)
            checked += 1
    assert checked == 2 * len(SCIPY_SHAPES) == 12


def test_restatement_of_the_edge_cases_and_inputs():
    assert np.all(np.isposinf(R.sq_dist(np.zeros((3, 4), bool)))) and np.all(R.sq_dist(np.ones((3, 4), bool)) == 0)
    assert np.all(np.isposinf(R.signed_sq(np.zeros((3, 4), bool)))) and np.all(np.isneginf(R.signed_sq(np.ones((3, 4), bool))))
    assert np.array_equal(R.root32(np.array([-4.0, 9.0, np.inf, -np.inf])), np.array([-2, 3, np.inf, -np.inf], np.float32))
    # an extent of one: every voxel of the set lies at the border of the volume
    m = R.feature_set(0.5, (1, 7, 1), 1)
    assert np.array_equal(R.surface(m), m)
    m = np.ones((5, 5), bool)
    assert R.surface(m).sum() == 16 and not R.surface(m)[2, 2]
    assert R.feature_set('corners', (5, 6, 7)).sum() == 8 and R.feature_set('corners', (1, 7, 1)).sum() == 2
    assert R.feature_set('ball', (1, 1, 1)).all() and 0 < R.feature_set('ball', (17, 65)).mean() < 1
    ids = R.label_map((5, 6, 7), 4, 2)
    assert ids.dtype == np.int32 and ids.shape == (5, 6, 7) and set(np.unique(ids)) <= set(range(4))
    # the metric definitions on a case worked by hand: two 1-voxel surfaces 3 and 4 apart along the axes -> every distance is 5
    t, p = np.zeros((1, 8, 8), np.int32), np.zeros((1, 8, 8), np.int32)
    t[0, 1, 1], p[0, 4, 5] = 1, 1
    got = R.surface_metrics(t, p, [1, 2], percentiles=(0, 95, 100))
    assert got['hausdorff'][0, 0] == 5 and got['assd'][0, 0] == 5 and np.all(got['hd_percentile'][:, 0, 0] == 5)
    assert got['count_t'][0].tolist() == [1, 0] and np.isnan(got['hausdorff'][0, 1]) and np.all(np.isnan(got['hd_percentile'][:, 0, 1]))
    got = R.surface_metrics(t, p, [1], voxel_size=(2, 1), percentiles=(50,))
    assert got['max_tp'][0, 0] == np.sqrt(36 + 16)
