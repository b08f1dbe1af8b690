"""
CPU tests of connected-component labelling (no kernel is launched): the entry points of csrc/ccl.hip are declared, typed and exported
and the mode #defines are present; every invalid argument is refused with NRT_ERR_INVALID_ARG and every limit with NRT_ERR_UNSUPPORTED
before any launch, the workspace check coming last; the Python entry points (utils.connected_components, largest_component,
keep_largest_components, remove_small_components, fill_holes, metrics.ComponentCount, SynthStrip.brain_mask) validate on the host and
refuse CPU tensors; and the restatement the GPU tests compare against (tests/ccl_restatement.py, a flood fill by definition) agrees bit
for bit with scipy.ndimage.label and binary_fill_holes where scipy imports.
"""

import contextlib
import io

import numpy as np
import pytest
import torch

import ccl_restatement as R

ENTRY_POINTS = ['nrt_ccl_workspace_bytes', 'nrt_ccl_label_i32', 'nrt_ccl_select']
D = 16                                             # a non-NULL, 8-byte aligned "pointer"; nothing is launched on an argument error
BIG = 1 << 40


def _L():
    from neurite_amd import _lib
    return _lib


def _label(mask=D, ids=None, labels=None, nlabels=1, batch=2, shape=(5, 6, 7), nd=None, connectivity=1, comp=D, count=D, ws=D, nws=BIG,
           shape_null=False):
    L = _L()
    return L.lib().nrt_ccl_label_i32(mask, ids, labels, nlabels, batch, None if shape_null else L.ints(shape),
                                     len(shape) if nd is None else nd, connectivity, comp, count, ws, nws, None)


def _select(mask=D, ids=None, labels=None, nlabels=1, batch=2, shape=(5, 6, 7), nd=None, connectivity=1, mode=1, min_size=0, fill=0,
            table=D, out=D, ws=D, nws=BIG, shape_null=False):
    L = _L()
    return L.lib().nrt_ccl_select(mask, ids, labels, nlabels, batch, None if shape_null else L.ints(shape),
                                  len(shape) if nd is None else nd, connectivity, mode, min_size, fill, table, out, ws, nws, None)


def _as_ids(kw):
    kw = dict(kw)
    kw.setdefault('nlabels', 3)
    kw.setdefault('labels', D)
    kw.setdefault('ids', D)
    kw['mask'] = None
    return kw


def _bytes(batch=2, shape=(5, 6, 7), nd=None, nlabels=1):
    L = _L()
    return L.lib().nrt_ccl_workspace_bytes(batch, L.ints(shape), len(shape) if nd is None else nd, nlabels)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
    assert (L.CCL_LARGEST, L.CCL_MIN_SIZE, L.CCL_BORDER_FREE, L.CCL_INVERT) == (1, 2, 4, 8)
    with open(L.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('LARGEST', 1), ('MIN_SIZE', 2), ('BORDER_FREE', 4), ('INVERT', 8)):
        assert '#define NRT_CCL_%s %d\n' % (name, value) in text


GEOMETRY_INVALID = ({'shape_null': True}, {'batch': 0}, {'batch': -2}, {'shape': (5, 0, 7)}, {'shape': (5, -6, 7)}, {'shape': (0, 6)},
                    {'shape': (7,), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 1}, {'shape': (5, 6, 7), 'nd': 4}, {'shape': (5, 6, 7), 'nd': 0},
                    {'connectivity': 0}, {'connectivity': -1}, {'connectivity': 4}, {'shape': (5, 6), 'connectivity': 3})


def test_invalid_arguments_are_refused_before_any_launch():
    L = _L()
    inv = L.NRT_ERR_INVALID_ARG
    source = ({'mask': None}, {'ids': D, 'labels': D}, {'labels': D}, {'nlabels': 2}, {'nlabels': 0})
    for fn in (_label, _select):
        for kw in source + GEOMETRY_INVALID:
            assert fn(**kw) == inv, (fn.__name__, kw)
        for kw in ({'labels': None}, {'nlabels': 0}, {'nlabels': -1}, {'nlabels': 257}, {'nlabels': 1 << 20}, {'mask': D}) + GEOMETRY_INVALID:
            kw = _as_ids(kw) if 'mask' not in kw else dict(_as_ids(kw), mask=D)
            assert fn(**kw) == inv, (fn.__name__, kw)
    for kw in ({'comp': None}, {'count': None}):
        assert _label(**kw) == inv and _label(**_as_ids(kw)) == inv, kw
    for kw in ({'table': None, 'out': None}, {'mode': 16}, {'mode': -1}, {'mode': 1 | 32}, {'mode': L.CCL_MIN_SIZE, 'min_size': -1}):
        assert _select(**kw) == inv and _select(**_as_ids(kw)) == inv, kw
    assert _select(**_as_ids({'mode': L.CCL_INVERT | L.CCL_BORDER_FREE})) == inv      # the complement of an id map is no id map
    # an argument error wins over a limit and over the workspace
    assert _label(batch=0, shape=(1 << 15, 1 << 15, 4), ws=None, nws=0) == inv
    for kw in ({'batch': 0}, {'shape': (5, 0, 7)}, {'shape': (5, 6, 7), 'nd': 4}, {'nlabels': 0}, {'nlabels': 257}):
        assert _bytes(**kw) == 0, kw


def test_limits_are_unsupported_and_the_workspace_comes_last():
    L = _L()
    unsup, ws = L.NRT_ERR_UNSUPPORTED, L.NRT_ERR_WORKSPACE
    limits = ({'batch': 2, 'shape': (1 << 10, 1 << 10, 1 << 10)},                     # 2^31 voxels
              {'batch': 2048, 'shape': (1 << 10, 1 << 10)},                           # 2^31 voxels
              {'batch': 1, 'shape': (1 << 16, 1 << 15)},                              # 2^31 voxels in one entry
              {'batch': 1, 'shape': (1 << 20, 1 << 20, 1 << 20)},                     # (the product does not wrap)
              {'batch': 65536, 'shape': (2, 2)})
    for kw in limits:
        for fn in (_label, _select):
            assert fn(**kw) == unsup, kw
            assert fn(ws=None, nws=0, **kw) == unsup, kw
            assert fn(**_as_ids(kw)) == unsup, kw
        assert _bytes(**kw) == 0, kw
    # just inside: every check but the workspace's passes, and nothing was launched
    inside = ({'batch': 1, 'shape': (1 << 10, 1 << 10, (1 << 11) - 1)}, {'batch': 65535, 'shape': (2, 2)}, {'shape': (1, 1, 1)},
              {'shape': (5, 6), 'connectivity': 2}, {'connectivity': 3})
    for kw in inside:
        for fn in (_label, _select):
            assert fn(ws=None, nws=0, **kw) == ws, kw
            assert fn(ws=None, nws=0, **_as_ids(dict(kw, nlabels=256))) == ws, kw
    for mode in range(16):
        assert _select(mode=mode, min_size=7, fill=-3, ws=None, nws=0) == ws
        if not mode & L.CCL_INVERT:
            assert _select(**_as_ids({'mode': mode, 'ws': None, 'nws': 0})) == ws
    assert _select(table=None, ws=None, nws=0) == ws and _select(out=None, mode=0, ws=None, nws=0) == ws


def test_missing_or_short_workspace_is_refused():
    L = _L()
    ws = L.NRT_ERR_WORKSPACE
    need = _bytes()
    # parent and size words per voxel, one count per chunk and entry, and per (entry, slot) a count and a 64-bit maximum
    assert need >= 2 * 5 * 6 * 7 * 2 * 4 + 2 * 4 + 2 * 12 and need % 8 == 0
    assert _bytes(nlabels=3) >= need + 2 * 2 * 12 - 8
    assert _bytes(batch=3, shape=(9, 33, 34)) >= 3 * _bytes(batch=1, shape=(9, 33, 34)) - 16 > 0
    assert _bytes(batch=1, shape=(1 << 10, 1 << 10, (1 << 11) - 1)) > 1 << 33                  # (size_t, not int)
    for kw in ({'ws': None, 'nws': 0}, {'ws': None, 'nws': BIG}, {'ws': 256, 'nws': need - 1}, {'ws': 20, 'nws': BIG}):
        assert _label(**kw) == ws and _select(**kw) == ws, kw
    assert _label(**_as_ids({'ws': 256, 'nws': _bytes(nlabels=3) - 1})) == ws


def test_python_entry_points_are_public():
    import neurite_amd as ne
    for name in ('connected_components', 'largest_component', 'keep_largest_components', 'remove_small_components', 'fill_holes'):
        assert name in ne.utils.__all__ and callable(getattr(ne.utils, name))
        assert 'differentiable' in getattr(ne.utils, name).__doc__
    assert 'ComponentCount' in ne.metrics.__all__
    cc = ne.metrics.ComponentCount([1, 2, 7], connectivity=2)
    assert cc.labels == (1, 2, 7) and cc.connectivity == 2 and ne.metrics.ComponentCount([4]).connectivity == 1
    assert all(callable(getattr(cc, k)) for k in ('counts', 'largest', 'extra'))
    assert callable(ne.models.SynthStrip.brain_mask) and 'restated, not recorded' in ne.models.SynthStrip.brain_mask.__doc__


def _entry_points():
    import neurite_amd as ne
    cc = ne.metrics.ComponentCount([1, 2])
    masks = (ne.utils.connected_components, ne.utils.largest_component, ne.utils.fill_holes,
             lambda t: ne.utils.remove_small_components(t, 3), lambda t: ne.utils.fill_holes(t[None], batched=True),
             lambda t: ne.utils.connected_components(t, connectivity=2))
    labelled = (lambda t: ne.utils.connected_components(t, labels=[1, 2]), lambda t: ne.utils.keep_largest_components(t, [1, 2]),
                lambda t: ne.utils.remove_small_components(t, 3, labels=[2]), lambda t: cc.counts(t[None]), lambda t: cc.largest(t[None]),
                lambda t: cc.extra(t[None]))
    return masks, labelled


def test_cpu_tensors_are_refused():
    L = _L()
    masks, labelled = _entry_points()
    for shape in ((5, 6, 7), (17, 65)):
        for fn in masks:
            for dtype in (torch.bool, torch.uint8, torch.int32, torch.float32):
                with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                    fn(torch.ones(shape).to(dtype))
        for fn in labelled:
            with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
                fn(torch.ones(shape, dtype=torch.int32))
    import neurite_amd as ne
    with contextlib.redirect_stdout(io.StringIO()):
        model = ne.models.SynthStrip((16, 16, 16), [0, 1, 2, 3], {1: 1, 2: 1, 3: 1}, nb_unet_features=4, nb_unet_levels=2)
    with pytest.raises((L.NeuriteAmdError, RuntimeError)):
        model.brain_mask(torch.zeros(1, 16, 16, 16))
    for bad in (torch.zeros(1, 16, 16, 15), torch.zeros(16, 16, 16), torch.zeros(1, 16, 16, 16, 2)):
        with pytest.raises(ValueError):
            model.brain_mask(bad)
    with pytest.raises(TypeError):
        model.brain_mask(np.zeros((1, 16, 16, 16), np.float32))


def test_host_side_argument_errors():
    import neurite_amd as ne
    masks, labelled = _entry_points()
    for fn in masks + labelled:
        for shape in ((9,), (2, 3, 4, 5)):                                                   # 1-D, 4-D
            with pytest.raises(NotImplementedError):
                fn(torch.zeros(shape, dtype=torch.int32))
        with pytest.raises(ValueError):
            fn(torch.zeros((5, 0, 7), dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(np.zeros((5, 6, 7), np.int32))
    for fn in labelled:
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((5, 6, 7), dtype=torch.float32))                                # ids are integers
    x = torch.zeros((5, 6, 7), dtype=torch.uint8)
    for connectivity in (0, 4, -1, 1.5, True):
        for fn in (ne.utils.connected_components, ne.utils.largest_component, ne.utils.fill_holes):
            with pytest.raises(ValueError):
                fn(x, connectivity)
        with pytest.raises(ValueError):
            ne.metrics.ComponentCount([1], connectivity)
    with pytest.raises(ValueError):
        ne.utils.fill_holes(x[0], 3)                                                       # connectivity 3 of a 2-D mask
    with pytest.raises(ValueError):
        ne.metrics.ComponentCount([1], 3).counts(torch.zeros((2, 5, 6), dtype=torch.int32))
    for fn in (ne.utils.connected_components, ne.utils.fill_holes):
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((65536, 2, 2), dtype=torch.uint8, device='meta'), batched=True)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((2048, 1024, 1024), dtype=torch.uint8, device='meta'), batched=True)        # 2^31 voxels
        with pytest.raises(NotImplementedError):
            fn(torch.zeros((5, 6, 7), dtype=torch.complex64))
    ids = torch.zeros((2, 5, 6, 7), dtype=torch.int32)
    for labels in ([], list(range(257))):
        with pytest.raises(NotImplementedError):
            ne.utils.connected_components(ids, labels=labels, batched=True)
        with pytest.raises(NotImplementedError):
            ne.utils.keep_largest_components(ids, labels, batched=True)
        with pytest.raises(NotImplementedError):
            ne.metrics.ComponentCount(labels)
    for labels in ([1, 1], [1.5], [1 << 31]):
        with pytest.raises(ValueError):
            ne.utils.connected_components(ids, labels=labels, batched=True)
        with pytest.raises(ValueError):
            ne.utils.remove_small_components(ids, 2, labels=labels, batched=True)
        with pytest.raises(ValueError):
            ne.metrics.ComponentCount(labels)
    with pytest.raises(ValueError):
        ne.utils.keep_largest_components(ids, None, batched=True)
    for min_size in (-1, 2.5, 1 << 31, True):
        with pytest.raises(ValueError):
            ne.utils.remove_small_components(x, min_size)
    for fill in (1.5, 1 << 31, True):
        with pytest.raises(ValueError):
            ne.utils.keep_largest_components(ids, [1], fill=fill, batched=True)
        with pytest.raises(ValueError):
            ne.utils.remove_small_components(ids, 2, labels=[1], fill=fill, batched=True)


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------------
def _scipy_ids(ndi, ids, labels, connectivity):
    """label each id's mask with scipy, then renumber by first voxel"""
    st = ndi.generate_binary_structure(ids.ndim, connectivity)
    firsts, maps = [], []
    for lab in labels:
        comp, n = ndi.label(ids == lab, st)
        flat = comp.reshape(-1)
        for k in range(1, n + 1):
            firsts.append(int(np.flatnonzero(flat == k)[0]))
            maps.append(comp == k)
    out = np.zeros(ids.shape, np.int32)
    for number, i in enumerate(np.argsort(firsts), 1):
        out[maps[i]] = number
    return out, len(firsts)


def test_restatement_equals_scipy_bit_for_bit():
    """executed wherever scipy imports (it does where this suite is developed); the definition needs no scipy"""
    ndi = pytest.importorskip('scipy.ndimage')
    checked = 0
    for shape in R.SHAPES:
        nd = len(shape)
        for connectivity in range(1, nd + 1):
            st = ndi.generate_binary_structure(nd, connectivity)
            for density in (0, 0.3, 0.5, 0.7, 1):
                m = np.random.default_rng(5).random(shape) < density
                want, n = ndi.label(m, st, output=np.int32)
                got, count = R.label(m.astype(np.uint8), connectivity)
                assert count == n and got.dtype == np.int32 and np.array_equal(got, want), (shape, connectivity, density)
                assert np.array_equal(R.fill_holes(m, connectivity), ndi.binary_fill_holes(m, st)), (shape, connectivity, density)
                if n:
                    sizes = np.bincount(want.reshape(-1))
                    sizes[0] = 0
                    assert np.array_equal(R.keep(m, connectivity, largest=True), want == np.argmax(sizes))
                    assert np.array_equal(R.keep(m, connectivity, min_size=3), (sizes >= 3)[want] & m)
                checked += 1
            if int(np.prod(shape)) <= 2000:                                                # (the per-component loop of the scipy side)
                ids = R.random_ids(shape, 4, seed=6)
                for labels in ([1, 2, 3], [3, 0]):
                    want, n = _scipy_ids(ndi, ids, labels, connectivity)
                    got, count = R.label(ids, connectivity, labels)
                    assert count == n and np.array_equal(got, want), (shape, connectivity, labels)
    assert checked == 5 * sum(len(s) for s in R.SHAPES)


def test_restatement_of_the_edge_cases_and_patterns():
    assert R.offsets(2, 1) == [(-1, 0), (0, -1), (0, 1), (1, 0)] and [len(R.offsets(3, c)) for c in (1, 2, 3)] == [6, 18, 26]
    assert len(R.offsets(2, 2)) == 8
    m = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], np.uint8)
    assert R.label(m, 1)[1] == 5 and R.label(m, 2)[1] == 1
    assert np.array_equal(R.label(m, 1)[0], np.array([[1, 0, 2], [0, 3, 0], [4, 0, 5]]))
    # equal ids only: two touching structures stay two components
    ids = np.array([[1, 1, 2, 2], [0, 1, 2, 9]], np.int32)
    comp, n = R.label(ids, 1, [2, 1])
    assert n == 2 and np.array_equal(comp, np.array([[1, 1, 2, 2], [0, 1, 2, 0]]))
    assert np.array_equal(R.table(ids, 1, [2, 1, 5]), np.array([[1, 3], [1, 3], [0, 0]]))
    assert np.array_equal(R.select_ids(ids, [1, 2], 1, fill=-1, min_size=4), np.array([[-1, -1, -1, -1], [0, -1, -1, 9]]))
    ring = np.ones((5, 5), np.uint8)
    ring[2, 2] = 0
    assert R.fill_holes(ring).all() and not R.keep(ring, 1, border_free=True).any()
    ring[0, 0] = 0
    assert not R.fill_holes(ring)[0, 0] and R.fill_holes(ring)[2, 2]
    # a diagonal gap leaks at connectivity 2 but not at 1
    leak = np.ones((5, 5), np.uint8)
    leak[2, 2] = leak[1, 1] = leak[0, 0] = 0
    assert R.fill_holes(leak, 1)[2, 2] and not R.fill_holes(leak, 2)[2, 2]
    # an extent of one: every voxel lies on the border
    assert not R.keep(np.ones((1, 7, 1), np.uint8), 1, border_free=True).any()
    assert R.pattern('corners', (5, 6, 7)).sum() == 8 and R.pattern('corners', (1, 7, 1)).sum() == 2
    for shape in R.SHAPES + R.CHUNK_SHAPES:
        assert R.label(R.pattern('comb', shape), 1)[1] == 1, shape
        two = R.two_combs(shape)
        assert set(np.unique(two)) <= {0, 3, 7} and R.label(two, len(shape), [3])[1] == 1
    assert int(np.prod(R.SCAN_SHAPE)) > 256 * R.CHUNK
    # ties go to the lowest number
    tie = np.array([[1, 1, 0, 1, 1]], np.uint8)
    assert np.array_equal(R.keep(tie, 1, largest=True), np.array([[1, 1, 0, 0, 0]], bool))
