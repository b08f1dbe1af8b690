"""
CPU tests of neurite_amd.seg (no kernel is launched): the four entry points of csrc/seg.hip are declared, typed and exported and refuse
bad arguments before any launch; the functions have the reference's signatures (by AST; the reference's side is recorded in
tests/golden/seg_small.npz by tests/golden/make_seg_golden.py); CPU tensors are refused; the NumPy quilt restatement
(tests/seg_restatement.py) inverts a NumPy patch extraction; the reference's own recorded prob_of_label outputs meet the bound the GPU
test holds the kernel to.
"""

import json
import os
import sys

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ast_signatures as sigs          # noqa: E402
import seg_restatement as rs           # noqa: E402
from conftest import golden_cases, load_golden          # noqa: E402

ENTRY_POINTS = ['nrt_seg_argmax', 'nrt_seg_recode', 'nrt_patch_extract', 'nrt_patch_quilt']
F32, BF16, F16, F64, I32 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16, _lib.DT_F64, _lib.DT_I32
INV, UNSUP = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_UNSUPPORTED
D = 16                                             # a non-NULL "pointer"; nothing is launched on a refused call


def _argmax(pred=D, dtype=F32, n=10, C=4, labels=D, l64=0, of=None, of64=0, prob=None):
    return _lib.lib().nrt_seg_argmax(pred, dtype, n, C, labels, l64, of, of64, prob, None)


def _recode(seg=D, s64=0, n=10, lookup=D, nl=5, out=D):
    return _lib.lib().nrt_seg_recode(seg, s64, n, lookup, nl, out, None)


def _arr(v):
    return None if v is None else _lib.ints(v)


def _extract(vol=D, dtype=F32, nd=None, shape=(12, 12, 12), C=1, patch=(8, 8, 8), stride=(4, 4, 4), grid=(2, 2, 2), n0=0, count=8, out=D):
    nd = nd if nd is not None else 3 if patch is None else len(patch)
    return _lib.lib().nrt_patch_extract(vol, dtype, nd, _arr(shape), C, _arr(patch), _arr(stride), _arr(grid), n0, count, out, None)


def _quilt(p=D, dtype=F32, nd=None, patch=(8, 8, 8), stride=(4, 4, 4), grid=(2, 2, 2), C=1, reduce=0, vol=D):
    nd = nd if nd is not None else 3 if patch is None else len(patch)
    return _lib.lib().nrt_patch_quilt(p, dtype, nd, _arr(patch), _arr(stride), _arr(grid), C, reduce, vol, None)


def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_null_pointers_and_non_positive_sizes_are_invalid_arguments():
    for kw in ({'pred': None}, {'labels': None}, {'labels': None, 'of': D}, {'of': D}, {'n': 0}, {'n': -3}, {'C': 0}, {'C': -1}):
        assert _argmax(**kw) == INV, kw
    for kw in ({'seg': None}, {'lookup': None}, {'out': None}, {'n': 0}, {'n': -1}, {'nl': 0}, {'nl': -2}):
        assert _recode(**kw) == INV, kw
    for kw in ({'vol': None}, {'out': None}, {'shape': None}, {'patch': None}, {'stride': None}, {'grid': None}, {'C': 0}, {'count': 0},
               {'count': -1}, {'n0': -1}, {'nd': 0}, {'nd': 4}, {'patch': (8, 0, 8)}, {'stride': (4, 4, 0)}, {'grid': (2, -2, 2)},
               {'shape': (12, 0, 12)}, {'n0': 1, 'count': 8}, {'n0': 8, 'count': 1}):
        assert _extract(**kw) == INV, kw
    for kw in ({'p': None}, {'vol': None}, {'patch': None}, {'stride': None}, {'grid': None}, {'C': 0}, {'nd': 0}, {'nd': 4},
               {'patch': (8, 8, -8)}, {'stride': (0, 4, 4)}, {'grid': (2, 2, 0)}, {'reduce': 2}, {'reduce': -1}):
        assert _quilt(**kw) == INV, kw


def test_a_grid_that_does_not_fit_is_an_invalid_argument():
    assert _extract(shape=(12, 12, 11)) == INV                              # (2 - 1) * 4 + 8 = 12 > 11
    assert _extract(grid=(2, 3, 2), count=12) == INV
    assert _extract(stride=(4, 5, 4)) == INV
    assert _extract(nd=1, shape=(9,), patch=(5,), stride=(2,), grid=(4,), count=4) == INV       # needs 11
    assert _extract(nd=2, shape=(9, 8), patch=(5, 5), stride=(2, 2), grid=(3, 3), count=9) == INV


def test_other_dtypes_are_unsupported():
    for dtype in (F16, F64, I32, 7, -1):
        assert _argmax(dtype=dtype) == UNSUP, dtype
        assert _extract(dtype=dtype) == UNSUP, dtype
    for dtype in (BF16, F16, F64, 7, -1):
        assert _quilt(dtype=dtype) == UNSUP, dtype
        assert _quilt(dtype=dtype, reduce=1) == UNSUP, dtype


def test_size_limits_are_unsupported():
    assert _argmax(C=257) == UNSUP
    assert _argmax(n=1 << 31, C=1) == UNSUP
    assert _argmax(n=1 << 29, C=4) == UNSUP                                 # n * C = 2^31
    assert _argmax(n=1 << 29, C=4, dtype=BF16) == UNSUP
    assert _recode(n=1 << 31) == UNSUP
    assert _recode(nl=1 << 31) == UNSUP
    big = dict(nd=3, patch=(1 << 10, 1 << 10, 1 << 9), stride=(1, 1, 1), grid=(1, 1, 1))            # one patch of 2^29 voxels
    assert _extract(shape=(1 << 10, 1 << 10, 1 << 9), C=4, count=1, **big) == UNSUP
    assert _extract(shape=(1 << 11, 1 << 10, 1 << 10), C=1, count=1, **big) == UNSUP                # the volume itself has 2^31
    assert _quilt(C=4, **big) == UNSUP
    assert _quilt(C=4, reduce=1, **big) == UNSUP
    assert _quilt(nd=1, patch=(4,), stride=(4,), grid=(1 << 29,)) == UNSUP                          # 2^31 patch elements


def test_median_takes_64_covers_and_refuses_65():
    assert _quilt(nd=1, patch=(65,), stride=(1,), grid=(2,), reduce=1) == UNSUP
    assert _quilt(nd=3, patch=(5, 4, 4), stride=(1, 1, 1), grid=(2, 2, 2), reduce=1) == UNSUP       # 80
    assert _quilt(nd=2, patch=(9, 9), stride=(1, 1), grid=(2, 2), reduce=1) == UNSUP                # 81
    assert _quilt(nd=3, patch=(9, 9, 9), stride=(2, 2, 2), grid=(2, 2, 2), reduce=1) == UNSUP       # ceil(9 / 2)^3 = 125


def test_signatures_equal_the_reference():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'seg_small.npz'), allow_pickle=False) as z:
        want = json.loads(str(z['__signatures__']))
    path = os.path.join(ROOT, 'neurite_amd', 'seg.py')
    for name in ('pred_to_label', 'prob_of_label', 'recode', 'predict_volumes', 'predict_volume_stack', '_quilt'):
        assert sigs.signature(path, name) == want[name], name
    assert want['predict_volumes']['defaults'][0] == 'np.nanmedian'
    for name in ('predict_volumes', 'predict_volume_stack', 'predict_volume', 'prob_of_label', 'pred_to_label', 'recode',
                 'extract_patches', 'quilt'):
        assert name in ne.seg.__all__ and callable(getattr(ne.seg, name))
    assert ne.utils.seg is ne.seg


def test_cpu_tensors_are_refused():
    x, lab = torch.rand(3, 4, 5), torch.zeros(3, 4, dtype=torch.int64)
    calls = [lambda: ne.seg.pred_to_label(x), lambda: ne.seg.prob_of_label(x, lab), lambda: ne.seg.recode(lab, [0, 1]),
             lambda: ne.seg.extract_patches(torch.rand(6, 6, 1), (4, 4), (2, 2)),
             lambda: ne.seg.quilt(torch.rand(4, 4, 4, 1), (4, 4), (2, 2), (2, 2)),
             lambda: ne.seg._quilt(torch.rand(4, 16), (4, 4), (2, 2), (2, 2), nan_func_layers=np.nanmedian, nan_func_K=np.nanmedian),
             lambda: ne.seg.predict_volume(lambda p: p, torch.rand(6, 6, 1), (4, 4), (2, 2)),
             lambda: ne.seg.predict_volumes(lambda p: p, iter([(x[None], x[None])]), 1, (3, 4), (3, 4), (1, 1)),
             lambda: ne.seg.predict_volume_stack(lambda p: p, iter([(x[None], x[None])]), 1, (1, 1))]
    for call in calls:
        with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
            call()


def test_host_side_argument_checks():
    with pytest.raises(ValueError, match='nan_func'):
        ne.seg.quilt(torch.zeros(1, 4), (4,), (1,), (1,), nan_func=np.mean)
    with pytest.raises(ValueError, match='mapping must be'):
        ne.seg.recode(torch.zeros(3, dtype=torch.int32), 5)


def test_restated_quilt_inverts_a_numpy_extraction():
    rng = np.random.default_rng(363)
    for shape, patch, stride, C in (((11,), (5,), (2,), 3), ((12, 9), (4, 5), (4, 2), 1), ((12, 12, 12), (8, 8, 8), (4, 4, 4), 1),
                                    ((6, 7, 5), (4, 4, 4), (1, 1, 1), 2)):
        vol = rng.integers(0, 50, size=shape + (C,)).astype(np.float32)
        grid = rs.grid_of(shape, patch, stride)
        assert rs.quilt_shape(patch, grid, stride) == shape
        patches = rs.extract(vol, patch, stride)
        assert patches.shape == (int(np.prod(grid)),) + patch + (C,)
        # patch n is the window at unravel_index(n) * stride
        n = patches.shape[0] - 1
        idx = np.unravel_index(n, grid)
        assert np.array_equal(patches[n], vol[tuple(slice(i * s, i * s + p) for i, s, p in zip(idx, stride, patch))])
        for f in (np.nanmean, np.nanmedian):
            assert np.array_equal(rs.quilt(patches, patch, grid, stride, f), vol), (shape, f.__name__)
    # a stride larger than the patch leaves NaN gaps, and NaN values are skipped
    patches = np.ones((3, 2, 1), np.float32)
    patches[1, 0, 0] = np.nan
    got = rs.quilt(patches, (2,), (3,), (3,))[:, 0]
    assert np.array_equal(np.isnan(got), [False, False, True, True, False, True, False, False])


def test_recorded_prob_of_label_meets_the_bound_of_the_gpu_test():
    cases = {k: v for k, v in golden_cases(load_golden('seg_small')).items() if k.startswith('pl_')}
    assert len(cases) >= 10
    for tag, c in cases.items():
        x, lab, got = c['x'].astype(np.float64), c['label'], c['prob'].astype(np.float64)
        C = x.shape[-1]
        want = np.take_along_axis(x, lab[..., None].astype(np.int64), -1)[..., 0] / x.sum(-1)
        assert np.all(np.abs(got - want) <= (C + 2) * 2.0 ** -24 * np.abs(want)), tag
