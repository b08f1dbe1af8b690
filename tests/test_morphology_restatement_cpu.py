"""
CPU test that pins the semantics: the NumPy definition of tests/morphology_restatement.py (what the GPU tests and the word-core test
compare against) equals scipy.ndimage for every function, boundary mode, connectivity and border value, the asymmetric structure
without its centre, the rank rules of median_filter / rank_filter / percentile_filter, and windows wider than the axis (extent 2
under a window of 5, extents 1 and 2 under 31).  It passes without the feature: it tests the definition, not the kernels.
"""

import numpy as np
import pytest

import morphology_restatement as R

ndi = pytest.importorskip('scipy.ndimage')


def _each(x):
    return [x[e] for e in range(x.shape[0])]


def test_binary_cases_equal_scipy():
    fns = {'erosion': ndi.binary_erosion, 'dilation': ndi.binary_dilation, 'opening': ndi.binary_opening, 'closing': ndi.binary_closing}
    seen = set()
    for key, m, want in R.binary_cases():
        shape, kind, structure, iterations, border, op = key
        nd = len(shape) - 1
        st = R.structure_of(R.structure_arg(structure, nd), nd)
        if isinstance(structure, int):
            assert np.array_equal(st, ndi.generate_binary_structure(nd, structure))
        got = np.stack([fns[op](v, structure=st, iterations=iterations, border_value=border) for v in _each(m)])
        assert np.array_equal(got, want), key
        seen.add((op, border, structure if isinstance(structure, str) else 'conn%d' % structure))
    for op in ('erosion', 'dilation'):
        for border in (0, 1):
            assert {(op, border, s) for s in ('conn1', 'conn2', 'conn3', 'asym')} <= seen
    assert {k[0][5] for k in R.binary_cases()} == set(fns)
    assert any(k[0][3] == R.STEPS_PER_LAUNCH + 1 for k in R.binary_cases())


def test_the_structure_bits_follow_the_offsets():
    assert R.structure_bits(1, 3) == sum(1 << i for i in (4, 10, 12, 13, 14, 16, 22))
    assert R.structure_bits(3, 3) == (1 << 27) - 1 and R.structure_bits(2, 2) == 0x1FF << 9
    one = np.zeros((3, 3, 3), dtype=bool)
    one[2, 0, 1] = True                                        # dz = +1, dy = -1, dx = 0
    assert R.structure_bits(one, 3) == 1 << (2 * 9 + 0 * 3 + 1)


@pytest.mark.parametrize('mode', R.MODES)
def test_minmax_equals_scipy(mode):
    for shape in R.FILTER_SHAPES:
        nd = len(shape) - 1
        for kind in ('float', 'int'):
            x = R.image(kind, shape)
            for size in R.MINMAX_SIZES[nd]:
                sizes = R.box(size, nd)
                for name, stages, fns in (('min', (0,), (ndi.minimum_filter, ndi.grey_erosion)),
                                          ('max', (1,), (ndi.maximum_filter, ndi.grey_dilation)),
                                          ('open', (0, 1), (ndi.grey_opening,)), ('close', (1, 0), (ndi.grey_closing,))):
                    want = R.minmax_filter(x, sizes, mode, R.CVAL, stages)
                    for fn in fns:
                        got = np.stack([fn(v, size=sizes, mode=mode, cval=R.CVAL) for v in _each(x)])
                        assert got.dtype == want.dtype and np.array_equal(got, want), (shape, kind, size, name, fn.__name__)


def test_the_fold_of_a_window_wider_than_the_axis():
    x = np.arange(1, 3, dtype=np.float32).reshape(1, 1, 2)                       # extent 2 under a window of 5
    assert R.padded(x, (1, 5), 'reflect')[0, 0].tolist() == [2, 1, 1, 2, 2, 1]
    assert R.padded(x, (1, 5), 'mirror')[0, 0].tolist() == [1, 2, 1, 2, 1, 2]
    assert R.padded(x, (1, 5), 'nearest')[0, 0].tolist() == [1, 1, 1, 2, 2, 2]
    assert R.padded(x, (1, 5), 'constant', 0.25)[0, 0].tolist() == [0.25, 0.25, 1, 2, 0.25, 0.25]
    for mode in R.MODES:
        got = ndi.maximum_filter(x[0], size=(1, 5), mode=mode, cval=R.CVAL)
        assert np.array_equal(got, R.minmax_filter(x, (1, 5), mode, R.CVAL, (1,))[0]), mode


@pytest.mark.parametrize('mode', R.MODES)
def test_rank_filters_equal_scipy(mode):
    for shape in R.FILTER_SHAPES:
        nd = len(shape) - 1
        for kind in ('float', 'ties', 'int'):
            x = R.image(kind, shape)
            for size in R.RANK_SIZES[nd]:
                sizes = R.box(size, nd)
                n = int(np.prod(sizes))
                for rule, arg in R.RANK_RULES:
                    want = R.rank_filter(x, R.rank_of(rule, n, arg), sizes, mode, R.CVAL)
                    if rule == 'median':
                        got = [ndi.median_filter(v, size=sizes, mode=mode, cval=R.CVAL) for v in _each(x)]
                    elif rule == 'rank':
                        got = [ndi.rank_filter(v, arg, size=sizes, mode=mode, cval=R.CVAL) for v in _each(x)]
                    else:
                        got = [ndi.percentile_filter(v, arg, size=sizes, mode=mode, cval=R.CVAL) for v in _each(x)]
                    got = np.stack(got)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (shape, kind, size, rule, arg)


def test_the_rank_rules():
    assert [R.rank_of('median', n) for n in (9, 25, 27)] == [4, 12, 13]
    assert R.rank_of('rank', 27, -1) == 26 and R.rank_of('rank', 27, 5) == 5
    assert [R.rank_of('percentile', 27, p) for p in (0, 10, 75, 100, -25)] == [0, 2, 20, 26, 20]
