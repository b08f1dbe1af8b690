"""
utils.binary_erosion / binary_dilation / binary_opening / binary_closing, minimum_filter / maximum_filter / grey_* and median_filter /
rank_filter / percentile_filter (csrc/morph.hip) on the GPU against the definition of tests/morphology_restatement.py.  Every
comparison is an equality: the results are exact integers and order statistics.

Binary shapes, the smallest at which each mechanism can go wrong: last-axis extents 1, 63 / 64 / 65 (a word and its edges), 128, 130
(three words, a tail of two bits) and 1024 (sixteen words: the whole LDS budget); 7 x 9 x 67 and 5 x 66 x 70 (no multiple of the
8 x 8 tile of a 4-step launch, nor of the 14 x 14 one of a single step; 66 rows take several blocks), 1 x 2 x 65 (fewer rows than one
halo), 12 x 13 x 70 (thick enough for 3 .. 9 iterations), 2-D 3 x 130, 33 x 65, 40 x 70 and 260 x 5 (the 2-D footprint is 32 rows: two to eleven tiles), a
batch of 3 (a halo must not read the next entry).  Iterations 1, 2, 3, 4, 5 and 9: 5 and 9 take two and three launches.  No expected
output is constant (asserted where the cases are built).
Filter shapes: 5 x 9 x 67, 1 x 2 x 5 (windows wider than two of the axes, up to 31 over an extent of 1), 33 x 65 and a batch of 3.
"""

import numpy as np
import pytest
import torch

import morphology_restatement as R

pytestmark = pytest.mark.gpu


def _ne():
    import neurite_amd as ne
    return ne


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                  # (a copy: the shared cases are read-only)


BINARY = {'erosion': 'binary_erosion', 'dilation': 'binary_dilation', 'opening': 'binary_opening', 'closing': 'binary_closing'}


def _typed(m, dtype):
    """the mask as a tensor of `dtype` whose != 0 is the mask: several nonzero values, and -0.0 as an unset float"""
    rng = np.random.default_rng(5)
    if dtype == 'bool':
        return m.copy()
    if dtype == 'uint8':
        return np.where(m, rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=m.shape), np.uint8(0))
    if dtype == 'int32':
        return np.where(m, rng.choice(np.array([1, -1, 256, -2 ** 31, 65536], dtype=np.int32), size=m.shape), np.int32(0))
    unset = rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=m.shape)
    return np.where(m, rng.choice(np.array([1.0, -2.5, 1e-40, np.inf], dtype=np.float32), size=m.shape), unset)


@pytest.mark.parametrize('op', sorted(BINARY))
def test_binary_cases_equal_the_restatement(dev, op):
    ne = _ne()
    seen = 0
    for key, m, want in R.binary_cases():
        shape, kind, structure, iterations, border, case_op = key
        if case_op != op:
            continue
        fn = getattr(ne.utils, BINARY[op])
        got = fn(_t(m, dev), structure=R.structure_arg(structure, len(shape) - 1), iterations=iterations, border_value=border,
                 batched=True)
        assert got.dtype == torch.bool and got.shape == m.shape and got.device == dev, key
        assert np.array_equal(got.cpu().numpy(), want), key
        if shape[0] == 1:                                        # without a batch axis
            single = fn(_t(m[0], dev), R.structure_arg(structure, len(shape) - 1), iterations, border)
            assert np.array_equal(single.cpu().numpy(), want[0]), key
        seen += 1
    assert seen >= 7


@pytest.mark.parametrize('dtype', ['bool', 'uint8', 'int32', 'float32'])
def test_binary_input_dtypes(dev, dtype):
    ne = _ne()
    for key, m, want in R.binary_cases()[:2] + R.binary_cases()[-2:]:
        shape, kind, structure, iterations, border, op = key
        x = _t(_typed(m, dtype), dev)
        assert str(x.dtype) == 'torch.' + dtype and np.array_equal((x != 0).cpu().numpy(), m)
        got = getattr(ne.utils, BINARY[op])(x, R.structure_arg(structure, len(shape) - 1), iterations, border, batched=True)
        assert np.array_equal(got.cpu().numpy(), want), (dtype, key)


def test_structure_none_is_connectivity_one_and_an_empty_structure_is_neutral(dev):
    ne = _ne()
    m = R.mask('blobs', (1, 7, 9, 67))
    x = _t(m, dev)
    assert np.array_equal(ne.utils.binary_erosion(x, batched=True).cpu().numpy(), R.binary(m, 1, 1, 0, (0,)))
    assert np.array_equal(ne.utils.binary_dilation(x, batched=True).cpu().numpy(), R.binary(m, 1, 1, 0, (1,)))
    empty = np.zeros((3, 3, 3), dtype=bool)
    assert bool(ne.utils.binary_erosion(x, empty, batched=True).all()) and not bool(ne.utils.binary_dilation(x, empty, batched=True).any())


def test_the_ball_goes_through_the_distance_transform(dev):
    ne = _ne()
    for shape in ((7, 9, 67), (33, 65)):
        m = R.mask('blobs', (1,) + shape)[0]
        x = _t(m, dev)
        for radius in (1, 1.5, 2.3):
            grow = ne.utils.binary_dilation(x, 'ball', radius=radius)
            shrink = ne.utils.binary_erosion(x, 'ball', radius=radius)
            assert grow.dtype == torch.bool and shrink.dtype == torch.bool
            assert torch.equal(grow, ne.utils.dist_trf(x, squared=True) <= radius * radius), (shape, radius)
            assert torch.equal(shrink, ne.utils.dist_trf(~x, squared=True) > radius * radius), (shape, radius)
            assert torch.equal(ne.utils.binary_opening(x, 'ball', radius=radius),
                               ne.utils.binary_dilation(shrink, 'ball', radius=radius))
        # radius 1 is connectivity 1 wherever the outside does not matter: a dilation with border 0, an erosion with border 1
        assert np.array_equal(ne.utils.binary_dilation(x, 'ball', radius=1).cpu().numpy(), R.binary(m[None], 1, 1, 0, (1,))[0])
        assert np.array_equal(ne.utils.binary_erosion(x, 'ball', radius=1).cpu().numpy(), R.binary(m[None], 1, 1, 1, (0,))[0])


MINMAX = (('minimum_filter', (0,)), ('maximum_filter', (1,)))


@pytest.mark.parametrize('mode', R.MODES)
def test_minmax_filters_equal_the_restatement(dev, mode):
    ne = _ne()
    for shape in R.FILTER_SHAPES:
        nd = len(shape) - 1
        x = R.image('float', shape)
        xt = _t(x, dev)
        for size in R.MINMAX_SIZES[nd]:
            for name, stages in MINMAX:
                got = getattr(ne.utils, name)(xt, size=size, mode=mode, cval=R.CVAL, batched=True)
                want = R.minmax_filter(x, R.box(size, nd), mode, R.CVAL, stages)
                assert got.dtype == torch.float32 and got.shape == x.shape, (shape, size, name)
                assert np.array_equal(got.cpu().numpy(), want), (shape, size, name)
    # without a batch axis, and the grey names
    x = R.image('float', R.FILTER_SHAPES[0])
    for name, stages in (('grey_erosion', (0,)), ('grey_dilation', (1,)), ('grey_opening', (0, 1)), ('grey_closing', (1, 0))):
        got = getattr(ne.utils, name)(_t(x[0], dev), (3, 1, 5), mode, R.CVAL)
        assert np.array_equal(got.cpu().numpy(), R.minmax_filter(x, (3, 1, 5), mode, R.CVAL, stages)[0]), name


def test_minmax_filters_on_int32_and_the_default_arguments(dev):
    ne = _ne()
    for shape in (R.FILTER_SHAPES[0], R.FILTER_SHAPES[2]):
        nd = len(shape) - 1
        x = R.image('int', shape)
        assert x.min() < 0
        for mode in R.MODES:
            for name, stages in MINMAX + (('grey_opening', (0, 1)), ('grey_closing', (1, 0))):
                got = getattr(ne.utils, name)(_t(x, dev), 5, mode, R.CVAL, batched=True)
                assert got.dtype == torch.int32, name
                assert np.array_equal(got.cpu().numpy(), R.minmax_filter(x, (5,) * nd, mode, R.CVAL, stages)), (shape, mode, name)
        got = ne.utils.maximum_filter(_t(x, dev), batched=True)                   # size 3, reflect
        assert np.array_equal(got.cpu().numpy(), R.minmax_filter(x, (3,) * nd, 'reflect', 0.0, (1,)))
    x = R.image('float', R.FILTER_SHAPES[0])
    got = ne.utils.minimum_filter(_t(x, dev), 1, batched=True)                    # every size 1: the identity
    assert np.array_equal(got.cpu().numpy(), x)


def _rank_call(ne, rule, arg, xt, size, mode):
    if rule == 'median':
        return ne.utils.median_filter(xt, size=size, mode=mode, cval=R.CVAL, batched=True)
    if rule == 'rank':
        return ne.utils.rank_filter(xt, arg, size=size, mode=mode, cval=R.CVAL, batched=True)
    return ne.utils.percentile_filter(xt, arg, size=size, mode=mode, cval=R.CVAL, batched=True)


@pytest.mark.parametrize('mode', R.MODES)
def test_rank_filters_equal_the_restatement(dev, mode):
    ne = _ne()
    for shape in R.FILTER_SHAPES:
        nd = len(shape) - 1
        for kind in ('float', 'ties', 'int'):
            x = R.image(kind, shape)
            xt = _t(x, dev)
            for size in R.RANK_SIZES[nd]:
                sizes = R.box(size, nd)
                n = int(np.prod(sizes))
                windows = np.sort(R.windows(x, sizes, mode, R.CVAL), axis=-1)
                for rule, arg in R.RANK_RULES:
                    got = _rank_call(ne, rule, arg, xt, size, mode)
                    assert got.dtype == xt.dtype and got.shape == x.shape
                    assert np.array_equal(got.cpu().numpy(), windows[..., R.rank_of(rule, n, arg)]), (shape, kind, size, rule, arg)


def test_two_runs_are_bit_identical(dev):
    ne = _ne()
    m = _t(R.mask('blobs', (3, 7, 9, 67)), dev)
    x = _t(R.image('float', (3, 5, 9, 67)), dev)
    runs = (lambda: ne.utils.binary_closing(m, 2, 5, batched=True),
            lambda: ne.utils.grey_opening(x, (3, 5, 7), 'mirror', batched=True),
            lambda: ne.utils.median_filter(x, 3, 'nearest', batched=True))
    for run in runs:
        a, b = run(), run()
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))


def test_graph_capture(dev):
    ne = _ne()
    shape = (3, 7, 9, 67)
    masks = [R.mask('blobs', shape, seed=s) for s in (0, 1)]
    images = [R.image('float', shape, seed=s) for s in (0, 1)]

    def run(m, x):
        return (ne.utils.binary_opening(m, 2, R.STEPS_PER_LAUNCH + 1, 1, batched=True),
                ne.utils.grey_closing(x, (3, 5, 3), 'reflect', batched=True),
                ne.utils.percentile_filter(x, 75, 3, 'mirror', batched=True))

    def want(k):
        return (R.binary(masks[k], 2, R.STEPS_PER_LAUNCH + 1, 1, (0, 1)), R.minmax_filter(images[k], (3, 5, 3), 'reflect', 0.0, (1, 0)),
                R.rank_filter(images[k], R.rank_of('percentile', 27, 75), (3, 3, 3), 'mirror'))

    m, x = _t(masks[0], dev), _t(images[0], dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(m, x)                                                                 # (warm-up: workspaces and the device are set up)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(m, x)
    for k in (1, 0):
        m.copy_(_t(masks[k], dev))
        x.copy_(_t(images[k], dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, ref in zip(out, want(k)):
            assert np.array_equal(got.cpu().numpy(), ref), k


def test_results_carry_no_grad(dev):
    ne = _ne()
    x = _t(R.image('float', (1, 5, 9, 67)), dev).requires_grad_(True)
    for out in (ne.utils.binary_dilation(x, batched=True), ne.utils.maximum_filter(x, batched=True),
                ne.utils.median_filter(x, (1, 3, 3), batched=True)):
        assert not out.requires_grad
