"""
utils.connected_components / largest_component / keep_largest_components / remove_small_components / fill_holes,
metrics.ComponentCount and SynthStrip.brain_mask (csrc/ccl.hip) on the GPU against the flood fill of tests/ccl_restatement.py.  Every
comparison is exact (torch.equal): there is no tolerance in this feature.

The kernels have no spatial tile.  A block takes 1024 consecutive voxels of an entry's raster (256 threads, four rounds), so the seams
a union, a representative count or a number can go wrong at lie in the linear index: R.CHUNK_SHAPES holds 1023, 1024, 1025 and 2049
voxels as one row, as one column and as rows that straddle the seam, in 2-D and 3-D.  The scan of the chunk counts is one block per entry
that loops with a carry; R.SCAN_SHAPE (257 x 1021 = 262397 voxels, 257 chunks) reaches its second round.  There is no multi-level arm.
The size pass gives a block eight chunks (8192 voxels): 3x65x66 (12870 voxels) and R.SCAN_SHAPE have more than one such block per entry.
Patterns: empty, full, one voxel in each corner, a checkerboard (V / 2 components at connectivity 1, one at full connectivity), random
masks near the percolation thresholds (0.3, 0.5, 0.7 in 3-D, 0.6 in 2-D), a serpentine (one component, the longest parent chains), two
interleaved id patterns, random id maps, and blob id maps with 1, 5 and 33 listed labels and unlisted ids.  Batch 1, and batch 3 with
distinct entries, one of them empty, so that the numbering restarts per entry.
"""

import contextlib
import io

import numpy as np
import pytest
import torch

import ccl_restatement as R

pytestmark = pytest.mark.gpu

ids_of = lambda s: 'x'.join(map(str, s))            # noqa: E731


def _ne():
    import neurite_amd as ne
    return ne


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mask_patterns(shape):
    names = ['empty', 'full', 'corners', 'checker', 'comb'] + (['random0.3', 'random0.5', 'random0.7'] if len(shape) == 3 else ['random0.6'])
    return [(name, R.pattern(name, shape, seed=11)) for name in names]


def _check_mask(ne, m, connectivity, dev, what):
    """every mask entry point on m [B, *S] uint8 (NumPy) against the restatement, entry by entry"""
    x = _t(m, dev)
    comp, count = ne.utils.connected_components(x, connectivity, batched=True)
    largest = ne.utils.largest_component(x, connectivity, batched=True)
    small = ne.utils.remove_small_components(x, 3, connectivity, batched=True)
    filled = ne.utils.fill_holes(x, connectivity, batched=True)
    _, inner = ne.utils._ccl_select(x, None, connectivity, True, 'test', want_table=True, want_out=False)
    free, table = ne.utils._ccl_select(x, None, connectivity, True, 'test', mode=ne._lib.CCL_BORDER_FREE, want_table=True)
    cc = ne.metrics.ComponentCount([1], connectivity)
    xi = x.to(torch.int32)
    counts, big, extra = cc.counts(xi), cc.largest(xi), cc.extra(xi)
    assert comp.dtype == torch.int32 and count.dtype == torch.int32 and largest.dtype == torch.uint8 and table.dtype == torch.int32
    for b in range(m.shape[0]):
        want, n = R.label(m[b], connectivity)
        tag = (what, b, connectivity)
        assert torch.equal(comp[b].cpu(), torch.from_numpy(want)), tag
        assert int(count[b]) == n, tag
        tab = R.table(m[b], connectivity)
        assert torch.equal(table[b].cpu(), torch.from_numpy(tab)), tag
        assert torch.equal(inner[b].cpu(), torch.from_numpy(tab)), tag
        assert torch.equal(largest[b].cpu(), _t(R.keep(m[b], connectivity, largest=True).astype(np.uint8), 'cpu')), tag
        assert torch.equal(small[b].cpu(), _t(R.keep(m[b], connectivity, min_size=3).astype(np.uint8), 'cpu')), tag
        assert torch.equal(free[b].cpu(), _t(R.keep(m[b], connectivity, border_free=True).astype(np.uint8), 'cpu')), tag
        assert torch.equal(filled[b].cpu(), _t(R.fill_holes(m[b], connectivity).astype(np.uint8), 'cpu')), tag
        assert counts[b].tolist() == [tab[0, 0]] and big[b].tolist() == [tab[0, 1]] and extra[b].tolist() == [max(tab[0, 0] - 1, 0)], tag


def _check_ids(ne, ids, labels, connectivity, dev, what, fill=-5):
    """every id-map entry point on ids [B, *S] int32 (NumPy)"""
    x = _t(ids, dev)
    comp, count = ne.utils.connected_components(x, connectivity, labels=labels, batched=True)
    largest = ne.utils.keep_largest_components(x, labels, connectivity, fill=fill, batched=True)
    small = ne.utils.remove_small_components(x, 4, connectivity, labels=labels, fill=fill, batched=True)
    free, _ = ne.utils._ccl_select(x, labels, connectivity, True, 'test', mode=ne._lib.CCL_BORDER_FREE, fill=fill)
    cc = ne.metrics.ComponentCount(labels, connectivity)
    table = cc.table(x.to(torch.int64))
    for b in range(ids.shape[0]):
        want, n = R.label(ids[b], connectivity, labels)
        tag = (what, b, connectivity, len(labels))
        assert torch.equal(comp[b].cpu(), torch.from_numpy(want)), tag
        assert int(count[b]) == n, tag
        tab = R.table(ids[b], connectivity, labels)
        assert torch.equal(table[b].cpu(), torch.from_numpy(tab)), tag
        assert torch.equal(largest[b].cpu(), torch.from_numpy(R.select_ids(ids[b], labels, connectivity, fill, largest=True))), tag
        assert torch.equal(small[b].cpu(), torch.from_numpy(R.select_ids(ids[b], labels, connectivity, fill, min_size=4))), tag
        assert torch.equal(free[b].cpu(), torch.from_numpy(R.select_ids(ids[b], labels, connectivity, fill, border_free=True))), tag
    assert torch.equal(cc.extra(x), (table[..., 0] - 1).clamp(min=0)) and torch.equal(cc.largest(x), table[..., 1])


@pytest.mark.parametrize('shape', R.SHAPES + R.CHUNK_SHAPES, ids=ids_of)
def test_masks_equal_the_flood_fill(dev, shape):
    ne = _ne()
    patterns = _mask_patterns(shape)
    dense = 'random0.5' if len(shape) == 3 else 'random0.6'
    by_name = dict(patterns)
    batch3 = np.stack([by_name[dense], by_name['empty'], by_name['comb']])
    for connectivity in range(1, len(shape) + 1):
        for name, m in patterns:
            _check_mask(ne, m[None], connectivity, dev, name)
        _check_mask(ne, batch3, connectivity, dev, 'batch3')
    # the checkerboard: every voxel of it alone at connectivity 1, one component at full connectivity (where two axes have extent)
    n = int(np.prod(shape))
    assert R.label(by_name['checker'], 1)[1] == (n + 1) // 2
    assert R.label(by_name['checker'], len(shape))[1] == (1 if sum(v > 1 for v in shape) >= 2 else (n + 1) // 2)
    assert R.label(by_name['comb'], 1)[1] == 1


@pytest.mark.parametrize('shape', R.SHAPES + R.CHUNK_SHAPES[:7], ids=ids_of)
def test_id_maps_equal_the_flood_fill(dev, shape):
    ne = _ne()
    combs = R.two_combs(shape)
    rnd = R.random_ids(shape, 4, seed=7)
    batch3 = np.stack([rnd, np.zeros(shape, np.int32), combs])
    for connectivity in range(1, len(shape) + 1):
        _check_ids(ne, combs[None], [3, 7], connectivity, dev, 'combs')
        _check_ids(ne, combs[None], [7], connectivity, dev, 'combs7')
        _check_ids(ne, rnd[None], [2, 0, 3], connectivity, dev, 'random')          # (0 is an id like any other once it is listed)
        _check_ids(ne, batch3, [3, 1, 7], connectivity, dev, 'batch3')


@pytest.mark.parametrize('nlabels', [1, 5, 33])
def test_blob_label_maps(dev, nlabels):
    """blob maps from synth.blob_labels with 36 ids, of which 1, 5 and 33 are listed (in an order of their own); the others are background"""
    ne = _ne()
    from neurite_amd import synth
    vols = [synth.blob_labels(seed, size=20, nb_labels=36, coarse=5).numpy().astype(np.int32) for seed in (1, 2)]
    order = np.random.default_rng(3).permutation(36)
    labels = [int(v) for v in order[:nlabels]]
    shaped = [vols[0], vols[0][:5, :18, :19], vols[0][7]]
    for ids in shaped:
        for connectivity in range(1, ids.ndim + 1):
            _check_ids(ne, np.ascontiguousarray(ids)[None], labels, connectivity, dev, 'blob')
    _check_ids(ne, np.stack([vols[0], np.full_like(vols[0], labels[0]), vols[1]]), labels, 1, dev, 'blob batch')


def test_scan_second_round(dev):
    """257 chunks: the block that scans the chunk counts goes round its loop twice"""
    ne = _ne()
    assert -(-int(np.prod(R.SCAN_SHAPE)) // R.CHUNK) == 257
    m = R.pattern('random0.6', R.SCAN_SHAPE, seed=2)
    _check_mask(ne, m[None], 1, dev, 'scan')
    comp, count = ne.utils.connected_components(_t(R.pattern('checker', R.SCAN_SHAPE), dev))
    n = int(np.prod(R.SCAN_SHAPE))
    assert int(count) == (n + 1) // 2 and count.dim() == 0
    flat = comp.reshape(-1)
    assert torch.equal(flat[0::2], torch.arange(1, (n + 1) // 2 + 1, dtype=torch.int32, device=dev)) and not flat[1::2].any()


def test_largest_component_ties_and_dtypes(dev):
    ne = _ne()
    m = np.zeros((6, 9), np.uint8)
    m[4, 0:3] = 1                                                               # three components of three voxels: the first in raster
    m[1, 5:8] = 1                                                               # order is the one in row 1
    m[3:6, 8] = 1
    want = np.zeros_like(m)
    want[1, 5:8] = 1
    for connectivity in (1, 2):
        assert np.array_equal(R.keep(m, connectivity, largest=True), want.astype(bool))
        for dtype in (torch.uint8, torch.bool, torch.float32, torch.int64):
            got = ne.utils.largest_component(_t(m, dev).to(dtype), connectivity)
            assert got.dtype == dtype and got.shape == m.shape and torch.equal(got.cpu(), torch.from_numpy(want).to(dtype))
    ids = np.where(m, 4, 9).astype(np.int32)
    got = ne.utils.keep_largest_components(_t(ids, dev), [4], fill=1)
    assert torch.equal(got.cpu(), torch.from_numpy(np.where(m & ~want.astype(bool), 1, ids).astype(np.int32)))
    empty = torch.zeros((4, 5, 6), dtype=torch.bool, device=dev)
    assert not ne.utils.largest_component(empty).any() and not ne.utils.fill_holes(empty).any()
    hole = torch.ones((5, 5, 5), dtype=torch.float32, device=dev)
    hole[2, 2, 2] = 0
    filled = ne.utils.fill_holes(hole)
    assert filled.dtype == torch.float32 and bool(filled.all()) and bool(ne.utils.fill_holes(hole.bool()).all())
    comp, count = ne.utils.connected_components(hole)
    assert comp.shape == hole.shape and count.dim() == 0 and int(count) == 1


def test_two_runs_are_identical(dev):
    ne = _ne()
    x = _t(R.pattern('random0.5', (40, 41, 42), seed=9), dev)
    ids = _t(R.random_ids((40, 41, 42), 5, seed=9), dev)
    for connectivity in (1, 3):
        a, b = [ne.utils.connected_components(x, connectivity) for _ in range(2)]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a, b = [ne.utils.fill_holes(x, connectivity) for _ in range(2)]
        assert torch.equal(a, b)
        a, b = [ne.utils.keep_largest_components(ids, [1, 2, 3], connectivity) for _ in range(2)]
        assert torch.equal(a, b)
        a, b = [ne.metrics.ComponentCount([1, 2, 3], connectivity).table(ids[None]) for _ in range(2)]
        assert torch.equal(a, b)


def test_pipeline_captures_into_a_graph(dev):
    """connected_components -> largest_component -> fill_holes on one stream, captured once and replayed on a second input"""
    ne = _ne()
    shape = (24, 25, 26)
    inputs = [_t(R.pattern('random0.5', shape, seed=s), dev) for s in (1, 2)]

    def pipeline(x):
        comp, count = ne.utils.connected_components(x, 2)
        return comp, count, ne.utils.fill_holes(ne.utils.largest_component(x, 2), 2)

    eager = [pipeline(x) for x in inputs]
    static = inputs[0].clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pipeline(static)                                                        # (warm-up: workspaces and the device are set up)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipeline(static)
    for x, want in zip(inputs[::-1], eager[::-1]):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, w in zip(out, want):
            assert torch.equal(got, w)
    assert torch.equal(eager[0][2].cpu(), _t(R.fill_holes(R.keep(inputs[0].cpu().numpy(), 2, largest=True), 2).astype(np.uint8), 'cpu'))


def test_synthstrip_brain_mask(dev):
    ne = _ne()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ne.models.SynthStrip((16, 16, 16), [0, 1, 2, 3], {1: 1, 2: 1, 3: 1}, nb_unet_features=4, nb_unet_levels=2)
    model = model.to(dev)
    image = torch.rand((2, 16, 16, 16, 1), device=dev)
    with torch.no_grad():
        sdt = model.get_strip_model()(image)[..., 0]
    border = float(sdt.median())                                                # (an untrained net: a border that splits its output)
    for connectivity in (1, 3):
        got = model.brain_mask(image, border=border, connectivity=connectivity)
        assert got.dtype == torch.bool and got.shape == (2, 16, 16, 16)
        assert torch.equal(got, model.brain_mask(image[..., 0], border=border, connectivity=connectivity))
        for b in range(2):
            m = (sdt[b] < border).cpu().numpy()
            assert 0 < m.sum() < m.size
            want = R.fill_holes(R.keep(m, connectivity, largest=True), connectivity)
            assert torch.equal(got[b].cpu(), torch.from_numpy(want)), (b, connectivity)
