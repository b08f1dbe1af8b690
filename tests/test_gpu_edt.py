"""
utils.dist_trf / signed_dist_trf / vol_to_sdt / vol_to_sdt_batch / label_dist_trf, metrics.SurfaceDistance and losses.SignedDistanceMSE
(csrc/edt.hip) on the GPU against the brute-force restatement of tests/edt_restatement.py.  Every call is made twice and the two results
are compared bit for bit.  At unit spacing every squared distance is an integer below 2^24, so the squares are compared bit for bit and
the roots against np.sqrt of the float32 square.

The transform is one pass per axis over out viewed as [outer, n, inner] (inner holds the later axes and the label channels): the first
pass walks every line up and down (one thread per line), the others search outward from every element, four distances at a time, so
lines of 1 .. 5 voxels (no group, one partial group, one full group and one more) are in the list as well: 1x1x1, 1x7x1, 2x2x129,
3x65x66, 130x3x5, 5x6x7.  The boundaries the kernel has, and the shapes that sit on either side of them (besides the fixed list,
which covers axes of extent 1 and lines just under, at and just over one wave and over two waves at each axis position):
    n * inner <= 16384 floats: the contiguous arm, else the tiled arm       128x128 (16384) | 128x129 (16512: tiles of 64, 64, 1)
    tiled arm, tile width 64 for n <= 256, 32 for n <= 512, else 16          256x65 | 257x65 (32, 32, 1);  512x33 | 513x33 (16, 16, 1)
    the largest extent, 1024, on each axis position                         1024x17 (16, 1) | 3x1024 (contiguous, 4 lines per block)
    first pass, one thread of 1024 per line of the block                    3x1024 (1024 lines) | 2x1024 (2048 lines in a block of two entries);
                                                                             5x6x7 with 33 labels (1386 lines)
    contiguous arm, outer entries per block = max(1, 4096 / (n * inner))     23x89, 32x64 (2047, 2048: two entries per block, the batch of
                                                                             three leaves the last block one) | 3x683 (2049: one)
    tiled arm in 3-D, more than one outer entry per batch entry             2x130x130 (265 tiles, the last 4 wide; then 3 tiles of 64, 64, 2)
    label channels move the arms: 17x65 with 33 labels                      axis 0 tiled (inner 2145), axis 1 contiguous, one entry per block
    surface statistics: runs of at least 2048 voxels, at most 256 runs      23x89, 32x64, 3x683 (one run, one run, two);  725x725
                                                                             (525625 voxels: 256 runs of 2054)
Batch 1 and 3.  Feature sets: empty, full, one voxel at each corner, densities 0.5 and 0.02, a ball; they travel as the entries of a batch.
The brute force costs voxels x features, so the signed transform (whose complement is large whenever the set is small) is brute-forced
for every set up to 5000 voxels, for density 0.5, empty and full up to 13000, and for empty and full above, where the unsigned sets are
the sparse ones and the ball: the signed transform runs the same pass kernel twice and differs in the last pass's combination only.

Measured on MI355X (every test prints its ratio): with voxel sizes d^2 at most 0.60 and d at most 0.59 of the derived bounds; means and
ASSD at most 0.095 of theirs; percentiles at most 5.1e-8 relative from np.percentile (criterion 2^-23 = 1.19e-7).
"""

import contextlib
import io

import numpy as np
import pytest
import torch

import edt_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FIXED = [(1, 1, 1), (1, 7, 1), (5, 6, 7), (3, 65, 66), (130, 3, 5), (2, 2, 129), (17, 65), (64, 64), (1, 130)]
ARMS = [(128, 128), (128, 129), (256, 65), (257, 65), (512, 33), (513, 33), (1024, 17), (3, 1024), (2, 1024), (23, 89), (32, 64), (3, 683), (2, 130, 130)]
SMALL = 13000                                       # voxels up to which the dense sets are brute-forced
ids_of = lambda s: 'x'.join(map(str, s))            # noqa: E731
_CACHE = {}


def _ne():
    import neurite_amd as ne
    return ne


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]).numpy() if t.dtype.is_floating_point else t.numpy()


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), '%s is not bit-identical run to run' % k
    else:
        assert np.array_equal(_bits(a), _bits(b)), 'not bit-identical run to run'
    return a


def _same(got, want, what):
    """bit for bit, +-inf included (both are float32 and hold no NaN)"""
    got = got.detach().cpu().numpy()
    want = np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert not np.isnan(want).any()
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _mask(kind, shape, seed=0):
    key = ('mask', kind, shape, seed)
    if key not in _CACHE:
        _CACHE[key] = R.feature_set(kind, shape, seed)
    return _CACHE[key]


def _pos(kind, shape, seed=0, sampling=None):
    """squared distance to the set, float64, made once"""
    key = ('pos', kind, shape, seed, sampling)
    if key not in _CACHE:
        _CACHE[key] = R.sq_dist(_mask(kind, shape, seed), sampling)
    return _CACHE[key]


def _signed(kind, shape, seed=0, sampling=None):
    key = ('signed', kind, shape, seed, sampling)
    if key not in _CACHE:
        m = _mask(kind, shape, seed)
        _CACHE[key] = np.where(m, -R.sq_dist(~m, sampling), _pos(kind, shape, seed, sampling))
    return _CACHE[key]


def _groups(shape):
    """[(kinds of the batch entries, whether the signed transform is brute-forced too)]"""
    voxels = int(np.prod(shape))
    if voxels <= 5000:
        return [((0.5, 0.02, 'ball'), True), (('empty', 'full', 'corners'), True), ((0.02,), True)]
    if voxels <= SMALL:
        return [((0.5, 0.02, 'ball'), False), (('empty', 'full', 'corners'), False), ((0.5,), True), (('empty', 'full', 'empty'), True)]
    return [((0.02, 'corners', 'ball'), False), (('empty', 'full', 'empty'), True), ((0.02,), False)]


# ---- 1. binary volumes at unit spacing: bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', FIXED + ARMS, ids=ids_of)
def test_binary_volumes_at_unit_spacing_are_exact(dev, shape):
    ne = _ne()
    for g, (kinds, signed) in enumerate(_groups(shape)):
        batch = len(kinds)
        m = np.stack([_mask(k, shape) for k in kinds], 0)
        # the three input forms: bool, uint8 with values other than 1, and another dtype (which goes through != 0)
        vol = (torch.tensor(m), torch.tensor(m.astype(np.uint8) * 7), torch.tensor(m.astype(np.float32) * -0.5))[g % 3].to(dev)
        d2 = np.stack([_pos(k, shape) for k in kinds], 0)
        assert float(d2[np.isfinite(d2)].max(initial=0)) < 2 ** 24
        what = '%s %s' % (shape, kinds)
        got = _twice(lambda: ne.utils.dist_trf(vol, squared=True, batched=True))
        assert got.shape == (batch,) + shape
        _same(got, d2.astype(np.float32), what + ' squared')
        _same(_twice(lambda: ne.utils.dist_trf(vol, batched=True)), R.root32(d2), what + ' root')
        _same(ne.utils.dist_trf(vol[0], squared=True), d2[0].astype(np.float32), what + ' unbatched')
        if not signed:
            continue
        s2 = np.stack([_signed(k, shape) for k in kinds], 0)
        _same(_twice(lambda: ne.utils.signed_dist_trf(vol, squared=True, batched=True)), s2.astype(np.float32), what + ' signed squared')
        _same(_twice(lambda: ne.utils.signed_dist_trf(vol, batched=True)), R.root32(s2), what + ' signed root')
        _same(_twice(lambda: ne.utils.vol_to_sdt_batch(vol[..., None])), R.root32(s2)[..., None], what + ' vol_to_sdt_batch')
        _same(ne.utils.vol_to_sdt_batch(vol[..., None], sdt=False), np.abs(R.root32(s2))[..., None], what + ' vol_to_sdt_batch, sdt=False')
        for b in range(batch):
            _same(_twice(lambda: ne.utils.vol_to_sdt(vol[b])), R.root32(s2[b]), what + ' vol_to_sdt')
        _same(ne.utils.vol_to_sdt(vol[0], sdt=False), np.abs(R.root32(s2[0])), what + ' vol_to_sdt, sdt=False')


def test_empty_and_full_sets_deviate_from_scipy_as_documented(dev):
    ne = _ne()
    for shape in ((3, 4), (5, 6, 7)):
        empty, full = torch.zeros(shape, dtype=torch.bool, device=dev), torch.ones(shape, dtype=torch.bool, device=dev)
        for squared in (False, True):
            assert bool(torch.isposinf(ne.utils.dist_trf(empty, squared=squared)).all())
            assert bool((ne.utils.dist_trf(full, squared=squared) == 0).all())
            assert bool(torch.isposinf(ne.utils.signed_dist_trf(empty, squared=squared)).all())
            assert bool(torch.isneginf(ne.utils.signed_dist_trf(full, squared=squared)).all())
        assert bool(torch.isposinf(ne.utils.vol_to_sdt(full, sdt=False)).all())


def test_a_non_contiguous_volume_is_made_contiguous(dev):
    ne = _ne()
    m = torch.tensor(_mask(0.02, (5, 6, 7))).to(dev)
    strided = m.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not strided.is_contiguous() and torch.equal(strided, m)
    for fn in (ne.utils.dist_trf, ne.utils.signed_dist_trf):
        assert np.array_equal(_bits(fn(strided)), _bits(fn(m)))


# ---- 2. label maps ------------------------------------------------------------------------------------------------------------------
def _label_case(shape, nlabels, batch, seed=0):
    """(ids int32 [batch, *shape], label list): the map holds nlabels + 1 regions with ids 2, 5, 8, ..; the list holds the ids of
    regions 1 .. nlabels - 1 and, from two labels on, one id that does not occur (1000); the ids of region 0 and of the last region
    occur but are not in the list"""
    key = ('labels', shape, nlabels, batch, seed)
    if key not in _CACHE:
        ids = np.stack([R.label_map(shape, nlabels + 1, seed + 10 * b, coarse=2) for b in range(batch)], 0) * 3 + 2
        labels = [2 + 3 * v for v in range(1, nlabels)] + [1000] if nlabels > 1 else [5]
        _CACHE[key] = (ids.astype(np.int32), labels)
    return _CACHE[key]


def _label_ref(shape, nlabels, batch, what, seed=0):
    """float64 [batch, *shape, L] squared transforms of every label: 'pos', 'signed' or 'surface'"""
    key = ('label_ref', shape, nlabels, batch, what, seed)
    if key not in _CACHE:
        ids, labels = _label_case(shape, nlabels, batch, seed)
        out = np.empty(ids.shape + (len(labels),))
        for b in range(batch):
            for k, lab in enumerate(labels):
                m = ids[b] == lab
                out[b, ..., k] = R.signed_sq(m) if what == 'signed' else R.sq_dist(R.surface(m) if what == 'surface' else m)
        _CACHE[key] = out
    return _CACHE[key]


LABEL_CASES = [((5, 6, 7), 1, 3), ((5, 6, 7), 3, 3), ((5, 6, 7), 33, 3), ((17, 65), 1, 1), ((17, 65), 3, 3), ((17, 65), 33, 1),
               ((2, 2, 129), 3, 3), ((130, 3, 5), 33, 1), ((3, 65, 66), 3, 1), ((1, 7, 1), 3, 3), ((64, 64), 3, 1)]


@pytest.mark.parametrize('shape,nlabels,batch', LABEL_CASES, ids=lambda v: ids_of(v) if isinstance(v, tuple) else str(v))
def test_label_maps_at_unit_spacing_are_exact(dev, shape, nlabels, batch):
    ne = _ne()
    L = ne._lib
    ids, labels = _label_case(shape, nlabels, batch)
    assert len(labels) == nlabels
    if nlabels > 1:
        assert not (ids == 1000).any() and (ids == 2).any(), 'an absent label and an id outside the list'
    t = torch.tensor(ids).to(dev)
    what = '%s x %d labels' % (shape, nlabels)
    d2 = _label_ref(shape, nlabels, batch, 'pos')
    got = _twice(lambda: ne.utils.label_dist_trf(t, labels, squared=True))
    assert got.shape == (batch,) + shape + (nlabels,)
    _same(got, d2.astype(np.float32), what + ' squared')
    _same(_twice(lambda: ne.utils.label_dist_trf(t, labels)), R.root32(d2), what + ' root')
    if nlabels > 1:
        assert bool(torch.isposinf(got[..., -1]).all()), 'the absent label'
    # int64 ids give the same; a single label agrees with the binary call on its mask
    _same(ne.utils.label_dist_trf(t.long(), labels, squared=True), d2.astype(np.float32), what + ' int64 ids')
    assert np.array_equal(_bits(ne.utils.dist_trf(t == labels[0], squared=True, batched=True)), _bits(got[..., 0]))
    # the surface source (what metrics.SurfaceDistance transforms)
    surf = _twice(lambda: ne.utils._label_dist_trf(t, tuple(labels), None, L.EDT_SURFACE | L.EDT_SQUARED, 'test'))
    _same(surf, _label_ref(shape, nlabels, batch, 'surface').astype(np.float32), what + ' from the surfaces')
    if int(np.prod(shape)) * nlabels <= 8000:
        s2 = _label_ref(shape, nlabels, batch, 'signed')
        _same(_twice(lambda: ne.utils.label_dist_trf(t, labels, signed=True, squared=True)), s2.astype(np.float32), what + ' signed squared')
        _same(_twice(lambda: ne.utils.label_dist_trf(t, labels, signed=True)), R.root32(s2), what + ' signed root')


# ---- 3. voxel sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 6, 7), (3, 65, 66), (130, 3, 5), (2, 2, 129), (17, 65), (64, 64), (1, 130), (128, 129), (257, 65)],
                         ids=ids_of)
def test_sampling_within_the_derived_bound(dev, shape):
    """every term fl(fl(s d)^2) and each of the (at most two) additions rounds once and all terms are positive: d^2 within
    6 * 2^-24 d^2 and d within 4 * 2^-24 d of the float64 restatement at the float32 voxel sizes.  Measured on MI355X: at most 0.60 and
    0.59 of the bounds."""
    ne = _ne()
    small = int(np.prod(shape)) <= 5000                                          # (the float64 brute force makes one pass per axis)
    kinds = (0.5, 0.02, 'ball') if small else (0.02, 'corners')
    vol = torch.tensor(np.stack([_mask(k, shape) for k in kinds], 0)).to(dev)
    for sampling in ((1.5, 1, 2)[:len(shape)], (0.3, 1.7, 0.9)[-len(shape):], 0.75):
        key = tuple(sampling) if isinstance(sampling, tuple) else sampling
        refs = [np.stack([_pos(k, shape, 0, key) for k in kinds], 0)]
        calls = [ne.utils.dist_trf]
        if small and sampling == (1.5, 1, 2)[:len(shape)]:
            refs.append(np.stack([_signed(k, shape, 0, key) for k in kinds], 0))
            calls.append(ne.utils.signed_dist_trf)
        for fn, want2 in zip(calls, refs):
            got2 = _twice(lambda: fn(vol, sampling=sampling, squared=True, batched=True)).cpu().numpy().astype(np.float64)
            got = _twice(lambda: fn(vol, sampling=sampling, batched=True)).cpu().numpy().astype(np.float64)
            want = np.sign(want2) * np.sqrt(np.abs(want2))
            nz = (want2 != 0) & np.isfinite(want2)                               # (0 on the set and +-inf without one: exactly)
            assert np.array_equal(got2[~nz], want2[~nz]) and np.array_equal(got[~nz], want[~nz])
            r2 = float((np.abs(got2[nz] - want2[nz]) / (6 * U * np.abs(want2[nz]))).max(initial=0))
            r1 = float((np.abs(got[nz] - want[nz]) / (4 * U * np.abs(want[nz]))).max(initial=0))
            print('%s sampling %s %s: worst |err| / bound = %.3g (d^2), %.3g (d)' % (shape, sampling, fn.__name__, r2, r1))
            assert r2 <= 1.0 and r1 <= 1.0, (r2, r1)
    # sampling 1 is unit spacing, bit for bit
    assert np.array_equal(_bits(ne.utils.dist_trf(vol, sampling=1, batched=True)), _bits(ne.utils.dist_trf(vol, batched=True)))


# ---- 4. surface distances -------------------------------------------------------------------------------------------------------------
PERCENTILES = (0, 50, 95, 100)


def _pair(shape, nlabels, batch, seed=0):
    """two label maps of one case: y_true as _label_case makes it, y_pred shifted by a voxel or two with 2 % of its voxels redrawn"""
    key = ('pair', shape, nlabels, batch, seed)
    if key not in _CACHE:
        t, labels = _label_case(shape, nlabels, batch, seed)
        rng = np.random.default_rng(seed + 1)
        p = np.roll(t, (1, 2, 1)[:len(shape)], axis=tuple(range(1, len(shape) + 1)))
        redraw = rng.random(p.shape) < 0.02
        p = np.where(redraw, rng.integers(0, nlabels + 1, p.shape) * 3 + 2, p).astype(np.int32)
        _CACHE[key] = (t, p, labels)
    return _CACHE[key]


def _blobs(shape):
    """two maps with one small box of label 1 each, 3 and 4 voxels apart: few surface voxels in a large volume"""
    t, p = np.zeros((1,) + shape, np.int32), np.zeros((1,) + shape, np.int32)
    c = [n // 2 for n in shape]
    t[(0,) + tuple(slice(v - 4, v + 3) for v in c)] = 1
    p[(0,) + tuple(slice(v - 1, v + 7) for v in c)] = 1
    return t, p, [1]


def _check_metrics(dev, t, p, labels, what, voxel_size=None):
    ne = _ne()
    want = R.surface_metrics(t, p, labels, voxel_size, PERCENTILES)
    td, pd = torch.tensor(t).to(dev), torch.tensor(p).to(dev)
    unit = voxel_size is None
    got = None
    for j, q in enumerate(PERCENTILES):
        sd = ne.metrics.SurfaceDistance(labels, voxel_size=voxel_size, percentile=q)
        got = _twice(lambda: sd.distances(td, pd))
        hp = got['hd_percentile'].cpu().numpy()
        ref = want['hd_percentile'][j]
        assert hp.dtype == np.float32 and np.array_equal(np.isnan(hp), np.isnan(ref))
        ok = ~np.isnan(ref)
        err = np.abs(hp.astype(np.float64) - ref)[ok]
        print('%s percentile %g: worst relative error %.3g (bound %.3g)' % (what, q, float((err / np.maximum(ref[ok], 1e-300)).max(initial=0)),
                                                                          2.0 ** -23))
        assert np.all(err <= 2.0 ** -23 * ref[ok])
        assert np.array_equal(_bits(sd.hd95(td, pd)), _bits(got['hd_percentile']))
        if q == 100:
            assert np.array_equal(_bits(got['hd_percentile']), _bits(got['hausdorff'])), 'the 100th percentile is the Hausdorff distance'
    assert sorted(got) == sorted(['count_t', 'count_p', 'max_tp', 'max_pt', 'mean_tp', 'mean_pt', 'hausdorff', 'assd', 'hd_percentile'])
    for k in ('count_t', 'count_p'):
        assert got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    empty = (want['count_t'] == 0) | (want['count_p'] == 0)
    for k in ('max_tp', 'max_pt', 'hausdorff', 'mean_tp', 'mean_pt', 'assd'):
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == empty.shape and np.array_equal(np.isnan(g), empty), k
    ok = ~empty
    for k in ('max_tp', 'max_pt', 'hausdorff'):
        g = got[k].cpu().numpy()[ok]
        if unit:                                                                 # the float32 root of the largest integer square
            assert np.array_equal(g, np.sqrt(np.round(want[k][ok] ** 2).astype(np.float32))), k
        else:
            assert np.all(np.abs(g - want[k][ok]) <= 2.0 ** -23 * want[k][ok]), k
    nt, npd = want['count_t'][ok].astype(np.float64), want['count_p'][ok].astype(np.float64)
    for k, n, total in (('mean_tp', nt, want['sum_tp'][ok]), ('mean_pt', npd, want['sum_pt'][ok]),
                        ('assd', nt + npd, want['sum_tp'][ok] + want['sum_pt'][ok])):
        err = np.abs(got[k].cpu().numpy()[ok].astype(np.float64) - want[k][ok])
        bound = (n + 2) * U * total / n                                          # (n + 2) 2^-24 sum |d| on the sum, carried to the mean
        print('%s %s: worst |err| / bound = %.3g' % (what, k, float((err / np.maximum(bound, 1e-300)).max(initial=0))))
        assert np.all(err <= bound), k
    sd = ne.metrics.SurfaceDistance(labels, voxel_size=voxel_size)
    assert np.array_equal(_bits(sd.hausdorff(td, pd)), _bits(got['hausdorff'])) and np.array_equal(_bits(sd.assd(td, pd)), _bits(got['assd']))
    return got, want


METRIC_CASES = [((5, 6, 7), 3, 3), ((17, 65), 3, 3), ((8, 20, 21), 33, 1), ((23, 89), 1, 3), ((32, 64), 1, 3), ((3, 683), 1, 3),
                ((2, 2, 129), 3, 1), ((1, 7, 1), 3, 3)]


@pytest.mark.parametrize('shape,nlabels,batch', METRIC_CASES, ids=lambda v: ids_of(v) if isinstance(v, tuple) else str(v))
def test_surface_distances_at_unit_spacing(dev, shape, nlabels, batch):
    """counts exact, maxima bit for bit, means within (n + 2) 2^-24 sum |d| / n, percentiles within 2^-23 relative of np.percentile.
    Measured on MI355X: means at most 0.095 of the bound, percentiles at most 5.1e-8 relative."""
    t, p, labels = _pair(shape, nlabels, batch)
    got, want = _check_metrics(dev, t, p, labels, '%s x %d' % (shape, nlabels))
    if nlabels > 1:
        assert want['count_t'][:, -1].max() == 0 and bool(torch.isnan(got['hausdorff'][:, -1]).all()), 'an absent label: NaN, count 0'
        assert (want['count_t'] > 0).any()


def test_surface_distances_over_more_than_256_runs(dev):
    t, p, labels = _blobs((725, 725))
    got, want = _check_metrics(dev, t, p, labels, '725x725 boxes')
    assert want['count_t'][0, 0] == 24 and want['count_p'][0, 0] == 28 and float(got['hausdorff'][0, 0]) == float(np.sqrt(np.float32(32)))


def test_one_and_two_surface_voxels_and_a_bool_mask(dev):
    ne = _ne()
    t, p = np.zeros((2, 9, 10, 11), bool), np.zeros((2, 9, 10, 11), bool)
    t[0, 1, 1, 1] = p[0, 4, 5, 1] = True                                          # one voxel each, (3, 4, 0) apart
    t[1, 2, 2, 2] = t[1, 2, 2, 3] = p[1, 8, 2, 2] = True                          # two voxels against one
    for q in (100, 95, 0):
        sd = ne.metrics.SurfaceDistance([1], percentile=q)
        got = _twice(lambda: sd.distances(torch.tensor(t).to(dev), torch.tensor(p).to(dev)))
        want = R.surface_metrics(t.astype(np.int32), p.astype(np.int32), [1], None, (q,))
        assert got['count_t'].cpu().tolist() == [[1], [2]] and got['count_p'].cpu().tolist() == [[1], [1]]
        assert got['hausdorff'].cpu().tolist() == [[5.0], [float(np.sqrt(np.float32(37)))]]
        assert np.all(np.abs(got['hd_percentile'].cpu().numpy() - want['hd_percentile'][0]) <= 2.0 ** -23 * want['hd_percentile'][0])
        if q == 100:
            assert np.array_equal(_bits(got['hd_percentile']), _bits(got['hausdorff']))
    # identical maps: every distance is 0
    same = ne.metrics.SurfaceDistance([1]).distances(torch.tensor(t).to(dev), torch.tensor(t).to(dev))
    assert all(float(same[k].abs().max()) == 0 for k in ('hausdorff', 'assd', 'hd_percentile', 'mean_tp'))


def test_voxel_sizes_of_the_surface_distances(dev):
    ne = _ne()
    t, p, labels = _pair((5, 6, 7), 3, 3)
    # isotropic: the unit-spacing transform, scaled; every key is there
    _check_metrics(dev, t, p, labels, '5x6x7 voxel size 0.75', voxel_size=0.75)
    # anisotropic: the percentile needs the integer histogram and says so; the other keys are returned
    sd = ne.metrics.SurfaceDistance(labels, voxel_size=(1.5, 1, 2))
    td, pd = torch.tensor(t).to(dev), torch.tensor(p).to(dev)
    got = _twice(lambda: sd.distances(td, pd))
    with pytest.raises(NotImplementedError):
        got['hd_percentile']
    with pytest.raises(NotImplementedError):
        sd.hd95(td, pd)
    want = R.surface_metrics(t, p, labels, (1.5, 1, 2), ())
    ok = (want['count_t'] > 0) & (want['count_p'] > 0)
    assert ok.any()
    for k in ('count_t', 'count_p'):
        assert np.array_equal(got[k].cpu().numpy(), want[k])
    for k in ('max_tp', 'max_pt', 'hausdorff', 'mean_tp', 'mean_pt', 'assd'):
        g = got[k].cpu().numpy()
        assert np.array_equal(np.isnan(g), ~ok), k
        assert np.all(np.abs(g[ok] - want[k][ok]) <= 5 * U * want[k][ok]), k      # 4 2^-24 on every distance, and the rounding to float32


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------------
def test_transform_and_surface_distances_capture_into_one_graph(dev):
    ne = _ne()
    t, p, labels = _pair((17, 65), 3, 3)
    first = [torch.tensor(a).to(dev) for a in (t, p, _mask(0.02, (3, 17, 65)))]
    second = [torch.tensor(a).to(dev) for a in (p, t, _mask(0.5, (3, 17, 65)))]
    T, P, M = (x.clone() for x in first)
    sd = ne.metrics.SurfaceDistance(labels)

    def step():
        out = sd.distances(T, P)
        return [ne.utils.dist_trf(M, batched=True), ne.utils.signed_dist_trf(M, batched=True)] + [out[k] for k in sorted(out)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                           # workspace growth and the label list's copy: outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    for values in (second, first):
        for dst, src in zip((T, P, M), values):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        got = [_bits(x) for x in captured]
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert np.array_equal(a, _bits(b))


# ---- 6. the loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 6, 7), (17, 65), (16, 16, 16)], ids=ids_of)
def test_signed_distance_mse_in_both_input_forms(dev, shape):
    ne = _ne()
    batch = 3
    ids, _ = _label_case(shape, 3, batch)
    fg = [5, 8, 1000]                                                            # two regions and an id that does not occur
    V = int(np.prod(shape))
    rng = np.random.default_rng(3)
    pred = torch.tensor((3.0 * rng.standard_normal((batch,) + shape + (1,))).astype(np.float32))
    for max_dist, voxel_size in ((None, None), (2.5, None), (4.0, (1.5, 1, 2)[:len(shape)])):
        samp = None if voxel_size is None else tuple(voxel_size)
        s2 = np.stack([R.signed_sq(np.isin(ids[b], fg), samp) for b in range(batch)], 0)
        target = np.sign(s2) * np.sqrt(np.abs(s2))
        assert np.isfinite(target).all()
        if max_dist is not None:
            target = np.clip(target, -max_dist, max_dist)
        if samp is None:
            target = target.astype(np.float32).astype(np.float64)                # (exact squares: the device's root is this one)
        target = torch.tensor(target)
        want = ((pred[..., 0].double() - target) ** 2).flatten(1).mean(1)
        want_grad = 2.0 * (pred[..., 0].double() - target) / V
        mse = ne.losses.SignedDistanceMSE(fg, max_dist=max_dist, voxel_size=voxel_size)
        ids_d = torch.tensor(ids).to(dev)
        stacked = torch.cat([pred, torch.tensor(ids.astype(np.float32))[..., None]], -1).to(dev).requires_grad_(True)
        leaf = pred.to(dev).requires_grad_(True)
        forms = ((ids_d, leaf, leaf), (ids_d[..., None], leaf, leaf), (ids_d.long(), leaf, leaf), (None, stacked, stacked))
        for y_true, y_pred, wrt in forms:
            got = _twice(lambda: mse.loss(y_true, y_pred))
            assert got.shape == (batch,) and got.dtype == torch.float32
            rel = float(((got.detach().cpu().double() - want).abs() / want).max())
            tol = 1e-6 if samp is None else 1e-6 + 8 * U                         # (with voxel sizes the target itself is within 4 2^-24)
            assert rel <= tol, (rel, max_dist, voxel_size)
            grad, = torch.autograd.grad(got.sum(), (wrt,))
            gp = grad[..., 0].cpu().double()
            assert float((gp - want_grad).abs().max()) <= tol * float(want_grad.abs().max())
            if wrt is stacked:
                assert float(grad[..., 1].abs().max()) == 0.0, 'no gradient reaches the ids'
        assert np.array_equal(_bits(mse.target(ids_d)), _bits(mse.target(ids_d.long())))
    # inside multiple_losses_decorator: the weighted sum of what each gives alone
    a, b = ne.losses.SignedDistanceMSE([5], max_dist=3.0), ne.losses.SignedDistanceMSE([8, 5])
    both = ne.losses.multiple_losses_decorator([a.loss, b.loss], [1.0, 0.25])
    total = both(ids_d, leaf)
    assert np.allclose(total.detach().cpu().numpy(), (a.loss(ids_d, leaf) + 0.25 * b.loss(ids_d, leaf)).detach().cpu().numpy(), rtol=1e-6)
    assert total.requires_grad


def test_synthstrip_trains_end_to_end(dev):
    ne = _ne()
    from neurite_amd import synth
    labels = [0, 1, 2, 3]
    S, B = 16, 2
    lab = torch.stack([synth.blob_labels(1 + b, size=S, nb_labels=len(labels), coarse=4, device=dev) for b in range(B)], 0)
    lab = torch.tensor(labels, device=dev)[lab.long()][..., None].to(torch.int32)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ne.models.SynthStrip((S, S, S), labels, {1: 1, 2: 1, 3: 1}, nb_unet_features=4, nb_unet_levels=2,
                                     gen_args=dict(seeds=dict(warp=2, mean=3)))
    model = model.to(dev).train()
    out = model(lab)
    assert out.shape == (B, S, S, S, 2) and out.requires_grad
    mse = ne.losses.SignedDistanceMSE(1, max_dist=5.0)
    loss = mse.loss(None, out)
    assert loss.shape == (B,) and bool(torch.isfinite(loss).all())
    # the target is the restatement's on the label channel the model returned
    seg = out[..., 1].detach().cpu().numpy()
    s2 = np.stack([R.signed_sq(seg[b] == 1) for b in range(B)], 0)
    want = np.clip(R.root32(s2), -5.0, 5.0)
    assert np.array_equal(mse.target(out[..., 1].detach().to(torch.int32)).cpu().numpy(), want.astype(np.float32))
    loss.mean().backward()
    grads = [q.grad for q in model.unet.parameters() if q.requires_grad]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
