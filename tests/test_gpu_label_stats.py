"""
utils.label_stats / label_volumes / label_centroids, metrics.LabelOverlap and synthesis.intensity_priors (csrc/labelstats.hip) on the GPU
against the definition of tests/label_stats_restatement.py.

Exact, always: counts, coordinate sums, boxes and the whole confusion matrix.  Bit for bit: sum and sumsq on integer-valued images (every
order is exact there), mean and std against the float64 expressions on the kernel's own sums.  By value: min and max.  On float images
the sums are held to the order-free bound of any float32 summation: |sum - exact| <= (n + 2) 2^-24 sum|x| and
|sumsq - exact| <= (n + 3) 2^-24 sum x^2 with n the label's count (n - 1 additions, one rounding of each square, the higher-order terms);
the largest observed fraction of the bound is printed (DESIGN 4.6n quotes it).

Shapes, the smallest at which each mechanism can go wrong: (2, 7, 9, 11) nothing divides 4 or 64; (1, 5, 6, 130) rows cross wave
boundaries; (3, 33, 65) 2-D; (2, 16, 16, 16) everything aligned; (1, 40, 48, 56) 27 blocks, so more than one partial row per entry.
Label counts 1, 3, 33 and 256, and for the confusion 111 and 112, the two sides of its LDS-table crossover; each with the ids 0 .. L - 1
and with an unsorted list of arbitrary ids (0, 2035, 41, -7, ...).
"""

import contextlib
import io
import warnings

import numpy as np
import pytest
import torch

import label_stats_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TORCH_DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float16': torch.float16}
SHAPE_IDS = ['x'.join(map(str, s)) for s in R.SHAPES]


def _ne():
    import neurite_amd as ne
    return ne


def _labels(slots, listed):
    return list(slots) if listed else len(slots)


def _image_tensor(image, dtype, dev):
    """(device tensor stored as dtype, the float32 values it stands for)"""
    stored, values = R.store(image, dtype)
    if dtype == 'bfloat16':
        return torch.from_numpy(np.ascontiguousarray(stored).view(np.int16)).to(dev).view(torch.bfloat16), values
    return torch.from_numpy(np.ascontiguousarray(stored)).to(dev), values


def _ids_tensor(ids, dev):
    return torch.from_numpy(np.array(ids)).to(dev)               # (a copy: the shared cases are read-only)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same_values(got, want):
    """equal by value: zeros of either sign count as equal, infinities compare as themselves"""
    return got.shape == want.shape and bool(np.all(got == want))


def _check_integers(got, want, shape, tag):
    nd = len(shape) - 1
    assert got['count'].dtype == np.int64 and got['coord_sum'].dtype == np.int64 and got['bbox_min'].dtype == np.int32, tag
    assert np.array_equal(got['count'], want['count']), tag
    assert np.array_equal(got['coord_sum'], want['coord_sums']), tag
    assert np.array_equal(got['bbox_min'], want['bbox_min']) and np.array_equal(got['bbox_max'], want['bbox_max']), tag
    empty = want['count'] == 0
    assert np.all(got['bbox_min'][empty] == np.asarray(shape[1:])) and np.all(got['bbox_max'][empty] == -1), tag
    with np.errstate(invalid='ignore', divide='ignore'):
        centroid = got['coord_sum'].astype(np.float64) / got['count'].astype(np.float64)[..., None]
    assert got['centroid'].dtype == np.float64 and got['centroid'].shape == got['count'].shape + (nd,), tag
    assert np.array_equal(got['centroid'], centroid, equal_nan=True) and np.all(np.isnan(got['centroid'][empty])), tag


def _check_moments(got, tag):
    """mean and std equal, bit for bit, the float64 expressions on the kernel's own sum, sumsq and count"""
    n = got['count'].astype(np.float64)[..., None]
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = got['sum'] / n
        std = np.sqrt(np.maximum(0.0, got['sumsq'] / n - mean * mean))
    assert got['mean'].dtype == np.float64 and got['std'].dtype == np.float64, tag
    assert np.array_equal(got['mean'].view(np.int64)[~np.isnan(mean)], mean.view(np.int64)[~np.isnan(mean)]), tag
    assert np.array_equal(np.isnan(got['mean']), np.isnan(mean)) and np.array_equal(np.isnan(got['std']), np.isnan(std)), tag
    assert np.array_equal(got['std'].view(np.int64)[~np.isnan(std)], std.view(np.int64)[~np.isnan(std)]), tag
    assert np.all(np.isnan(got['mean'][got['count'] == 0])) and np.all(np.isnan(got['std'][got['count'] == 0])), tag


@pytest.mark.parametrize('listed', (False, True), ids=('range', 'listed'))
@pytest.mark.parametrize('n', R.LABEL_COUNTS)
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_integer_statistics_are_exact(dev, shape, n, listed):
    ne = _ne()
    voxel_size = (0.5, 1.25, 2.0)[:len(shape) - 1]
    for kind in R.KINDS:
        slots, ids, want = R.case(kind, shape, n, listed)
        t = _ids_tensor(ids, dev)
        labels = _labels(slots, listed)
        got = _np(ne.utils.label_stats(t, labels=labels, voxel_size=voxel_size, batched=True))
        tag = (kind, shape, n, listed)
        assert set(got) == {'count', 'volume', 'centroid', 'coord_sum', 'bbox_min', 'bbox_max'}, tag
        _check_integers(got, want, shape, tag)
        assert got['volume'].dtype == np.float64 and np.array_equal(got['volume'], want['count'] * float(np.prod(voxel_size))), tag
        assert got['count'].sum() <= np.prod(shape) and (kind in ('outside', 'absent') or got['count'].sum() == np.prod(shape)), tag
    # the thin wrappers, other integer dtypes, and one entry without the batch axis
    slots, ids, want = R.case('blobs', shape, n, listed)
    t = _ids_tensor(ids, dev)
    assert torch.equal(ne.utils.label_volumes(t, labels, voxel_size, batched=True).cpu(),
                       torch.from_numpy(want['count'] * float(np.prod(voxel_size))))
    centroid = ne.utils.label_centroids(t.to(torch.int64), labels, batched=True).cpu().numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.array_equal(centroid, want['coord_sums'] / want['count'].astype(np.float64)[..., None], equal_nan=True)
    one = _np(ne.utils.label_stats(t[0], labels=labels))
    assert one['count'].shape == (n,) and one['bbox_min'].shape == (n, len(shape) - 1)
    _check_integers({k: v[None] for k, v in one.items()}, {k: v[:1] for k, v in want.items()}, (1,) + shape[1:], 'unbatched')
    assert ne.utils.label_volumes(t[0], labels).shape == (n,) and ne.utils.label_centroids(t[0], labels).shape == (n, len(shape) - 1)


# (n, listed, kind of id map, channels, storage)
IMAGE_CASES = ((33, True, 'blobs', 3, 'float32'), (3, False, 'iid', None, 'bfloat16'), (256, True, 'outside', 4, 'float16'),
               (1, False, 'constant', 1, 'float32'), (33, False, 'absent', 4, 'bfloat16'), (256, False, 'blobs', None, 'float32'))


@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_integer_valued_images_bit_for_bit(dev, shape):
    """sums of small integers are exact in every float32 order: sum and sumsq equal the definition's bits"""
    ne = _ne()
    for n, listed, kind, channels, dtype in IMAGE_CASES:
        slots, ids, _ = R.case(kind, shape, n, listed)
        x, values = _image_tensor(R.make_image(shape, channels, 'small'), dtype, dev)
        values = values if channels is not None else values[..., None]
        want = R.stats(ids, values, slots)
        assert want['sumsq'].max() < 2 ** 24
        got = _np(ne.utils.label_stats(_ids_tensor(ids, dev), x, _labels(slots, listed), batched=True))
        tag = (shape, n, listed, kind, channels, dtype)
        c = 1 if channels is None else channels
        assert got['sum'].shape == (shape[0], n, c) and got['sum'].dtype == np.float64 and got['min'].dtype == np.float32, tag
        _check_integers(got, want, shape, tag)
        assert np.array_equal(got['sum'].view(np.int64), (want['sum'] + 0.0).view(np.int64)), tag               # (+ 0.0: one zero)
        assert np.array_equal(got['sumsq'].view(np.int64), want['sumsq'].view(np.int64)), tag
        assert _same_values(got['min'], want['min']) and _same_values(got['max'], want['max']), tag
        _check_moments(got, tag)
        full = want['count'] > 0
        x64 = values.astype(np.float64)
        for e in range(shape[0]):
            for l in np.nonzero(full[e])[0]:
                sel = x64[e][ids[e] == slots[l]]
                assert np.allclose(got['mean'][e, l], sel.mean(0), rtol=1e-12, atol=0) or np.all(sel.mean(0) == got['mean'][e, l]), tag
                assert np.allclose(got['std'][e, l], sel.std(0), rtol=1e-12, atol=1e-300), tag


@pytest.mark.parametrize('dtype', list(TORCH_DTYPES))
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_float_images_within_the_order_free_bound(dev, shape, dtype):
    ne = _ne()
    worst = 0.0
    for n, listed, kind, channels in ((33, True, 'blobs', 3), (3, False, 'iid', 1), (256, True, 'outside', 4), (1, True, 'constant', None)):
        slots, ids, _ = R.case(kind, shape, n, listed)
        x, values = _image_tensor(R.make_image(shape, channels, 'normal'), dtype, dev)
        values = values if channels is not None else values[..., None]
        want = R.stats(ids, values, slots)
        got = _np(ne.utils.label_stats(_ids_tensor(ids, dev), x, _labels(slots, listed), batched=True))
        tag = (shape, dtype, n, listed, kind, channels)
        _check_integers(got, want, shape, tag)
        count = want['count'].astype(np.float64)[..., None]
        bound_sum, bound_sq = (count + 2) * U * want['abs_sum'], (count + 3) * U * want['sumsq']
        err_sum, err_sq = np.abs(got['sum'] - want['sum']), np.abs(got['sumsq'] - want['sumsq'])
        assert np.all(err_sum <= bound_sum) and np.all(err_sq <= bound_sq), tag
        present = want['count'] > 0
        worst = max(worst, float((err_sum[present] / bound_sum[present]).max()), float((err_sq[present] / bound_sq[present]).max()))
        assert np.all(got['sum'][~present] == 0) and np.all(got['sumsq'][~present] == 0), tag
        assert _same_values(got['min'], want['min']) and _same_values(got['max'], want['max']), tag
        _check_moments(got, tag)
    print('label_stats %s %s: largest error / bound = %.3g' % (shape, dtype, worst))


@pytest.mark.parametrize('dtype', list(TORCH_DTYPES))
def test_nan_is_skipped_by_min_max_and_propagates_into_the_sums(dev, dtype):
    ne = _ne()
    shape = R.SHAPES[0]
    slots, ids, _ = R.case('iid', shape, 3, True)
    image = R.make_image(shape, 2, 'small').copy()
    image[..., 0][(ids == slots[0]) & (np.random.default_rng(3).random(shape) < 0.3)] = np.nan               # some NaNs in one label
    image[..., 1][ids == slots[1]] = np.nan                                                                  # a label that is all NaN
    x, values = _image_tensor(image, dtype, dev)
    want = R.stats(ids, values, slots)
    got = _np(ne.utils.label_stats(_ids_tensor(ids, dev), x, list(slots), batched=True))
    assert _same_values(got['min'], want['min']) and _same_values(got['max'], want['max'])
    assert np.all(got['min'][:, 1, 1] == np.inf) and np.all(got['max'][:, 1, 1] == -np.inf) and np.all(np.isfinite(got['min'][:, 0, 0]))
    assert np.array_equal(np.isnan(got['sum']), np.isnan(want['sum'])) and np.isnan(got['sum'][:, 0, 0]).all() and np.isnan(got['sum'][:, 1, 1]).all()
    assert np.array_equal(np.isnan(got['sumsq']), np.isnan(want['sumsq']))
    clean = ~np.isnan(want['sum'])
    assert np.array_equal(got['sum'][clean], want['sum'][clean]) and np.array_equal(got['sumsq'][clean], want['sumsq'][clean])
    assert np.isnan(got['mean'][:, 1, 1]).all() and np.isnan(got['std'][:, 0, 0]).all()


def test_misaligned_inputs_give_the_same_results(dev):
    """an id map and an image that start one element into a larger buffer"""
    ne = _ne()
    shape = R.SHAPES[0]
    slots, ids, _ = R.case('blobs', shape, 33, True)
    t = _ids_tensor(ids, dev)
    other = _ids_tensor(R.case('outside', shape, 33, True)[1], dev)
    overlap = ne.metrics.LabelOverlap(list(slots))
    for dtype in TORCH_DTYPES:
        x, _ = _image_tensor(R.make_image(shape, 3, 'normal'), dtype, dev)
        want = ne.utils.label_stats(t, x, list(slots), batched=True)
        buf_t = torch.zeros(t.numel() + 1, dtype=torch.int32, device=dev)
        buf_x = torch.zeros(x.numel() + 1, dtype=x.dtype, device=dev)
        buf_t[1:] = t.reshape(-1)
        buf_x[1:] = x.reshape(-1)
        t1, x1 = buf_t[1:].view(t.shape), buf_x[1:].view(x.shape)
        assert t1.data_ptr() % 8 == 4 and x1.data_ptr() % (2 * x.element_size()) == x.element_size() and t1.is_contiguous()
        got = ne.utils.label_stats(t1, x1, list(slots), batched=True)
        for key in want:
            assert torch.equal(got[key], want[key]) or bool(((got[key] == want[key]) | (got[key].isnan() & want[key].isnan())).all()), (dtype, key)
        buf_o = torch.zeros(t.numel() + 1, dtype=torch.int32, device=dev)
        buf_o[1:] = other.reshape(-1)
        assert torch.equal(overlap.confusion(t1, buf_o[1:].view(t.shape)), overlap.confusion(t, other))


def _bits(d):
    return {k: v.contiguous().view(torch.int64 if v.dtype == torch.float64 else torch.int32 if v.dtype == torch.float32 else v.dtype)
            for k, v in d.items()}


def test_two_runs_are_identical(dev):
    ne = _ne()
    shape = R.SHAPES[4]
    for n, listed, kind in ((33, True, 'blobs'), (256, False, 'iid')):
        slots, ids, _ = R.case(kind, shape, n, listed)
        t = _ids_tensor(ids, dev)
        x, _ = _image_tensor(R.make_image(shape, 4, 'normal'), 'float32', dev)
        a, b = [_bits(ne.utils.label_stats(t, x, _labels(slots, listed), batched=True)) for _ in range(2)]
        for key in a:
            assert torch.equal(a[key], b[key]), (n, key)
        overlap = ne.metrics.LabelOverlap(_labels(slots, listed))
        assert torch.equal(overlap.confusion(t, t.flip(1)), overlap.confusion(t, t.flip(1)))


CONFUSION_COUNTS = R.LABEL_COUNTS + (111, 112)                    # 111 / 112: the two sides of the LDS-table crossover


@pytest.mark.parametrize('listed', (False, True), ids=('range', 'listed'))
@pytest.mark.parametrize('n', CONFUSION_COUNTS)
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_confusion_matrix_is_exact(dev, shape, n, listed):
    ne = _ne()
    slots, a, b, want = R.confusion_case(shape, n, listed)
    labels = _labels(slots, listed)
    overlap = ne.metrics.LabelOverlap(labels)
    ta, tb = _ids_tensor(a, dev), _ids_tensor(b, dev)
    got = overlap.confusion(ta, tb)
    assert got.dtype == torch.int64 and got.shape == (shape[0], n + 1, n + 1)
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    voxels = int(np.prod(shape[1:]))
    assert all(int(got[e].sum()) == voxels for e in range(shape[0]))
    # the row and column sums are the counts of label_stats on each map
    count_a = ne.utils.label_stats(ta, labels=labels, batched=True)['count'].cpu().numpy()
    count_b = ne.utils.label_stats(tb, labels=labels, batched=True)['count'].cpu().numpy()
    assert np.array_equal(got.sum(2)[:, :n], count_a) and np.array_equal(got.sum(1)[:, :n], count_b)
    assert np.array_equal(got.sum(2)[:, n], voxels - count_a.sum(1)) and np.array_equal(got.sum(1)[:, n], voxels - count_b.sum(1))
    # other integer dtypes, and the transposed pair
    assert np.array_equal(overlap.confusion(tb.to(torch.int64), ta.to(torch.int64)).cpu().numpy(), want.transpose(0, 2, 1))
    # the scores: the float64 formulas on the matrix
    scores = _np(overlap.scores(ta, tb))
    table = got.astype(np.float64)
    tp = np.stack([np.diag(table[e])[:n] for e in range(shape[0])])
    n_t, n_p = table.sum(2)[:, :n], table.sum(1)[:, :n]
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = {'dice': 2.0 * tp / (n_t + n_p), 'jaccard': tp / (n_t + n_p - tp), 'sensitivity': tp / n_t, 'precision': tp / n_p,
               'volume_similarity': 1.0 - np.abs(n_p - n_t) / (n_p + n_t), 'count_true': n_t, 'count_pred': n_p}
    assert set(scores) == set(ref)
    for key, value in ref.items():
        assert scores[key].dtype == np.float64 and scores[key].shape == (shape[0], n), key
        assert np.array_equal(scores[key], value, equal_nan=True), (key, shape, n, listed)
    assert np.array_equal(np.isnan(scores['dice']), (n_t + n_p) == 0) and np.array_equal(np.isnan(scores['sensitivity']), n_t == 0)


@pytest.mark.parametrize('n', (3, 33, 256))
def test_dice_score_agrees_with_the_hard_dice_metric(dev, n):
    """both are at most three float32 roundings away from the same ratio of exact integers"""
    ne = _ne()
    shape = R.SHAPES[3]
    _, a, _ = R.case('iid', shape, n, False)
    _, b, _ = R.case('blobs', shape, n, False)
    b = np.where(np.random.default_rng(n).random(shape) < 0.5, a, b).astype(np.int32)                         # (half of the voxels agree)
    ta, tb = _ids_tensor(a, dev), _ids_tensor(b, dev)
    mine = ne.metrics.LabelOverlap(n).scores(ta, tb)['dice'].cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        theirs = ne.metrics.Dice(dice_type='hard', input_type='max_label', nb_labels=n).dice(ta, tb).cpu().numpy().astype(np.float64)
    assert theirs.shape == mine.shape == (shape[0], n) and not np.isnan(mine).any() and (mine > 0).any()
    assert np.all(np.abs(theirs - mine) <= 2.0 ** -22 * np.abs(mine))


def test_label_stats_and_confusion_capture_into_one_graph(dev):
    ne = _ne()
    shape = R.SHAPES[4]
    slots = R.slot_ids(33, True)
    maps = [_ids_tensor(R.case(kind, shape, 33, True)[1], dev) for kind in ('blobs', 'outside')]
    images = [_image_tensor(R.make_image(shape, 2, 'normal', seed=s), 'float32', dev)[0] for s in (0, 1)]
    overlap = ne.metrics.LabelOverlap(slots)

    def run(ids, other, image):
        return dict(ne.utils.label_stats(ids, image, slots, batched=True), confusion=overlap.confusion(ids, other))

    eager = [_bits(run(maps[k], maps[1 - k], images[k])) for k in (0, 1)]
    ids, other, image = maps[0].clone(), maps[1].clone(), images[0].clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(ids, other, image)                                                      # (warm-up: workspaces and the device are set up)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(ids, other, image)
    for k in (1, 0):
        ids.copy_(maps[k])
        other.copy_(maps[1 - k])
        image.copy_(images[k])
        graph.replay()
        torch.cuda.synchronize(dev)
        got = _bits(out)
        for key, want in eager[k].items():
            assert torch.equal(got[key], want), (k, key)


def test_results_carry_no_grad(dev):
    ne = _ne()
    shape = R.SHAPES[0]
    slots, ids, _ = R.case('blobs', shape, 3, False)
    image = torch.from_numpy(R.make_image(shape, 1, 'normal')).to(dev).requires_grad_(True)
    got = ne.utils.label_stats(_ids_tensor(ids, dev), image, 3, batched=True)
    assert not any(v.requires_grad for v in got.values())


def test_intensity_priors(dev):
    ne = _ne()
    labels = [12, 0, 7, 3]                                                          # unsorted: the results follow np.unique's order
    order = sorted(labels)
    shape = (1, 16, 16, 16)
    pairs, means, stds = [], [], []
    for seed in range(3):
        ids = R.make_ids('iid', shape, order if seed else order[:3], (), seed)      # (label 12 is absent from the first pair)
        image = R.make_image(shape, 2, 'small', seed)
        want = R.stats(ids, image, order)
        with np.errstate(invalid='ignore', divide='ignore'):
            x64 = image.astype(np.float64)[0, ..., 1]
            means.append([x64[ids[0] == l].mean() if (ids[0] == l).any() else np.nan for l in order])
            stds.append([x64[ids[0] == l].std() if (ids[0] == l).any() else np.nan for l in order])
        assert (want['count'][0] > 0).tolist() == [True, True, True, seed > 0]
        pairs.append((torch.from_numpy(image[0]).to(dev), torch.from_numpy(ids[0]).to(dev)))
    got = ne.synthesis.intensity_priors(pairs, labels, channel=1)
    assert set(got) == {'mean_min', 'mean_max', 'std_min', 'std_max'} and all(isinstance(v, list) and len(v) == 4 for v in got.values())
    want = {'mean_min': np.nanmin(means, 0), 'mean_max': np.nanmax(means, 0), 'std_min': np.nanmin(stds, 0), 'std_max': np.nanmax(stds, 0)}
    for key, value in want.items():
        assert all(isinstance(v, float) for v in got[key])
        assert np.allclose(got[key], value, rtol=1e-12, atol=1e-15), key
    # a label that is absent everywhere gives None
    gap = ne.synthesis.intensity_priors(pairs[:1], labels + [99], channel=0)
    assert [v is None for v in gap['mean_min']] == [False, False, False, True, True] and gap['std_max'][3] is None
    # single-channel images without a channel axis
    flat = ne.synthesis.intensity_priors([(im[..., 0], ids) for im, ids in pairs], labels)
    assert flat['mean_min'] == ne.synthesis.intensity_priors(pairs, labels, channel=0)['mean_min']
    # labels_to_image takes the lists as they are
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter('ignore')
        model = ne.synthesis.labels_to_image((16, 16, 16), labels, warp_std=0, bias_std=0, blur_std=0, **got)
        image, out = model(pairs[1][1].view(1, 16, 16, 16, 1))[:2]
    assert image.shape == (1, 16, 16, 16, 1) and bool(torch.isfinite(image).all())
