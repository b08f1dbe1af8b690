"""
utils.percentile / quantile / median / percentile_norm and SynthStrip.brain_mask(normalize=True) (csrc/select.hip) on the GPU against the
definition of tests/percentile_restatement.py.  Every comparison is exact: `lower` / `higher` are order statistics, `linear` and
`midpoint` IEEE float64 expressions of them without contraction, the counts integers, and percentile_norm a float32 expression of the
kernel's own bounds.  Values are compared with equal NaN positions (the sign of a zero is not compared).

Shapes, the smallest at which each mechanism can fail: n = 1, 2, 3; 63 / 64 / 65 (one wave and its edge); 101 with q = 50 (pos an exact
integer); 4099 (a vector tail of 3); 3x37x41 = 4551; 41x43x41 = 72283 (nine blocks per entry, no power of two; with three entries
the second and third start at element indices that are no multiple of 4, so their blocks have vector heads as well as tails).  A view
one element into a buffer takes the kernels' unaligned arm, and 1100 entries of 37 elements the one-block-per-entry share of a launch
that has more entries than blocks.  Distributions: R.DISTRIBUTIONS and NaNs in both modes.
"""

import contextlib
import io

import numpy as np
import pytest
import torch

import percentile_restatement as R

pytestmark = pytest.mark.gpu

TORCH_DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float16': torch.float16}


def _ne():
    import neurite_amd as ne
    return ne


def _tensor(stored, dtype, dev):
    if dtype == 'bfloat16':
        return torch.from_numpy(np.ascontiguousarray(stored).view(np.int16)).to(dev).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(stored)).to(dev)


def _same(got, want):
    return np.array_equal(got, want, equal_nan=True)


def _check(ne, dev, rows, dtype='float32', masks=None, qs=R.Q8, methods=R.METHODS, nan_modes=(False,), what=''):
    """every output of nrt_percentile on the entries `rows` (a list of float32 arrays of one size) against the definition"""
    pairs = [R.store(np.asarray(r, np.float32).reshape(-1), dtype) for r in rows]
    x = _tensor(np.stack([p[0] for p in pairs]), dtype, dev)
    values = [p[1] for p in pairs]
    m = None if masks is None else torch.from_numpy(np.stack([np.asarray(k).reshape(-1) for k in masks])).to(dev)
    x2, m2 = ne.utils._pct_source(x, m, True, 'test')
    fractions = [float(q) / 100.0 for q in qs]
    for ignore_nan in nan_modes:
        for method in methods:
            out, lower, upper, count = [t.cpu().numpy() for t in ne.utils._select_call(x2, fractions, m2, method, ignore_nan)]
            assert out.dtype == np.float32 and out.shape == (len(rows), len(qs)) and count.dtype == np.int32
            for b, v in enumerate(values):
                want = R.percentile(v, qs, None if masks is None else masks[b], method, ignore_nan)
                tag = (what, dtype, v.size, b, method, ignore_nan)
                assert int(count[b]) == want[3], tag
                assert _same(lower[b], want[1]) and _same(upper[b], want[2]), tag + (lower[b], want[1], upper[b], want[2])
                assert _same(out[b], want[0]), tag + (out[b], want[0])


@pytest.mark.parametrize('n', R.SIZES)
def test_every_distribution_and_method(dev, n):
    ne = _ne()
    for name in R.DISTRIBUTIONS:
        _check(ne, dev, [R.draw(name, n, seed=4)], what=name)
    _check(ne, dev, [R.draw('nan', n, seed=4)], nan_modes=(False, True), what='nan')
    _check(ne, dev, [np.full(n, np.nan, np.float32)], nan_modes=(False, True), methods=('linear',), what='all nan')


@pytest.mark.parametrize('dtype', list(TORCH_DTYPES))
@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_volumes_batches_masks_and_dtypes(dev, shape, dtype):
    ne = _ne()
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    for names in (('normal', 'zeros70', 'ties'), ('last_pass', 'negative', 'inf'), ('one_bin', 'constant', 'denormal')):
        rows = [R.draw(name, n, seed=5) for name in names]
        _check(ne, dev, rows, dtype, methods=('linear', 'midpoint'), what=names)
        _check(ne, dev, rows[:1], dtype, methods=('lower',), what=names[0])
    rows = [R.draw(name, n, seed=6) for name in ('zeros70', 'nan', 'mixed_zeros')]
    one = np.zeros(n, bool)
    one[n // 3] = True
    masks = [rng.random(n) < 0.3, one, np.zeros(n, bool)]                           # random, exactly one element, empty
    _check(ne, dev, rows, dtype, masks, methods=('linear', 'higher'), nan_modes=(False, True), what='masks')
    masks = [rng.random(n) < 0.3, rng.random(n) < 0.3, rng.random(n) < 0.9]
    _check(ne, dev, rows, dtype, masks, methods=('linear',), nan_modes=(False, True), what='masks per entry')
    _check(ne, dev, rows, dtype, [k.astype(np.uint8) * 7 for k in masks], methods=('midpoint',), what='uint8 masks')


def test_public_functions(dev):
    ne = _ne()
    u = ne.utils
    v = R.draw('zeros70', 4551, seed=7).reshape(3, 37, 41)
    x = torch.from_numpy(v).to(dev)
    for q in R.QS:
        got = u.percentile(x, q)
        assert got.shape == () and got.dtype == torch.float32 and not got.requires_grad
        assert _same(got.cpu().numpy(), R.percentile(v, [q])[0][0]), q
        f = q / 100.0
        if 100.0 * f / 100.0 == f:
            assert torch.equal(u.quantile(x, f), u.percentile(x, 100.0 * f)), q
        assert _same(u.quantile(x, f).cpu().numpy(), R.from_sorted(R.population(v), f)[0]), q
    got = u.percentile(x, list(R.Q8), batched=True, method='higher')
    assert got.shape == (3, 8)
    for b in range(3):
        assert _same(got[b].cpu().numpy(), R.percentile(v[b], R.Q8, method='higher')[0])
    assert torch.equal(got[:, 2], got[:, 7])                                         # the duplicate in the list
    assert torch.equal(u.median(x), u.percentile(x, 50)) and torch.equal(u.median(x, batched=True), u.percentile(x, 50, batched=True))
    assert u.percentile(x, [50]).shape == (1,) and u.percentile(x, 50, batched=True).shape == (3,)
    odd = torch.arange(101, dtype=torch.float32, device=dev)
    assert float(u.median(odd)) == 50.0 and float(u.percentile(odd.flip(0), 50, method='lower')) == 50.0
    mask = torch.from_numpy(np.random.default_rng(1).random(v.shape) < 0.3).to(dev)
    assert _same(u.median(x, mask=mask).cpu().numpy(), R.percentile(v, [50], mask.cpu().numpy())[0][0])
    grad = x.clone().requires_grad_(True)
    assert not u.percentile(grad, 50).requires_grad and not u.percentile_norm(grad).requires_grad
    # a view that starts one element into its buffer: no 16-byte alignment
    buf = torch.from_numpy(R.draw('normal', 4100, seed=8)).to(dev)
    assert _same(u.percentile(buf[1:], [0.5, 50, 99.5]).cpu().numpy(), R.percentile(buf[1:].cpu().numpy(), [0.5, 50, 99.5])[0])
    half = buf.to(torch.float16)
    assert _same(u.percentile(half[1:], [0.5, 50, 99.5]).cpu().numpy(),
                 R.percentile(half[1:].float().cpu().numpy(), [0.5, 50, 99.5])[0])


def test_many_entries(dev):
    """more entries than the launch has blocks to share out: one block per entry, and an entry of 37 elements is all head and tail"""
    ne = _ne()
    v = R.draw('normal', 1100 * 37, seed=12).reshape(1100, 37)
    v[5] = 0
    v[7, 3] = np.nan
    x = torch.from_numpy(v).to(dev)
    got = ne.utils.percentile(x, [0, 33.3, 100], batched=True).cpu().numpy()
    want = np.stack([R.percentile(v[b], [0, 33.3, 100])[0] for b in range(1100)])
    assert got.shape == (1100, 3) and _same(got, want)
    normed = ne.utils.percentile_norm(x, 0, 100, batched=True, clip=False).cpu().numpy()
    assert _same(normed, np.stack([R.rescale_clip(v[b], want[b, 0], want[b, 2], clip=False) for b in range(1100)]))


def _norm_want(u, x, lower, upper, mask=None, **kw):
    """the NumPy float32 expression on the kernel's own bounds, entry by entry of x [B, ...]"""
    bounds = u.percentile(x, [lower, upper], mask=mask, batched=True).cpu().numpy()
    xs = x.float().cpu().numpy()
    return np.stack([R.rescale_clip(xs[b], bounds[b, 0], bounds[b, 1], **kw) for b in range(xs.shape[0])])


@pytest.mark.parametrize('dtype', list(TORCH_DTYPES))
def test_percentile_norm(dev, dtype):
    ne = _ne()
    u = ne.utils
    shape = (3, 37, 41)
    rows = [R.draw(name, 4551, seed=9) for name in ('zeros70', 'normal', 'constant', 'nan')]
    x = _tensor(np.stack([R.store(r, dtype)[0] for r in rows]).reshape((4,) + shape), dtype, dev)
    for lower, upper in ((0, 99), (0.5, 99.5), (0, 100)):
        for kw in ({}, {'clip': False}, {'out_range': (-1, 1)}, {'clip': False, 'out_range': (0, 255)}):
            got = u.percentile_norm(x, lower, upper, batched=True, **kw)
            assert got.dtype == torch.float32 and got.shape == x.shape
            want = _norm_want(u, x, lower, upper, **kw)
            assert _same(got.cpu().numpy(), want), (dtype, lower, upper, kw)
            assert not got[2].any() if kw.get('out_range', (0, 1))[0] == 0 else bool((got[2] == -1).all())          # hi == lo
            assert bool(got[3].isnan().all()) and not bool(got[:2].isnan().any())                                    # NaN bounds
            if not kw:
                assert float(got[:2].min()) == 0.0 and float(got[:2].max()) == 1.0
    # the mask restricts where the bounds are measured, not where the output is written
    mask = torch.from_numpy(np.random.default_rng(2).random(tuple(x.shape)) < 0.3).to(dev)
    got = u.percentile_norm(x, 1, 90, mask=mask, batched=True)
    assert _same(got.cpu().numpy(), _norm_want(u, x, 1, 90, mask=mask))
    single = u.percentile_norm(x[0], 0.5, 99.5)
    assert single.shape == shape and torch.equal(single, u.percentile_norm(x[:1], 0.5, 99.5, batched=True)[0])
    flat = x[1].reshape(-1)[1:4100]                                                  # unaligned, with a tail
    assert _same(u.percentile_norm(flat).cpu().numpy(), _norm_want(u, flat[None], 0, 99)[0])


def test_two_runs_are_identical(dev):
    ne = _ne()
    x = torch.from_numpy(np.stack([R.draw(name, 72283, seed=10) for name in ('zeros70', 'normal', 'ties')])).to(dev)
    a, b = [ne.utils.percentile(x, list(R.Q8), batched=True) for _ in range(2)]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = [ne.utils.percentile_norm(x, 0.5, 99.5, batched=True) for _ in range(2)]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_percentile_norm_captures_into_a_graph(dev):
    """one percentile_norm call captured once and replayed on new data"""
    ne = _ne()
    inputs = [torch.from_numpy(R.draw(name, 2 * 4551, seed=11).reshape(2, 3, 37, 41)).to(dev) for name in ('zeros70', 'normal')]
    eager = [ne.utils.percentile_norm(x, 0.5, 99.5, batched=True) for x in inputs]
    static = inputs[0].clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ne.utils.percentile_norm(static, 0.5, 99.5, batched=True)                   # (warm-up: workspaces and the device are set up)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ne.utils.percentile_norm(static, 0.5, 99.5, batched=True)
    for x, want in zip(inputs[::-1], eager[::-1]):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want)


def test_synthstrip_brain_mask_normalize(dev):
    ne = _ne()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ne.models.SynthStrip((16, 16, 16), [0, 1, 2, 3], {1: 1, 2: 1, 3: 1}, nb_unet_features=4, nb_unet_levels=2)
    model = model.to(dev)
    image = torch.rand((2, 16, 16, 16, 1), device=dev) * 900.0 + 30.0
    normed = ne.utils.percentile_norm(image, 0, 99, batched=True)
    with torch.no_grad():
        border = float(model.get_strip_model()(normed)[..., 0].median())            # (an untrained net: a border that splits its output)
    got = model.brain_mask(image, border=border, normalize=True)
    assert got.dtype == torch.bool and got.shape == (2, 16, 16, 16) and 0 < int(got.sum()) < got.numel()
    assert torch.equal(got, model.brain_mask(normed, border=border))
    assert torch.equal(got, model.brain_mask(image[..., 0], border=border, normalize=True))
    assert torch.equal(model.brain_mask(image, border=border, normalize=False), model.brain_mask(image, border=border))
