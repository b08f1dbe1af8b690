"""
GPU tests of neurite_amd.seg on the kernels of csrc/seg.hip.

1. arg-max: bit-exact labels against the reference's recorded pred_to_label (tests/golden/seg_small.npz) and against np.argmax where the
   fixture has no case: every channel count that takes another arm or group width, voxel counts around the block and wave sizes, ties,
   NaNs, float32 / bfloat16 inputs, int32 / int64 outputs.
2. the fused probability: within (C + 2) 2^-24 relative of float64 on the same non-negative inputs (C - 1 additions and one division
   of positive terms, each within 2^-24 relative, in any order; tests/test_seg_abi.py holds the reference's recorded outputs to the same
   bound); a label outside the row gives NaN and leaves its neighbours alone.
3. recode: bit-exact against the recorded outputs.
4. extract / quilt against the NumPy restatement (tests/seg_restatement.py): exact copies, exact round trips, the median bit for bit
   against np.nanmedian, the mean within (k + 1) 2^-24 sum|v_i| / k of float64 (k - 1 float32 additions and one division).
5. predict_volume / predict_volumes / predict_volume_stack end to end, and arg-max + quilt captured into a graph.
"""

import os
import sys

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import seg_restatement as rs                                  # noqa: E402
from conftest import bits_equal, golden_cases, load_golden    # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = golden_cases(load_golden('seg_small'))
CHANNELS = [1, 2, 3, 4, 5, 8, 20, 32, 33, 64, 100, 256]
NVOX = [1, 63, 65, 4099]
ARMS = CHANNELS + [140, 252]                # bfloat16 rows of 8-byte pieces, more than 32 of them: four per lane
U = 2.0 ** -24
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
AM_TAGS = sorted(t for t in GOLD if t.startswith('am_'))
PL_TAGS = sorted(t for t in GOLD if t.startswith('pl_'))
RC_TAGS = sorted(t for t in GOLD if t.startswith('rc_'))


def _stored(x, storage, dev):
    """x on the device as `storage`, and the float32 values that storage holds"""
    t = torch.tensor(np.asarray(x, np.float32)).to(dev).to(TORCH[storage])
    return t, t.to(torch.float32).cpu().numpy()


def _labels(pred, dtype):
    out = torch.empty(pred.shape[:-1], dtype=dtype, device=pred.device)
    seg._argmax(pred, labels=out)
    return out


# ---- 1. arg-max -----------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases_the_tests_name():
    assert len(AM_TAGS) >= 20 and len(PL_TAGS) >= 10 and len(RC_TAGS) == 4
    assert {'am_tie_c%d' % C for C in CHANNELS} <= set(AM_TAGS)
    assert GOLD['am_bf_nd_c5']['x'].shape == (2, 5, 6, 7, 5)


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
@pytest.mark.parametrize('tag', AM_TAGS)
def test_argmax_equals_the_recorded_reference(dev, tag, storage):
    case = GOLD[tag]
    x, held = _stored(case['x'], storage, dev)
    if bits_equal(held, np.asarray(case['x'], np.float32)):
        want = case['label']                                   # the storage holds the recorded input exactly
    else:
        want = np.argmax(held, -1)                             # bfloat16 rounds it: np.argmax of what is stored
    if storage == 'f32':
        assert np.array_equal(want, case['label'])
    got64, = ne.seg.pred_to_label(x)
    assert got64.dtype == torch.int64 and tuple(got64.shape) == want.shape
    assert np.array_equal(got64.cpu().numpy(), want)
    got32 = _labels(x, torch.int32)
    assert np.array_equal(got32.cpu().numpy(), want.astype(np.int32))


@pytest.mark.parametrize('C', ARMS)
def test_argmax_shapes_ties_and_the_last_element(dev, C):
    rng = np.random.default_rng(1000 + C)
    for n in NVOX:
        for storage in ('f32', 'bf16'):
            x = rng.integers(0, 4, size=(n, C)).astype(np.float32)             # most voxels are ties
            x[-1, :] = 1.0
            x[-1, C - 1] = 5.0 if C > 1 else 1.0                               # the maximum in the last channel of the last voxel
            t, held = _stored(x, storage, dev)
            want = np.argmax(held, -1)
            assert want[-1] == C - 1
            for dtype in (torch.int32, torch.int64):
                assert np.array_equal(_labels(t, dtype).cpu().numpy(), want), (n, storage, dtype)
            y = rng.standard_normal((n, C)).astype(np.float32)
            t, held = _stored(y, storage, dev)
            assert np.array_equal(ne.seg.pred_to_label(t)[0].cpu().numpy(), np.argmax(held, -1)), (n, storage)


def test_argmax_nan_positions_and_signed_zero(dev):
    for C in (4, 5, 32, 100):
        x = np.random.default_rng(C).standard_normal((70, C)).astype(np.float32)
        x[0:10, 0] = np.nan
        x[10:20, C // 2] = np.nan
        x[20:30, C - 1] = np.nan
        x[30:40, 1:] = np.nan
        x[40:50, :] = -0.0
        x[40:50, C - 1] = 0.0                                                  # -0 == +0: the first index wins
        for storage in ('f32', 'bf16'):
            t, held = _stored(x, storage, dev)
            want = np.argmax(held, -1)
            assert list(want[0:30:10]) == [0, C // 2, C - 1] and want[35] == 1 and want[45] == 0
            assert np.array_equal(ne.seg.pred_to_label(t)[0].cpu().numpy(), want), (C, storage)


def test_unaligned_and_other_dtype_inputs(dev):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((67, 8)).astype(np.float32)
    flat = torch.zeros(67 * 8 + 1, device=dev)
    flat[1:] = torch.tensor(x).to(dev).reshape(-1)
    view = flat[1:].view(67, 8)                                                # 4-byte aligned only: the per-voxel arm
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(ne.seg.pred_to_label(view)[0].cpu().numpy(), np.argmax(x, -1))
    assert np.array_equal(ne.seg.pred_to_label(torch.tensor(x).to(dev).double())[0].cpu().numpy(), np.argmax(x, -1))
    strided = torch.tensor(x).to(dev).t().contiguous().t()                     # not contiguous
    assert np.array_equal(ne.seg.pred_to_label(strided)[0].cpu().numpy(), np.argmax(x, -1))


# ---- 2. the fused probability ---------------------------------------------------------------------------------------------------------
def _prob_want(held, lab):
    h = held.astype(np.float64)
    return np.take_along_axis(h, lab[..., None].astype(np.int64), -1)[..., 0] / h.sum(-1)


def _within(got, want, C):
    got = got.astype(np.float64)
    return bool(np.all(np.abs(got - want) <= (C + 2) * U * np.abs(want)))


@pytest.mark.parametrize('tag', PL_TAGS)
def test_prob_of_label_on_the_recorded_cases(dev, tag):
    case = GOLD[tag]
    C = case['x'].shape[-1]
    for storage in (('f32', 'bf16') if tag.startswith('pl_bf') else ('f32',)):
        x, held = _stored(case['x'], storage, dev)
        assert bits_equal(held, case['x'])
        want = _prob_want(held, case['label'])
        assert _within(case['prob'], want, C)                                  # the reference itself
        for dtype in (torch.int32, torch.int64):
            got = ne.seg.prob_of_label(x, torch.tensor(case['label']).to(dev).to(dtype))
            assert got.dtype == torch.float32 and tuple(got.shape) == case['label'].shape
            assert _within(got.cpu().numpy(), want, C), (storage, dtype)


@pytest.mark.parametrize('C', ARMS)
def test_fused_probability_within_the_bound(dev, C):
    rng = np.random.default_rng(2000 + C)
    for n in NVOX:
        for storage in ('f32', 'bf16'):
            x = rng.random((n, C), dtype=np.float32) + np.float32(0.01)
            t, held = _stored(x, storage, dev)
            lab = rng.integers(0, C, size=n)
            lab[-1] = C - 1
            of = torch.tensor(lab).to(dev).to(torch.int32 if n % 2 else torch.int64)
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            prob = torch.empty(n, dtype=torch.float32, device=dev)
            seg._argmax(t, labels=labels, of=of, prob=prob)                    # both in one pass
            assert np.array_equal(labels.cpu().numpy(), np.argmax(held, -1))
            assert _within(prob.cpu().numpy(), _prob_want(held, lab), C), (n, storage)
            seg._argmax(t, labels=labels, prob=prob)                           # the probability of the arg-max itself
            assert _within(prob.cpu().numpy(), _prob_want(held, np.argmax(held, -1)), C), (n, storage)
            seg._argmax(t, prob=prob)                                          # no labels wanted
            assert _within(prob.cpu().numpy(), _prob_want(held, np.argmax(held, -1)), C), (n, storage)


@pytest.mark.parametrize('C', [1, 3, 4, 20, 32, 100, 252, 256])
def test_label_outside_the_row_gives_nan_and_spares_its_neighbours(dev, C):
    rng = np.random.default_rng(C)
    n = 130
    x = rng.random((n, C), dtype=np.float32) + np.float32(0.01)
    lab = rng.integers(0, C, size=n)
    bad = {0: -1, 64: C, 65: -1, 129: C, 77: 1 << 40, 78: -(1 << 40)}
    for storage in ('f32', 'bf16'):
        t, held = _stored(x, storage, dev)
        for dtype in (torch.int32, torch.int64):
            l2 = lab.copy()
            for i, v in bad.items():
                if dtype == torch.int64 or abs(v) < (1 << 31):
                    l2[i] = v
            wrong = (l2 < 0) | (l2 >= C)
            prob = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
            seg._argmax(t, of=torch.tensor(l2).to(dev).to(dtype), prob=prob)
            got = prob.cpu().numpy()
            assert np.all(np.isnan(got[wrong])) and wrong.sum() >= 4
            assert _within(got[~wrong], _prob_want(held[~wrong], l2[~wrong]), C), (storage, dtype)
            with pytest.raises(IndexError):
                ne.seg.prob_of_label(t, torch.tensor(l2).to(dev).to(dtype))
    for v in (-1, C):
        l2 = lab.copy()
        l2[5] = v
        with pytest.raises(IndexError):
            ne.seg.prob_of_label(t, torch.tensor(l2).to(dev))


# ---- 3. recode ------------------------------------------------------------------------------------------------------------------------
def _mapping(case):
    if int(case['is_list']):
        return [int(k) for k in case['keys']]
    return {int(k): int(v) for k, v in zip(case['keys'], case['values'])}


@pytest.mark.parametrize('tag', RC_TAGS)
def test_recode_equals_the_recorded_reference(dev, tag):
    case = GOLD[tag]
    max_label = int(case['max_label']) if 'max_label' in case else None
    for dtype in (torch.int32, torch.int64):
        got = ne.seg.recode(torch.tensor(case['seg']).to(dev).to(dtype), _mapping(case), max_label)
        assert got.dtype == torch.float32
        assert bits_equal(got.cpu().numpy(), case['out']), dtype

    class Table:
        mapping = _mapping(case)
    if not int(case['is_list']):
        got = ne.seg.recode(torch.tensor(case['seg']).to(dev), Table(), max_label)
        assert bits_equal(got.cpu().numpy(), case['out'])


def test_recode_out_of_range_gives_zero(dev):
    s = np.array([[0, 1, 2, 3, 4, 5, -1, 1000, 2, -7]] * 30, np.int64)           # the lookup has 4 entries
    s[3, 3] = 1 << 40
    for dtype in (torch.int32, torch.int64):
        sv = s if dtype == torch.int64 else np.where(np.abs(s) < (1 << 31), s, 9)
        got = ne.seg.recode(torch.tensor(sv).to(dev).to(dtype), {1: 5, 3: 2}).cpu().numpy()
        want = np.where(sv == 1, 5.0, np.where(sv == 3, 2.0, 0.0)).astype(np.float32)
        assert bits_equal(got, want), dtype
    got = ne.seg.recode(torch.tensor(s).to(dev), [1, 0], max_label=5).cpu().numpy()   # the list form: label l -> its place + 1
    assert bits_equal(got, np.where(s == 1, 1.0, np.where(s == 0, 2.0, 0.0)).astype(np.float32))


# ---- 4. extract and quilt -------------------------------------------------------------------------------------------------------------
# (vol_shape, patch, stride): the grid is every patch that fits, and it tiles the volume exactly
GRIDS = {
    'r1_cover1to3': ((11,), (5,), (2,)),
    'r1_stride_eq_patch': ((12,), (4,), (4,)),
    'r2': ((12, 9), (4, 5), (4, 2)),
    'r2_one_patch': ((5, 6), (5, 6), (1, 1)),
    'r3_stride_eq_patch': ((8, 8, 8), (4, 4, 4), (4, 4, 4)),
    'r3_cover1to3': ((9, 7, 6), (5, 5, 4), (2, 2, 2)),
    'r3_64_covers': ((7, 7, 8), (4, 4, 4), (1, 1, 1)),
    'r3_one_patch': ((5, 6, 7), (5, 6, 7), (2, 2, 2)),
    'r3_12_8_4': ((12, 12, 12), (8, 8, 8), (4, 4, 4)),
}
PATCH_CHANNELS = [1, 3, 4, 32]


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_extract_equals_the_restatement(dev, name):
    shape, patch, stride = GRIDS[name]
    grid = rs.grid_of(shape, patch, stride)
    N = int(np.prod(grid))
    rng = np.random.default_rng(len(name))
    for C in PATCH_CHANNELS:
        v = rng.standard_normal(shape + (C,)).astype(np.float32)
        want = rs.extract(v, patch, stride)
        for storage in ('f32', 'bf16'):
            t, held = _stored(v, storage, dev)
            got = ne.seg.extract_patches(t, patch, stride)
            assert got.dtype == t.dtype and tuple(got.shape) == want.shape
            assert bits_equal(got.float().cpu().numpy(), rs.extract(held, patch, stride)), (C, storage)
        t = torch.tensor(v).to(dev)
        for start, count in ((0, 1), (N - 1, 1), (N // 2, N - N // 2), (max(N - 3, 0), None)):       # the ranges end on the last patch
            got = ne.seg.extract_patches(t, patch, stride, grid, start, count)
            assert bits_equal(got.cpu().numpy(), want[start:] if count is None else want[start:start + count]), (C, start, count)
    # a smaller grid than fits, and an unaligned volume
    if N > 1:
        sub = tuple(max(g - 1, 1) for g in grid)
        flat = torch.zeros(v.size + 1, device=dev)
        flat[1:] = torch.tensor(v).to(dev).reshape(-1)
        got = ne.seg.extract_patches(flat[1:].view(v.shape), patch, stride, sub)
        assert bits_equal(got.cpu().numpy(), rs.extract(v, patch, stride, sub))


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_quilt_inverts_extract_bit_for_bit(dev, name):
    shape, patch, stride = GRIDS[name]
    grid = rs.grid_of(shape, patch, stride)
    rng = np.random.default_rng(10 + len(name))
    for C in PATCH_CHANNELS:
        vi = rng.integers(0, 1000, size=shape + (C,)).astype(np.float32)
        vf = (rng.standard_normal(shape + (C,)) * 100).astype(np.float32)
        for v, funcs in ((vi, (np.nanmean, np.nanmedian, 'mean', 'median')), (vf, (np.nanmedian,))):
            p = ne.seg.extract_patches(torch.tensor(v).to(dev), patch, stride)
            for f in funcs:
                got = ne.seg.quilt(p, patch, grid, stride, nan_func=f)
                assert got.dtype == torch.float32 and tuple(got.shape) == v.shape
                assert bits_equal(got.cpu().numpy(), v), (C, f)
        # integer patches are converted
        p = ne.seg.extract_patches(torch.tensor(vi).to(dev), patch, stride).to(torch.int32)
        for f in ('mean', 'median'):
            assert bits_equal(ne.seg.quilt(p, patch, grid, stride, nan_func=f).cpu().numpy(), vi), (C, f)
        if C == 1:
            for q in (p[..., 0], p.reshape(p.shape[0], -1), p.to(torch.int64)[..., 0]):                # single-channel forms
                got = ne.seg.quilt(q, patch, grid, stride, nan_func='median')
                assert bits_equal(got.cpu().numpy(), vi[..., 0])
            got = ne.seg._quilt(p.reshape(p.shape[0], -1), patch, grid, stride, nan_func_layers=np.nanmedian, nan_func_K=np.nanmedian)
            assert bits_equal(got.cpu().numpy(), vi[..., 0])


# stride > patch leaves NaN gaps: (patch, stride, grid)
GAPS = {'r1_gap': ((2,), (3,), (3,)), 'r2_gap': ((2, 3), (3, 3), (3, 2)), 'r3_gap': ((2, 2, 3), (3, 2, 4), (2, 3, 2)),
        'r3_gap_overlap': ((3, 2, 2), (2, 5, 1), (3, 2, 4))}


def _quilt_cases():
    out = []
    for name in sorted(GRIDS):
        shape, patch, stride = GRIDS[name]
        out.append((name, patch, stride, rs.grid_of(shape, patch, stride)))
    for name in sorted(GAPS):
        out.append((name,) + GAPS[name])
    return out


@pytest.mark.parametrize('name,patch,stride,grid', _quilt_cases(), ids=[c[0] for c in _quilt_cases()])
def test_quilt_of_independent_patches_against_the_restatement(dev, name, patch, stride, grid):
    """patches that disagree where they overlap, with NaN values inside them: odd and even counts, partly and wholly NaN elements"""
    N = int(np.prod(grid))
    rng = np.random.default_rng(20 + len(name))
    for C in PATCH_CHANNELS:
        p = (rng.random((N,) + patch + (C,), dtype=np.float32) * 2000 - 1000).astype(np.float32)         # |v| < 10^3
        p[rng.random(p.shape) < 0.15] = np.nan
        p.reshape(N, -1)[:, 0] = np.nan                                        # the first element of every patch
        t = torch.tensor(p).to(dev)
        stack = rs.layers(p, patch, grid, stride)
        k = np.sum(~np.isnan(stack), axis=0)
        if name in GAPS:
            assert (k == 0).any()
        elif N > 1 and 'stride_eq_patch' not in name:
            assert k.max() >= 2
        if name == 'r3_64_covers':
            assert np.sum(~np.isnan(rs.layers(np.ones_like(p), patch, grid, stride)), axis=0).max() == 64

        got = ne.seg.quilt(t, patch, grid, stride, nan_func=np.nanmedian).cpu().numpy()
        want = rs.quilt(p, patch, grid, stride, np.nanmedian)
        assert want.dtype == np.float32 and np.array_equal(np.isnan(want), k == 0)
        assert bits_equal(got, want), (C, 'median')

        got = ne.seg.quilt(t, patch, grid, stride, nan_func=np.nanmean).cpu().numpy()
        again = ne.seg.quilt(t, patch, grid, stride, nan_func='mean').cpu().numpy()
        assert bits_equal(got, again)                                          # run to run
        want = rs.quilt(p.astype(np.float64), patch, grid, stride, np.nanmean)
        assert np.array_equal(np.isnan(got), k == 0)
        bound = (k + 1) * U * np.nansum(np.abs(stack.astype(np.float64)), axis=0) / np.maximum(k, 1)
        live = k > 0
        assert np.all(np.abs(got.astype(np.float64) - want)[live] <= bound[live]), (C, 'mean')


def test_quilt_and_predict_volume_refusals(dev):
    with pytest.raises(NotImplementedError, match='64'):
        ne.seg.quilt(torch.zeros(2, 65, device=dev), (65,), (2,), (1,), nan_func='median')
    assert tuple(ne.seg.quilt(torch.zeros(2, 65, device=dev), (65,), (2,), (1,), nan_func='mean').shape) == (66,)
    with pytest.raises(ValueError):
        ne.seg.quilt(torch.zeros(3, 4, device=dev), (4,), (2,), (1,))
    with pytest.raises(ValueError, match='tile'):
        ne.seg.predict_volume(lambda p: p, torch.zeros(13, 12, 12, 1, device=dev), (8, 8, 8), (4, 4, 4))
    with pytest.raises(ValueError):
        ne.seg.extract_patches(torch.zeros(12, 12, 1, device=dev), (8, 8), (4, 4), (2, 3))


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
VOL, PATCH, STRIDE, NB_LABELS = (12, 12, 12), (8, 8, 8), (4, 4, 4), 4
GRID = rs.grid_of(VOL, PATCH, STRIDE)


def _scan():
    return np.random.default_rng(41).integers(0, NB_LABELS, size=VOL + (1,)).astype(np.float32)


def _toy_labels_np(p):
    """the label a patch voxel gets depends on the patch: overlapping patches disagree"""
    return ((p[..., 0] + p[:, :1, :1, :1, 0]) % NB_LABELS).astype(np.int64)


def _toy_model(p):
    lab = ((p[..., 0] + p[:, :1, :1, :1, 0]) % NB_LABELS).long()
    return torch.nn.functional.one_hot(lab, NB_LABELS).to(torch.float32) * 0.75 + 0.125


@pytest.mark.parametrize('batch_size', [1, 4, 5])
def test_predict_volume_with_a_known_model(dev, batch_size):
    v = _scan()
    patches = rs.extract(v, PATCH, STRIDE)
    lab = _toy_labels_np(patches)[..., None]
    for f in (np.nanmedian, np.nanmean):
        want = rs.quilt(lab, PATCH, GRID, STRIDE, f)[..., 0]
        got = ne.seg.predict_volume(_toy_model, torch.tensor(v).to(dev), PATCH, STRIDE, batch_size=batch_size, nan_func=f)
        assert got.dtype == torch.int64 and tuple(got.shape) == VOL
        if f is np.nanmedian:
            assert np.array_equal(got.cpu().numpy(), want.astype('int'))
            assert (want != np.floor(want)).any() and (want.astype('int') != v[..., 0]).any()
        else:                                                                  # a mean within its rounding of an integer may truncate either way
            w64 = rs.quilt(lab.astype(np.float64), PATCH, GRID, STRIDE, f)[..., 0]
            clear = np.abs(w64 - np.round(w64)) > 1e-4
            assert np.array_equal(got.cpu().numpy()[clear], w64.astype('int')[clear])
    got, prob = ne.seg.predict_volume(_toy_model, torch.tensor(v).to(dev), PATCH, STRIDE, batch_size=batch_size, return_prob=True)
    assert np.array_equal(got.cpu().numpy(), rs.quilt(lab, PATCH, GRID, STRIDE, np.nanmedian)[..., 0].astype('int'))
    assert prob.dtype == torch.float32 and tuple(prob.shape) == VOL
    assert _within(prob.cpu().numpy(), np.full(VOL, 0.875 / 1.25), NB_LABELS)      # (0.75 + 0.125) / (0.75 + 4 * 0.125) everywhere


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
def test_predict_volume_with_a_unet(dev, storage):
    torch.manual_seed(7)
    net = ne.models.unet(4, PATCH + (1,), 2, 3, 3).to(dev)
    if storage == 'bf16':
        net = net.to(torch.bfloat16)
    v = np.random.default_rng(43).standard_normal(VOL + (1,)).astype(np.float32)
    patches = rs.extract(v, PATCH, STRIDE)

    def labels_in_batches(b):
        labs = []
        with torch.no_grad():
            for n in range(0, patches.shape[0], b):
                out = net(torch.tensor(patches[n:n + b]).to(dev))
                assert out.dtype == TORCH[storage] and tuple(out.shape[1:]) == PATCH + (3,)
                labs.append(torch.argmax(out.float(), -1).cpu().numpy())
        return np.concatenate(labs)[..., None]

    one_by_one = labels_in_batches(1)                                          # patch by patch
    for batch_size in (1, 4):
        got = ne.seg.predict_volume(net, torch.tensor(v).to(dev), PATCH, STRIDE, batch_size=batch_size)
        # float32: against the network applied patch by patch.  A bfloat16 batch may take another kernel arm than a single patch and
        # round differently, so a bfloat16 run is held to the network applied to the same batches.
        lab = one_by_one if storage == 'f32' else labels_in_batches(batch_size)
        want = rs.quilt(lab, PATCH, GRID, STRIDE, np.nanmedian)[..., 0].astype('int')
        assert np.array_equal(got.cpu().numpy(), want), batch_size
    assert len(np.unique(one_by_one)) > 1
    assert not net.training


def _generator(dev, batch_size, with_prior):
    """(inputs, y_true) batches over the patches of a scan, the last one padded by repeating its last patch"""
    v = _scan()
    truth = np.random.default_rng(44).integers(0, NB_LABELS, size=VOL)
    onehot = np.eye(NB_LABELS, dtype=np.float32)[truth]
    prior = np.random.default_rng(45).random(VOL + (NB_LABELS,), dtype=np.float32) + np.float32(0.05)
    pv, pt, pp = (rs.extract(a, PATCH, STRIDE) for a in (v, onehot, prior))
    N = pv.shape[0]

    def gen():
        for s in range(0, N, batch_size):
            idx = np.minimum(np.arange(s, s + batch_size), N - 1)
            x = torch.tensor(pv[idx]).to(dev)
            yield ([x, torch.tensor(pp[idx]).to(dev)] if with_prior else x), torch.tensor(pt[idx]).to(dev)
    return gen(), (v, truth, prior, pv, pt, pp)


def _model_a(inputs):
    x = inputs[0] if isinstance(inputs, (list, tuple)) else inputs
    return _toy_model(x) + 0.01 * x                                            # keeps the arg-max, changes the probabilities


def _model_b(inputs):
    x = inputs[0] if isinstance(inputs, (list, tuple)) else inputs
    lab = ((2 * x[..., 0] + x[:, -1:, -1:, -1:, 0]) % NB_LABELS).long()
    return torch.nn.functional.one_hot(lab, NB_LABELS).to(torch.float32) * 0.5 + 0.25


class _Predictor:
    def predict(self, inputs):
        return _model_b(inputs)


def _expected(model, data, with_prior, do_extra_vol, do_prob_of_true, nan_func, dev):
    """[(is a label volume, float64 volume)]: label votes come back before their truncation"""
    v, truth, prior, pv, pt, pp = data
    with torch.no_grad():
        pred = model(torch.tensor(pv).to(dev)).cpu().numpy()
    q = lambda a, f: rs.quilt(a.astype(np.float64), PATCH, GRID, STRIDE, f)[..., 0]              # noqa: E731
    true_lab = np.argmax(pt, -1)
    out = [(True, q(true_lab[..., None], nan_func)), (True, q(np.argmax(pred, -1)[..., None], nan_func))]
    if do_extra_vol:
        out.append((False, q(pv, np.nanmean)))
        if with_prior:
            out.append((True, q(np.argmax(pp, -1)[..., None], nan_func)))
    if do_extra_vol and do_prob_of_true:
        out.append((False, q(_prob_want(pred, true_lab)[..., None], nan_func)))
        if with_prior:
            out.append((False, q(_prob_want(pp, true_lab)[..., None], nan_func)))
    return out


@pytest.mark.parametrize('with_prior', [False, True], ids=['plain', 'prior'])
@pytest.mark.parametrize('batch_size', [2, 3])
def test_predict_volumes_generator_form(dev, batch_size, with_prior):
    for models, extra, prob, f in ((_model_a, False, False, np.nanmedian), (_model_a, True, True, np.nanmedian),
                                   ([_model_a, _Predictor()], True, True, np.nanmedian), ((_model_a,), True, False, np.nanmean),
                                   ([_model_a, _Predictor()], True, True, np.nanmean), (_model_a, False, True, np.nanmedian)):
        gen, data = _generator(dev, batch_size, with_prior)
        got = ne.seg.predict_volumes(models, gen, batch_size, PATCH, STRIDE, GRID, nan_func=f, do_extra_vol=extra, do_prob_of_true=prob)
        many = isinstance(models, list) and len(models) > 1
        assert isinstance(got, tuple) and (len(got) == 2 if many else True)
        fns = [_model_a, _model_b] if many else [_model_a]
        for entry, fn in zip(got if many else (got,), fns):
            want = _expected(fn, data, with_prior, extra, prob, f, dev)
            assert len(entry) == len(want) == 2 + (1 + with_prior) * extra + (1 + with_prior) * (extra and prob)
            assert np.array_equal(entry[0].cpu().numpy(), data[1])             # the truth comes back: every patch agrees on it
            for g, (is_label, w) in zip(entry, want):
                assert tuple(g.shape) == VOL
                if is_label:
                    assert g.dtype == torch.int64
                    # a median of integers is an integer or a half, exact in float32.  A mean is compared where its float64 value is
                    # an integer (the float32 sum and division are then exact) or clear of one (a mean within its rounding of an
                    # integer may truncate either way); with at most 8 covers that is every voxel.
                    ok = (w == np.round(w)) | (np.abs(w - np.round(w)) > 1e-4)
                    assert ok.mean() > 0.99 and (f is np.nanmean or ok.all())
                    assert np.array_equal(g.cpu().numpy()[ok], w.astype('int')[ok])
                else:
                    assert g.dtype == torch.float32
                    # each probability is within (C + 2) u; a median adds at most one rounding (the half-sum of two), a float32 mean
                    # of k <= 8 positive values k - 1 additions and a division
                    np.testing.assert_allclose(g.cpu().numpy(), w, rtol=(NB_LABELS + (3 if f is np.nanmedian else 2 + 8)) * U, atol=0)
        if f is np.nanmean:                                                    # the mean vote is not the median vote: both are told apart
            assert (want[1][1] != np.round(want[1][1])).any()


def test_predict_volume_stack_keeps_the_reference_contract(dev):
    for with_prior in (False, True):
        gen, data = _generator(dev, 3, with_prior)
        v, truth, prior, pv, pt, pp = data
        got = ne.seg.predict_volume_stack(_model_a, gen, 3, GRID)
        assert len(got) == 3 + with_prior
        N, nb_vox = pv.shape[0], int(np.prod(PATCH))
        with torch.no_grad():
            pred = _model_a(torch.tensor(pv).to(dev)).cpu().numpy()
        want = [pt.reshape(N, nb_vox, NB_LABELS), pred.reshape(N, nb_vox, NB_LABELS), pv.reshape(N, nb_vox)]
        if with_prior:
            want.append(pp.reshape(N, nb_vox, NB_LABELS))
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and bits_equal(g.cpu().numpy(), w)
        gen, _ = _generator(dev, 3, with_prior)
        two = ne.seg.predict_volume_stack([_model_a, _Predictor()], gen, 3, GRID)
        assert len(two) == 2 and len(two[1]) == 3 + with_prior and bits_equal(two[0][1].cpu().numpy(), want[1])


def test_argmax_and_quilt_capture_into_a_graph(dev):
    rng = np.random.default_rng(9)
    N, L = int(np.prod(GRID)), 8
    first, second = (torch.tensor(rng.random((N,) + PATCH + (L,), dtype=np.float32)).to(dev) for _ in range(2))
    x = first.clone()
    labels = torch.empty((N,) + PATCH, dtype=torch.int32, device=dev)
    prob = torch.empty((N,) + PATCH, dtype=torch.float32, device=dev)

    def step():
        seg._argmax(x, labels=labels, prob=prob)
        return ne.seg.quilt(labels, PATCH, GRID, STRIDE, nan_func='median'), ne.seg.quilt(prob, PATCH, GRID, STRIDE, nan_func='mean')

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab_g, prob_g = step()
    seen = []
    for values in (second, first, second):
        x.copy_(values)
        g.replay()
        torch.cuda.synchronize()
        got = (lab_g.cpu().numpy().copy(), prob_g.cpu().numpy().copy())
        lab_e, prob_e = step()
        torch.cuda.synchronize()
        assert bits_equal(got[0], lab_e.cpu().numpy()) and bits_equal(got[1], prob_e.cpu().numpy())
        want = rs.quilt(np.argmax(values.cpu().numpy(), -1).reshape((N,) + PATCH + (1,)), PATCH, GRID, STRIDE, np.nanmedian)[..., 0]
        assert bits_equal(got[0], want.astype(np.float32))
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])
