"""
ne.fused.warp_labels / fuse_labels, ne.utils.resize_labels and the two label layers (csrc/warp_argmax.hip) against the one-hot oracle of
tests/warp_labels_restatement.py: np.argmax / max of the numpy SpatialTransformer on (ids[..., None] == arange(L)).  Every comparison is
exact: ids with array_equal, prob and votes bit for bit.  The shapes are the smallest that reach every arm: 7182 voxels are not a
multiple of 256 (a block walks several steps, the last with dead lanes), S_z = 1 takes the unpaired gather, a leading extent of 1 is the
2-D entry, and a 24^3 blob map has waves whose 64 voxels see eight equal corners of one id (the fast path) next to waves that do not.
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
import warp_labels_restatement as wr
from conftest import bits_equal
from neurite_amd import synth

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = ((2, (19, 14, 27), (19, 14, 27)), (1, (9, 8, 12), (7, 11, 5)))
BIG_IDS = np.array([0, 2, 41, 2035, 14175, (1 << 31) - 1])


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def draw_ids(rng, shape, L):
    return wr.iid_ids(rng, shape, L) if L else rng.choice(BIG_IDS, shape)


def check_warp(dev, ids, trf, L, dtype=torch.int32, want=None, **kw):
    """every assertion of this file for one warp: ids and prob against the oracle, and the same ids without the prob pointer"""
    want_ids, want_prob = want if want is not None else wr.warp_labels(ids, trf, L, **kw)
    m, t = G(ids, dev).to(dtype), G(trf, dev)
    got, prob = ne.fused.warp_labels(m, t, nb_labels=L, return_prob=True, **kw)
    assert got.dtype == dtype and prob.dtype == torch.float32 and not got.requires_grad and not prob.requires_grad
    assert np.array_equal(N(got).astype(np.int64), want_ids), (L, kw)
    assert bits_equal(N(prob), want_prob), (L, kw)
    alone = ne.fused.warp_labels(m, t, nb_labels=L, **kw)
    assert alone.dtype == dtype and torch.equal(alone, got), (L, kw)
    return got, prob


@pytest.mark.parametrize('L', [1, 2, 5, 33, None])
def test_iid_ids_against_oracle(dev, L):
    """i.i.d. ids from [-1, L + 1] (or from large ids where every value is a label): up to 8 labels per voxel, under a Gaussian field
    and under half-integer shifts (exact ties), with the edge clamped and under two fill labels"""
    rng = np.random.default_rng(300 + (L or 0))
    for B, S, O in SHAPES:
        ids = draw_ids(rng, (B,) + S, L)
        for trf in (wr.gaussian_field(rng, B, O), wr.half_integer_field(rng, B, O)):
            for fill in (None, 0, 7):
                check_warp(dev, ids, trf, L, fill_label=fill)
        trf = wr.half_integer_field(rng, B, O)
        check_warp(dev, ids, trf[:1], L, single_transform=True)
        check_warp(dev, ids, trf, L, indexing='xy', fill_label=0)
        check_warp(dev, ids, trf[:1], L, single_transform=True, indexing='xy')


@pytest.mark.parametrize('S,O', [((9, 8, 1), (7, 6, 3)), ((6, 7, 2), (5, 9, 4)), ((1, 9, 12), (1, 7, 5)), ((1, 9, 12), (3, 7, 5)),
                                 ((1, 1, 1), (2, 2, 2))])
def test_thin_volumes(dev, S, O):
    """S_z = 1 takes the unpaired gather; a leading extent of 1 is how 2-D maps run"""
    rng = np.random.default_rng(46)
    for L in (4, None):
        ids = draw_ids(rng, (2,) + S, L)
        for trf in (wr.gaussian_field(rng, 2, O, 1.5), wr.half_integer_field(rng, 2, O, 2)):
            for fill in (None, 3):
                check_warp(dev, ids, trf, L, fill_label=fill)


def test_2d_maps_against_the_2d_oracle(dev):
    rng = np.random.default_rng(47)
    for L in (3, None):
        ids = draw_ids(rng, (2, 13, 17), L)
        for trf in (wr.gaussian_field(rng, 2, (11, 9)), wr.half_integer_field(rng, 2, (11, 9))):
            for kw in ({}, {'fill_label': 0}, {'fill_label': 5, 'indexing': 'xy'}):
                check_warp(dev, ids, trf, L, **kw)
        check_warp(dev, ids, wr.half_integer_field(rng, 1, (11, 9)), L, single_transform=True)
        got = ne.fused.warp_labels(G(ids, dev).unsqueeze(-1), G(wr.gaussian_field(rng, 2, (11, 9)), dev), nb_labels=L)
        assert got.shape == (2, 11, 9)


def corner_ids(ids, shift):
    """the ids at the 8 corners of every output voxel of one map under one 'ij' displacement field: [8, voxels]"""
    S, O = ids.shape, shift.shape[:-1]
    mesh = np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij')
    i = []
    for d in range(3):
        l0 = np.clip(np.floor((mesh[d] + shift[..., d]).astype(F)), 0, S[d] - 1)
        i.append((l0.astype(np.int64), np.clip(l0 + 1, 0, S[d] - 1).astype(np.int64)))
    return np.stack([ids[i[0][x], i[1][y], i[2][z]].reshape(-1) for x in (0, 1) for y in (0, 1) for z in (0, 1)])


def corner_runs(ids, shift):
    """per aligned run of 64 consecutive output voxels of one map: do all 64 see eight equal corners of ONE id?"""
    c = corner_ids(ids, shift)
    n = c.shape[1] // 64 * 64
    eq8 = np.all(c == c[:1], 0)[:n].reshape(-1, 64)
    first = c[0, :n].reshape(-1, 64)
    return eq8.all(1) & (first == first[:, :1]).all(1)


def candidate_counts(atl, trfs):
    """distinct ids among the 8 N corners of every output voxel (the edge clamped, every value a label)"""
    c = np.sort(np.concatenate([corner_ids(atl[n], trfs[n]) for n in range(atl.shape[0])]), 0)
    return 1 + (c[1:] != c[:-1]).sum(0)


def test_blob_labels_fast_path(dev):
    """structures with an interior: waves that skip the slot merge (and, without prob, the weights) next to waves that do not"""
    L, size = 5, 24
    ids = np.stack([N(synth.blob_labels(s, size, L, coarse=2)) for s in (1, 2)])
    trf = np.stack([N(synth.smooth_displacement(s, size, coarse=4)) for s in (5, 6)])
    # (a block starts at a multiple of 256 voxels, so a wave's 64 voxels are an aligned run of 64)
    for b in range(2):
        uniform = corner_runs(ids[b], trf[b])
        assert uniform.any() and not uniform.all(), uniform.sum()
    for nb in (L, 3, None):                                       # (3: whole waves of a background id)
        for fill in (None, 0):
            check_warp(dev, ids, trf, nb, fill_label=fill)
    check_warp(dev, ids, np.zeros_like(trf), L)                   # zero flow: the map itself, prob 1
    got, prob = check_warp(dev, ids, np.zeros_like(trf), None, dtype=torch.int64)
    assert np.array_equal(N(got), ids) and np.all(N(prob) == 1)


def test_integer_dtypes_and_trailing_axis(dev):
    rng = np.random.default_rng(44)
    L, S = 7, (9, 8, 12)
    ids = rng.integers(0, L + 2, (2,) + S)
    trf = wr.gaussian_field(rng, 2, S)
    want = wr.warp_labels(ids, trf, L)
    for dt in (torch.int32, torch.uint8, torch.int8, torch.int16, torch.int64):
        check_warp(dev, ids, trf, L, dtype=dt, want=want)
        got = ne.fused.warp_labels(G(ids, dev).to(dt).unsqueeze(-1), G(trf, dev), nb_labels=L)
        assert got.dtype == dt and got.shape == (2,) + S and np.array_equal(N(got), want[0])
    # restricted labels: an int64 id beyond int32 is background, not wrapped into [0, L)
    big = ids.copy()
    big[ids == L + 1] = (1 << 32) + 1
    check_warp(dev, big, trf, L, dtype=torch.int64, want=want)
    # every value a label: int64 and int16 ids as they are
    check_warp(dev, rng.choice(BIG_IDS, (2,) + S), trf, None, dtype=torch.int64)
    check_warp(dev, rng.choice([-300, -1, 0, 7, 32767], (2,) + S), trf, None, dtype=torch.int16, fill_label=-5)


def one_hot_affine(dev, ids, M, L, **kw):
    """argmax / max of fused.affine_warp on the one-hot map (bit-identical to the dense-field path), and its out-of-bounds mask"""
    dense = N(ne.fused.affine_warp(G(wr.one_hot(ids, L), dev), G(M, dev), **kw))
    inside = N(ne.fused.affine_warp(torch.ones(ids.shape + (1,), device=dev), G(M, dev), **dict(kw, fill_value=0)))[..., 0]
    return np.argmax(dense, -1).astype(np.int64), dense.max(-1), inside == 0


@pytest.mark.parametrize('shift_center', [True, False])
def test_affine_front_end(dev, shift_center):
    rng = np.random.default_rng(48)
    B, S = 2, (19, 14, 27)
    M = (np.eye(3, 4, dtype=F)[None] + rng.normal(0, 0.03, (B, 3, 4))).astype(F)
    M[:, :, 3] += np.array([-1.5, 2.25, -0.75], F)                # x = 0 is sampled outside the volume
    seen_oob = 0
    for L in (5, None):
        ids = draw_ids(rng, (B,) + S, L)
        uniq, compact = (None, ids) if L else wr._compress(ids)
        for shape in (None, (7, 11, 5)):
            for single in (False, True):
                kw = dict(shape=shape, shift_center=shift_center, single_transform=single)
                for fill in (None, 0, 7):
                    w_ids, w_prob, oob = one_hot_affine(dev, compact, M, L or len(uniq), fill_value=None if fill is None else 0, **kw)
                    if uniq is not None:
                        w_ids = uniq[w_ids].astype(np.int64)
                    if fill is not None:
                        assert not oob.all() and np.all(w_prob[oob] == 0)
                        seen_oob += int(oob.sum())
                        w_ids[oob] = fill
                    check_warp(dev, ids, M, L, want=(w_ids, w_prob), fill_label=fill, **kw)
    assert seen_oob > 0
    # a square matrix is taken by its first three rows
    M4 = np.concatenate([M, np.broadcast_to(np.array([0, 0, 0, 1], F), (B, 1, 4))], 1)
    assert torch.equal(ne.fused.warp_labels(G(ids, dev), G(M4, dev), shift_center=shift_center),
                       ne.fused.warp_labels(G(ids, dev), G(M, dev), shift_center=shift_center))


@pytest.mark.parametrize('zoom', [2, 0.5, (1.5, 1, 0.75)])
def test_resize_labels(dev, zoom):
    rng = np.random.default_rng(49)
    for S in ((19, 14, 27), (9, 8, 12)):
        for L in (5, None):
            ids = draw_ids(rng, (2,) + S, L)
            want = [wr.resize_labels(ids[b], zoom, L)[0] for b in range(2)]
            for dt in (torch.int32, torch.int64):
                got = ne.utils.resize_labels(G(ids[0], dev).to(dt), zoom, nb_labels=L)
                assert got.dtype == dt and np.array_equal(N(got).astype(np.int64), want[0]), (S, L)
            layer = ne.layers.LabelResize(zoom, nb_labels=L)
            assert np.array_equal(N(layer(G(ids, dev))).astype(np.int64), np.stack(want))
            out = layer(G(ids, dev).unsqueeze(-1))
            assert out.shape[-1] == 1 and np.array_equal(N(out[..., 0]).astype(np.int64), np.stack(want))
    ids2 = draw_ids(rng, (13, 17), 3)
    z2 = zoom[:2] if isinstance(zoom, tuple) else zoom
    assert np.array_equal(N(ne.utils.zoom_labels(G(ids2, dev), z2, nb_labels=3)).astype(np.int64), wr.resize_labels(ids2, z2, 3)[0])


def test_label_transformer_layer(dev):
    rng = np.random.default_rng(50)
    B, S, O = SHAPES[1]
    ids, trf = G(wr.iid_ids(rng, (B,) + S, 5), dev), G(wr.gaussian_field(rng, B, O), dev)
    layer = ne.layers.LabelTransformer(nb_labels=5, fill_label=2, indexing='xy')
    want = ne.fused.warp_labels(ids, trf, nb_labels=5, fill_label=2, indexing='xy')
    assert torch.equal(layer([ids, trf]), want) and torch.equal(layer([ids.unsqueeze(-1), trf]), want.unsqueeze(-1))
    M = G(np.eye(3, 4, dtype=F)[None] + rng.normal(0, 0.05, (1, 3, 4)).astype(F), dev)
    assert torch.equal(ne.layers.LabelTransformer(shift_center=False)([ids, M]), ne.fused.warp_labels(ids, M, shift_center=False))
    trf.requires_grad_()
    assert not layer([ids, trf]).requires_grad


def check_fuse(dev, atl, trfs, w, L, fill=None, dtype=torch.int32):
    want_ids, want_votes = wr.fuse_labels(atl, trfs, w, L, fill)
    a, t = G(atl, dev).to(dtype), G(trfs, dev)
    got, votes = ne.fused.fuse_labels(a, t, weights=w, nb_labels=L, fill_label=fill, return_votes=True)
    assert got.dtype == dtype and not got.requires_grad and not votes.requires_grad
    assert np.array_equal(N(got).astype(np.int64), want_ids), (L, fill)
    assert bits_equal(N(votes), want_votes), (L, fill)
    assert torch.equal(ne.fused.fuse_labels(a, t, weights=w, nb_labels=L, fill_label=fill), got)
    return got, votes


@pytest.mark.parametrize('n', [1, 2, 3, 6, 16])
def test_fusion_against_oracle(dev, n):
    """i.i.d. ids from 8 N + 3 values: some voxels meet many distinct candidates.  A lane's list holds 32: up to 3 atlases it holds them
    all, at 6 some voxels of a wave overflow it and some do not, at 16 nearly all do (the list-free pass)"""
    rng = np.random.default_rng(60 + n)
    S, O = (SHAPES[0][1], SHAPES[0][2]) if n <= 3 else (SHAPES[1][1], SHAPES[1][2])
    atl = rng.integers(-1, 8 * n + 2, (n,) + S)
    gauss, half = wr.gaussian_field(rng, n, O), wr.half_integer_field(rng, n, O)
    if n >= 2:
        V, _ = wr.fuse_votes(atl, gauss, None, 8 * n, False)
        assert (V > 0).sum(-1).max() > 8
        for trfs in (gauss, half):
            cand = candidate_counts(atl, trfs)
            assert cand.max() > 8 and (n < 6 or (cand > 32).any()) and (n != 6 or (cand <= 32).any()), (cand.min(), cand.max())
    unequal = rng.uniform(0.25, 2, n).astype(F)
    unequal[n // 2] = 0                                           # (n = 1: the only weight)
    for L in (8 * n, None):
        check_fuse(dev, atl, gauss, None, L)
        check_fuse(dev, atl, half, None, L)                       # equal weights: ties
        check_fuse(dev, atl, half, np.full(n, 0.5, F), L, fill=0)
        check_fuse(dev, atl, gauss, unequal, L, fill=7)
        check_fuse(dev, atl, half[0], None, L)                    # one field for every atlas
        check_fuse(dev, atl, gauss[:1], unequal, L, fill=3, dtype=torch.int64)
    check_fuse(dev, rng.choice(BIG_IDS, (n,) + S), half, None, None)     # few labels: the list serves any number of atlases
    check_fuse(dev, rng.integers(-1, 6, (n,) + S), gauss, unequal, 4, fill=2)
    if n == 1:                                                    # one atlas of weight 1 is warp_labels
        for L in (8, None):
            for fill in (None, 4):
                ids, prob = ne.fused.warp_labels(G(atl, dev), G(gauss, dev), nb_labels=L, fill_label=fill, return_prob=True)
                got, votes = ne.fused.fuse_labels(G(atl, dev), G(gauss, dev), nb_labels=L, fill_label=fill, return_votes=True)
                assert torch.equal(got, ids[0]) and bits_equal(N(votes), N(prob[0]))


def test_run_to_run(dev):
    rng = np.random.default_rng(45)
    B, S, O = SHAPES[0]
    ids, trf = G(wr.iid_ids(rng, (B,) + S, 33), dev), G(wr.gaussian_field(rng, B, O), dev)
    a = [N(x) for x in ne.fused.warp_labels(ids, trf, nb_labels=33, return_prob=True)]
    b = [N(x) for x in ne.fused.warp_labels(ids, trf, nb_labels=33, return_prob=True)]
    assert np.array_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    atl, trfs = G(rng.integers(-1, 26, (3,) + S), dev), G(wr.gaussian_field(rng, 3, O), dev)
    a = [N(x) for x in ne.fused.fuse_labels(atl, trfs, weights=[0.5, 1.0, 0.75], return_votes=True)]
    b = [N(x) for x in ne.fused.fuse_labels(atl, trfs, weights=[0.5, 1.0, 0.75], return_votes=True)]
    assert np.array_equal(a[0], b[0]) and bits_equal(a[1], b[1])
