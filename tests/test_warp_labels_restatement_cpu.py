"""
CPU tests of tests/warp_labels_restatement.py, the oracle of the GPU tests of fused.warp_labels / fuse_labels / utils.resize_labels:
against an independent per-voxel brute force (a dict of id -> float32 weight sum in corner order, the winner by the tie rule), on two
tiny shapes; and the conditions the GPU inputs rely on -- with shifts drawn from the multiples of 0.5 at least 5 % of the voxels carry
an exact non-zero tie of their two largest labels and at least 1 % have an all-zero row.
"""

import itertools

import numpy as np
import pytest

import warp_labels_restatement as wr
from oracle import np_oracle as npo

F = np.float32
SHAPES = ((2, (5, 4, 6), (5, 4, 6)), (1, (4, 3, 5), (3, 5, 2)))


def corner_weights(ids, loc):
    """{id: p} at one float32 location of one map: the weights fl(fl(wx wy) wz) of the corners that carry the id, added in corner
    order starting from 0; and whether the location is out of bounds"""
    S = ids.shape
    i, w, oob = [], [], False
    for d, p in enumerate(loc):
        mx = F(S[d] - 1)
        oob = oob or bool(p < 0) or bool(p > mx)
        cl = min(max(p, F(0)), mx)
        l0 = min(max(F(np.floor(p)), F(0)), mx)
        l1 = min(max(F(l0 + F(1)), F(0)), mx)
        w0 = F(l1 - cl)
        i.append((int(l0), int(l1)))
        w.append((w0, F(F(1) - w0)))
    acc = {}
    for c in itertools.product((0, 1), repeat=len(S)):
        wt = w[0][c[0]]
        for d in range(1, len(S)):
            wt = F(wt * w[d][c[d]])
        l = int(ids[tuple(i[d][c[d]] for d in range(len(S)))])
        acc[l] = F(acc.get(l, F(0)) + wt)
    return acc, oob


def winner(acc, L):
    best, bp = 0, F(0)
    for l in sorted(acc):                                      # ascending: a later id only wins when strictly larger
        if (L is None or 0 <= l < L) and acc[l] > bp:
            best, bp = l, acc[l]
    return best, bp


def brute_warp(ids, locs, L, fill_label):
    """ids [B, *S], locs [B, *O, D] float32 absolute locations"""
    B, O = ids.shape[0], locs.shape[1:-1]
    out, prob = np.zeros((B,) + O, np.int64), np.zeros((B,) + O, F)
    for b in range(B):
        for q in np.ndindex(*O):
            acc, oob = corner_weights(ids[b], locs[b][q])
            out[b][q], prob[b][q] = (fill_label, F(0)) if (oob and fill_label is not None) else winner(acc, L)
    return out, prob


def brute_fuse(atlases, locs, weights, L, fill_label):
    N, O = atlases.shape[0], locs.shape[1:-1]
    out, votes = np.zeros(O, np.int64), np.zeros(O, F)
    for q in np.ndindex(*O):
        V, voted = {}, False
        for n in range(N):
            acc, oob = corner_weights(atlases[n], locs[n][q])
            if oob and fill_label is not None:
                continue
            voted = True
            for l, p in acc.items():
                V[l] = F(V.get(l, F(0)) + F(F(weights[n]) * p))
        out[q], votes[q] = winner(V, L) if voted else (fill_label, F(0))
    return out, votes


def shift_locs(shift):
    """[B, *O, D] 'ij' displacements -> float32 locations (grid + shift, one rounding)"""
    O = shift.shape[1:-1]
    mesh = np.stack(np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij'), -1)
    return (mesh[None] + shift).astype(F)


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1].dtype == F and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize('B,S,O', SHAPES)
@pytest.mark.parametrize('L', [1, 2, 5, None])
def test_warp_against_brute_force(B, S, O, L):
    rng = np.random.default_rng(7 + (L or 0))
    ids = wr.iid_ids(rng, (B,) + S, L) if L else rng.choice([0, 2, 41, 2035, 14175, -3, (1 << 31) - 1], (B,) + S)
    for field in (wr.gaussian_field(rng, B, O), wr.half_integer_field(rng, B, O)):
        for fill in (None, 0, 7):
            assert same(wr.warp_labels(ids, field, L, fill_label=fill), brute_warp(ids, shift_locs(field), L, fill)), (L, fill)
    f = wr.half_integer_field(rng, B, O)
    assert same(wr.warp_labels(ids, f[:1], L, single_transform=True), brute_warp(ids, shift_locs(np.repeat(f[:1], B, 0)), L, None))
    fxy = np.concatenate([f[..., 1:2], f[..., 0:1], f[..., 2:]], -1)
    assert same(wr.warp_labels(ids, fxy, L, indexing='xy'), brute_warp(ids, shift_locs(f), L, None))


def test_warp_2d_against_brute_force():
    rng = np.random.default_rng(11)
    ids = wr.iid_ids(rng, (2, 6, 7), 3)
    for field in (wr.gaussian_field(rng, 2, (5, 8), 1.5), wr.half_integer_field(rng, 2, (5, 8), 2)):
        for fill in (None, 0):
            assert same(wr.warp_labels(ids, field, 3, fill_label=fill), brute_warp(ids, shift_locs(field), 3, fill))


@pytest.mark.parametrize('shift_center', [True, False])
def test_affine_against_brute_force(shift_center):
    rng = np.random.default_rng(12)
    ids = wr.iid_ids(rng, (2, 5, 4, 6), 4)
    M = (np.eye(3, 4, dtype=F)[None] + rng.normal(0, 0.15, (2, 3, 4))).astype(F)
    for shape in (None, (4, 6, 3)):
        O = shape or (5, 4, 6)
        shift = np.stack([npo.affine_to_dense_shift(M[b], list(O), shift_center=shift_center) for b in range(2)])
        for fill in (None, 9):
            got = wr.warp_labels(ids, M, 4, fill_label=fill, shape=shape, shift_center=shift_center)
            assert same(got, brute_warp(ids, shift_locs(shift), 4, fill))


@pytest.mark.parametrize('zoom', [2, 0.5, (1.5, 1, 0.75)])
def test_resize_against_brute_force(zoom):
    rng = np.random.default_rng(13)
    S = (5, 4, 6)
    ids = wr.iid_ids(rng, S, 3)
    zf = list(zoom) if isinstance(zoom, tuple) else [zoom] * 3
    O = npo.resize_new_shape(S, zf)
    grid = np.stack(np.meshgrid(*[npo.tf_linspace(0., S[d] - 1., O[d]) for d in range(3)], indexing='ij'), -1).astype(F)
    for L in (3, None):
        assert same(wr.resize_labels(ids, zf, L), tuple(x[0] for x in brute_warp(ids[None], grid[None], L, None)))


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('L', [4, None])
def test_fusion_against_brute_force(N, L):
    rng = np.random.default_rng(14 + N)
    S, O = (5, 4, 6), (4, 5, 3)
    atl = rng.integers(-1, 8 * N + 2, (N,) + S)
    for field in (wr.gaussian_field(rng, N, O), wr.half_integer_field(rng, N, O)):
        for w in (None, rng.uniform(0, 2, N).astype(F), np.zeros(N, F)):
            for fill in (None, 5):
                got = wr.fuse_labels(atl, field, w, L, fill)
                assert same(got, brute_fuse(atl, shift_locs(field), np.ones(N, F) if w is None else w, L, fill)), (N, L, fill)
    shared = wr.half_integer_field(rng, 1, O)
    assert same(wr.fuse_labels(atl, shared[0], None, L), brute_fuse(atl, shift_locs(np.repeat(shared, N, 0)), np.ones(N, F), L, None))
    if N == 1:                                                  # one atlas with weight 1 is the plain warp
        assert same(wr.fuse_labels(atl, shared, None, L), tuple(x[0] for x in wr.warp_labels(atl, shared, L)))


@pytest.mark.parametrize('L', [2, 5, 33])
def test_half_integer_inputs_carry_ties_and_zero_rows(L):
    """what tests/test_gpu_warp_labels.py relies on, at its shape: the tie rule and the all-zero case are exercised by many voxels"""
    rng = np.random.default_rng(300 + L)
    B, S = 2, (19, 14, 27)
    ids = wr.iid_ids(rng, (B,) + S, L)
    field = wr.half_integer_field(rng, B, S)
    ties, _ = wr.tie_and_zero_fractions(npo.spatial_transformer(wr.one_hot(ids, L), field))
    _, zeros = wr.tie_and_zero_fractions(npo.spatial_transformer(wr.one_hot(ids, L), field, fill_value=0))
    print('L = %d: %.1f %% ties, %.1f %% all-zero rows under a fill' % (L, 100 * ties, 100 * zeros))
    assert ties >= 0.05 and zeros >= 0.01


def test_half_integer_fusion_carries_ties():
    rng = np.random.default_rng(304)
    N, L, S = 3, 4, (19, 14, 27)
    atl = wr.iid_ids(rng, (N,) + S, L)
    V, _ = wr.fuse_votes(atl, wr.half_integer_field(rng, N, S), None, L, False)
    ties, zeros = wr.tie_and_zero_fractions(V)
    print('fusion of 3 at L = 4: %.1f %% ties, %.1f %% all-zero rows' % (100 * ties, 100 * zeros))
    assert ties >= 0.05
