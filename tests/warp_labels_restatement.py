"""
The oracle of fused.warp_labels / utils.resize_labels / fused.fuse_labels (csrc/warp_argmax.hip), restated on the numpy oracle: the
one-hot map (ids[..., None] == arange(L)) goes through npo.spatial_transformer (npo.resize for the align-corners grid,
npo.affine_to_dense_shift for matrices), then np.argmax / max over the labels.  np.argmax returns the FIRST maximum: an exact tie goes
to the smaller id and an all-zero row gives id 0.  Fusion is the float32 running sum of w_n * warped_n in atlas order, then the arg-max.
Where every int32 value is a label (nb_labels=None) the ids are rank-compressed with np.unique first -- it sorts, so the order of the
ids and with it the tie rule are kept -- and mapped back afterwards.  Under a fill label the one-hot map is warped with fill_value=0
and the voxels sampled outside the volume get the fill label.
Also the input generators the GPU tests use; tests/test_warp_labels_restatement_cpu.py checks this file against an independent per-voxel
brute force and asserts what the GPU tests rely on (ties and all-zero rows are common in these inputs).
"""

import numpy as np

from oracle import np_oracle as npo

F = np.float32


def one_hot(ids, L):
    return (np.asarray(ids)[..., None] == np.arange(L)).astype(F)


def _ij(t, indexing):
    return np.concatenate([t[..., 1:2], t[..., 0:1], t[..., 2:]], -1) if indexing == 'xy' else t


def out_of_bounds(S, shift):
    """the fill mask of interpn for one 'ij' displacement field [*O, D] over a volume of shape S: the float32 location grid + shift
    (one rounding) lies outside [0, S - 1] along some axis"""
    O = shift.shape[:-1]
    mesh = np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij')
    oob = np.zeros(O, bool)
    for d in range(len(O)):
        loc = (mesh[d] + shift[..., d].astype(F)).astype(F)
        oob |= (loc < 0) | (loc > S[d] - 1)
    return oob


def _compress(ids):
    uniq, inv = np.unique(np.asarray(ids), return_inverse=True)
    return uniq, inv.reshape(np.shape(ids))


def dense_fields(ids_shape, trf, indexing='ij', single_transform=False, shape=None, shift_center=True):
    """trf (dense [Bt, *O, D] or affine [Bt, D, D + 1] / [Bt, D + 1, D + 1]) as one 'ij' displacement field per batch entry"""
    trf = np.asarray(trf, F)
    B, S = ids_shape[0], ids_shape[1:]
    D = len(S)
    out = []
    for b in range(B):
        t = trf[0 if single_transform else b]
        if t.ndim == 2:
            t = npo.affine_to_dense_shift(t, list(shape) if shape is not None else list(S), shift_center=shift_center)
        else:
            t = _ij(t, indexing)
        assert t.shape[-1] == D
        out.append(t.astype(F))
    return np.stack(out)


def warp_labels(ids, trf, nb_labels=None, indexing='ij', single_transform=False, fill_label=None, shape=None, shift_center=True):
    """ids [B, *S] integers -> (ids [B, *O] int64, prob [B, *O] float32)"""
    ids = np.asarray(ids)
    if nb_labels is None:
        uniq, compact = _compress(ids)
        out, prob = warp_labels(compact, trf, len(uniq), indexing, single_transform, None if fill_label is None else 0, shape, shift_center)
        out = uniq[out].astype(np.int64)
    else:
        fields = dense_fields(ids.shape, trf, indexing, single_transform, shape, shift_center)
        dense = npo.spatial_transformer(one_hot(ids, nb_labels), fields, fill_value=None if fill_label is None else 0)
        out, prob = np.argmax(dense, -1).astype(np.int64), dense.max(-1)
    if fill_label is not None:
        fields = dense_fields(ids.shape, trf, indexing, single_transform, shape, shift_center)
        oob = np.stack([out_of_bounds(ids.shape[1:], f) for f in fields])
        assert np.all(prob[oob] == 0)
        out[oob] = fill_label
    return out, prob


def resize_labels(ids, zoom_factor, nb_labels=None):
    """one un-batched map [*S] -> (ids, prob)"""
    ids = np.asarray(ids)
    zf = list(zoom_factor) if isinstance(zoom_factor, (list, tuple)) else [zoom_factor] * ids.ndim
    if nb_labels is None:
        uniq, compact = _compress(ids)
        out, prob = resize_labels(compact, zf, len(uniq))
        return uniq[out].astype(np.int64), prob
    dense = npo.resize(one_hot(ids, nb_labels), zf)
    return np.argmax(dense, -1).astype(np.int64), dense.max(-1)


def fuse_votes(atlases, trfs, weights, nb_labels, fill):
    """V [*O, L]: the float32 running sum of w_n * warped_n in atlas order, and the mask of voxels where every atlas is out of bounds"""
    atlases, trfs = np.asarray(atlases), np.asarray(trfs, F)
    N = atlases.shape[0]
    if trfs.ndim == atlases.ndim:
        trfs = trfs[None]
    w = np.ones(N, F) if weights is None else np.asarray(weights, F)
    V, all_oob = None, None
    for n in range(N):
        t = trfs[0 if trfs.shape[0] == 1 else n]
        warped = npo.spatial_transformer(one_hot(atlases[n:n + 1], nb_labels), t[None], fill_value=0 if fill else None)[0]
        term = (w[n] * warped).astype(F)
        V = (np.zeros_like(term) + term).astype(F) if V is None else (V + term).astype(F)
        oob = out_of_bounds(atlases.shape[1:], t) if fill else np.zeros(t.shape[:-1], bool)
        all_oob = oob if all_oob is None else (all_oob & oob)
    return V, all_oob


def fuse_labels(atlases, trfs, weights=None, nb_labels=None, fill_label=None):
    """atlases [N, *S] -> (ids [*O] int64, votes [*O] float32)"""
    atlases = np.asarray(atlases)
    if nb_labels is None:
        uniq, compact = _compress(atlases)
        V, all_oob = fuse_votes(compact, trfs, weights, len(uniq), fill_label is not None)
        out = uniq[np.argmax(V, -1)].astype(np.int64)
        out[V.max(-1) == 0] = 0                           # no label has a vote: id 0, not the smallest id of the maps
    else:
        V, all_oob = fuse_votes(atlases, trfs, weights, nb_labels, fill_label is not None)
        out = np.argmax(V, -1).astype(np.int64)
    votes = V.max(-1)
    if fill_label is not None:
        assert np.all(votes[all_oob] == 0)
        out[all_oob] = fill_label
    return out, votes


# ---- what the dense rows hold (asserted on the CPU for the inputs of the GPU tests) ---------------------------------------------------
def tie_and_zero_fractions(dense):
    """(share of voxels whose two largest values are equal and non-zero, share of all-zero rows) of dense [..., L]"""
    rows = dense.reshape(-1, dense.shape[-1])
    if rows.shape[1] == 1:
        return 0.0, float(np.mean(rows[:, 0] == 0))
    top = np.sort(rows, -1)[:, -2:]
    return float(np.mean((top[:, 0] == top[:, 1]) & (top[:, 1] > 0))), float(np.mean(top[:, 1] == 0))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def iid_ids(rng, shape, L):
    """i.i.d. ids from [-1, L + 1]: -1, L and L + 1 lie outside [0, L)"""
    return rng.integers(-1, L + 2, shape)


def gaussian_field(rng, B, O, sigma=2.5):
    return rng.normal(0, sigma, (B,) + tuple(O) + (len(O),)).astype(F)


def half_integer_field(rng, B, O, span=3):
    """shifts drawn from the multiples of 0.5 in [-span, span]: every weight is 0, 0.5 or 1, exact ties of the top two labels are common"""
    return (rng.integers(-2 * span, 2 * span + 1, (B,) + tuple(O) + (len(O),)) * 0.5).astype(F)
