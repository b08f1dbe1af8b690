"""
The oracle of the distance-transform tests (tests/test_edt_abi.py, tests/test_gpu_edt.py): NumPy by DEFINITION, not by the separable
algorithm of csrc/edt.hip.
    sq_dist          the squared distance from every voxel to the nearest feature voxel by brute force over all pairs, chunked: int64 at
                     unit spacing (returned as float64, +inf where there is no feature voxel), float64 with a sampling
    surface          voxels of a mask with a face neighbour outside it (the outside of the volume counts as outside), by comparing
                     shifted copies
    signed_sq        VoxelMorph's signed_dist_trf, restated on the squares: +d^2(p, set) outside the set, -d^2(p, complement) inside
    surface_metrics  the metric definitions of metrics.SurfaceDistance in float64, with np.percentile itself
"""

import numpy as np

PAIRS_PER_CHUNK = 1 << 22


def sq_dist(feat, sampling=None):
    """feat: bool [*S].  Returns float64 [*S]: min over feature voxels q of sum_a (s_a (p_a - q_a))^2, +inf without a feature."""
    feat = np.asarray(feat, dtype=bool)
    nd = feat.ndim
    out = np.full(feat.size, np.inf, dtype=np.float64)
    q = np.nonzero(feat)
    if q[0].size == 0:
        return out.reshape(feat.shape)
    if q[0].size == feat.size:                                                   # every voxel is its own nearest feature voxel
        return np.zeros(feat.shape, dtype=np.float64)
    p = np.unravel_index(np.arange(feat.size), feat.shape)
    unit = sampling is None
    s = [1] * nd if unit else [float(np.float32(v)) for v in (np.repeat(sampling, nd) if np.ndim(sampling) == 0 else sampling)]
    step = max(1, PAIRS_PER_CHUNK // q[0].size)
    if unit:
        # every pair, in int64, as |p|^2 + |q|^2 - 2 p.q (exact: integers), which takes one pass over the pairs instead of one per axis
        P, Q = np.stack(p, 1).astype(np.int64), np.stack(q, 1).astype(np.int64)
        pp, qq = (P * P).sum(1), (Q * Q).sum(1)
        for beg in range(0, feat.size, step):
            d2 = P[beg:beg + step] @ Q.T
            d2 *= -2
            d2 += pp[beg:beg + step, None]
            d2 += qq[None, :]
            out[beg:beg + step] = d2.min(1)                                      # (an int64 below 2^53: exact in float64)
        return out.reshape(feat.shape)
    for beg in range(0, feat.size, step):
        acc = None
        for a in range(nd):
            diff = (p[a][beg:beg + step, None].astype(np.float64) - q[a][None, :].astype(np.float64)) * s[a]
            acc = diff * diff if acc is None else acc + diff * diff
        out[beg:beg + step] = acc.min(1)
    return out.reshape(feat.shape)


def signed_sq(mask, sampling=None):
    """+d^2(p, mask) outside the mask, -d^2(p, ~mask) inside; +inf for an empty mask, -inf for a full one"""
    mask = np.asarray(mask, dtype=bool)
    return np.where(mask, -sq_dist(~mask, sampling), sq_dist(mask, sampling))


def root32(d2):
    """what the device returns for a squared distance that float32 holds exactly: the correctly rounded float32 root, signed"""
    d2 = np.asarray(d2, dtype=np.float64)
    r = np.sqrt(np.abs(d2).astype(np.float32))
    assert r.dtype == np.float32
    return np.where(d2 < 0, -r, r)


def surface(mask):
    """mask & ~erosion(mask) for the 2 D-connected cross and a border of zeros, by neighbour comparison"""
    mask = np.asarray(mask, dtype=bool)
    padded = np.pad(mask, 1, constant_values=False)
    inside = mask.copy()
    core = tuple(slice(1, -1) for _ in range(mask.ndim))
    for a in range(mask.ndim):
        for shift in (0, 2):
            sl = list(core)
            sl[a] = slice(shift, shift + mask.shape[a])
            inside &= padded[tuple(sl)]
    return mask & ~inside


def surface_metrics(t, p, labels, voxel_size=None, percentiles=(95,)):
    """t, p: integer maps [B, *S].  Returns a dict of float64 [B, L] arrays (counts int64); 'hd_percentile' is [len(percentiles), B, L].
    NaN wherever either surface is empty."""
    t, p = np.asarray(t), np.asarray(p)
    B, L = t.shape[0], len(labels)
    keys = ('max_tp', 'max_pt', 'mean_tp', 'mean_pt', 'hausdorff', 'assd', 'sum_tp', 'sum_pt')
    out = {k: np.full((B, L), np.nan) for k in keys}
    out['count_t'] = np.zeros((B, L), np.int64)
    out['count_p'] = np.zeros((B, L), np.int64)
    out['hd_percentile'] = np.full((len(percentiles), B, L), np.nan)
    for b in range(B):
        for k, lab in enumerate(labels):
            st, sp = surface(t[b] == lab), surface(p[b] == lab)
            out['count_t'][b, k], out['count_p'][b, k] = st.sum(), sp.sum()
            if not st.any() or not sp.any():
                continue
            d_tp = np.sqrt(sq_dist(sp, voxel_size))[st]
            d_pt = np.sqrt(sq_dist(st, voxel_size))[sp]
            out['max_tp'][b, k], out['max_pt'][b, k] = d_tp.max(), d_pt.max()
            out['sum_tp'][b, k], out['sum_pt'][b, k] = d_tp.sum(), d_pt.sum()
            out['mean_tp'][b, k], out['mean_pt'][b, k] = d_tp.mean(), d_pt.mean()
            out['hausdorff'][b, k] = max(d_tp.max(), d_pt.max())
            out['assd'][b, k] = (d_tp.sum() + d_pt.sum()) / (d_tp.size + d_pt.size)
            both = np.concatenate([d_tp, d_pt])
            for j, q in enumerate(percentiles):
                out['hd_percentile'][j, b, k] = np.percentile(both, q)
    return out


# ---- inputs, made from seeds -------------------------------------------------------------------------------------------------------
def feature_set(kind, shape, seed=0):
    """bool [*shape]: 'empty', 'full', 'corners' (one voxel at each corner), 'ball', or a density in (0, 1)"""
    rng = np.random.default_rng(seed)
    if kind == 'empty':
        return np.zeros(shape, bool)
    if kind == 'full':
        return np.ones(shape, bool)
    if kind == 'corners':
        m = np.zeros(shape, bool)
        m[tuple(np.meshgrid(*[[0, n - 1] for n in shape], indexing='ij'))] = True
        return m
    if kind == 'ball':
        grid = np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in shape], indexing='ij')
        r2 = sum((g / max(0.35 * n, 0.6)) ** 2 for g, n in zip(grid, shape))
        return r2 <= 1.0
    return rng.random(shape) < float(kind)


def label_map(shape, nlabels, seed=0, coarse=3):
    """int32 [*shape] of blocky regions with ids 0 .. nlabels - 1 (coarse^D-voxel blocks: surfaces and interiors both exist)"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, nlabels, size=[(n + coarse - 1) // coarse for n in shape])
    for a in range(len(shape)):
        small = np.repeat(small, coarse, axis=a)
    return small[tuple(slice(0, n) for n in shape)].astype(np.int32)
