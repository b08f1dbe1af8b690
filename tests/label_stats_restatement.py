"""
The definition the label statistics and the label confusion matrix are tested against (not a test file), in NumPy, and the id maps and
images the tests use.

stats(ids, image, slots): for every (entry, slot), with m = ids[e] == slots[l]:  m.sum();  np.nonzero(m) for the coordinate sums and
the bounding box (an empty slot holds (shape[a], -1));  the float64 sum of x[m] and of x[m] ** 2, x being the STORED values widened to
float64 (so the squares are exact);  np.nanmin / np.nanmax with (+inf, -inf) for an empty or all-NaN slot.  confusion(a, b, slots):
a double loop over the slots, with a last row and column for the ids that are in no slot.
"""

import functools

import numpy as np

SHAPES = ((2, 7, 9, 11), (1, 5, 6, 130), (3, 33, 65), (2, 16, 16, 16), (1, 40, 48, 56))       # [B, *S]
LABEL_COUNTS = (1, 3, 33, 256)
KINDS = ('blobs', 'iid', 'constant', 'absent', 'outside')
HEAD = (0, 2035, 41, -7)                                       # how every listed label set starts: unsorted, one negative id
OUTSIDE = (-2 ** 31, 2 ** 31 - 1, -3, 5000)                    # ids that are in no slot of any case


def slot_ids(n, listed):
    """the ids of the n slots: range(n), or an unsorted list of arbitrary distinct ids"""
    if not listed:
        return list(range(n))
    rest = np.random.default_rng(n).permutation(np.arange(100, 3000))
    return (list(HEAD) + [int(v) for v in rest if int(v) not in HEAD])[:n]


def outside_ids(n, listed):
    return OUTSIDE if listed else OUTSIDE[:3] + (n,)          # (without a list the id just past the last slot is in none)


def make_ids(kind, shape, slots, outside, seed=0):
    """an int32 id map [B, *S]"""
    rng = np.random.default_rng(seed + 7919 * len(slots) + int(np.prod(shape)))
    pool = np.asarray(slots, dtype=np.int64)
    batch, spatial = shape[0], shape[1:]
    if kind == 'constant':
        out = np.full(shape, pool[len(pool) // 2])
    elif kind == 'iid':
        out = rng.choice(pool, size=shape)
    elif kind == 'absent':                                     # the first listed label occurs nowhere
        out = rng.choice(pool[1:] if len(pool) > 1 else np.asarray(outside[:1], dtype=np.int64), size=shape)
    elif kind == 'outside':
        out = rng.choice(np.concatenate([pool, np.asarray(outside, dtype=np.int64)]), size=shape)
    elif kind == 'blobs':                                      # nearest-seed Voronoi cells: a wave sees one to three ids
        grid = np.stack(np.meshgrid(*[np.arange(s) for s in spatial], indexing='ij'), -1).reshape(-1, len(spatial)).astype(np.float64)
        out = np.empty(shape, dtype=np.int64)
        for e in range(batch):
            seeds = rng.random((12, len(spatial))) * np.asarray(spatial)
            owner = rng.choice(pool, size=12)
            near = ((grid[:, None, :] - seeds[None]) ** 2).sum(-1).argmin(1)
            out[e] = owner[near].reshape(spatial)
    else:
        raise ValueError(kind)
    return out.astype(np.int32)


def make_image(shape, channels, kind, seed=0):
    """float32 [B, *S, C] (channels None: no channel axis).  'small': integers in [-3, 3], whose sums and sums of squares every
    float32 order forms exactly on the shapes used here (sum of x^2 <= 9 * 107520 < 2^24); 'normal': 100 + 30 N(0, 1)"""
    rng = np.random.default_rng(seed + 31 * int(np.prod(shape)) + (channels or 0))
    full = tuple(shape) + (() if channels is None else (channels,))
    if kind == 'small':
        return rng.integers(-3, 4, size=full).astype(np.float32)
    return (100.0 + 30.0 * rng.standard_normal(full)).astype(np.float32)


def store(x, dtype):
    """(stored array as the device holds it, the float32 values it stands for)"""
    x = np.asarray(x, np.float32)
    if dtype == 'float32':
        return x, x
    if dtype == 'float16':
        h = x.astype(np.float16)
        return h, h.astype(np.float32)
    bits = x.view(np.uint32)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)                      # round to nearest even
    rounded = np.where(np.isnan(x), np.uint16(0x7FC0), rounded)
    return rounded, (rounded.astype(np.uint32) << 16).view(np.float32)


def stats(ids, image, slots):
    """the definition.  ids [B, *S]; image None or float32 [B, *S, C]; slots: the id of every slot.  A dict of arrays."""
    ids = np.asarray(ids)
    batch, spatial, nd, n = ids.shape[0], ids.shape[1:], ids.ndim - 1, len(slots)
    out = {'count': np.zeros((batch, n), np.int64), 'coord_sums': np.zeros((batch, n, nd), np.int64),
           'bbox_min': np.empty((batch, n, nd), np.int32), 'bbox_max': np.full((batch, n, nd), -1, np.int32)}
    out['bbox_min'][:] = np.asarray(spatial, np.int32)
    if image is not None:
        channels = image.shape[-1]
        for key in ('sum', 'sumsq', 'abs_sum'):
            out[key] = np.zeros((batch, n, channels), np.float64)
        out['min'] = np.full((batch, n, channels), np.inf, np.float32)
        out['max'] = np.full((batch, n, channels), -np.inf, np.float32)
    for e in range(batch):
        for l, label in enumerate(slots):
            m = ids[e] == label
            count = int(m.sum())
            out['count'][e, l] = count
            if count == 0:
                continue
            where = np.nonzero(m)
            for a in range(nd):
                out['coord_sums'][e, l, a] = where[a].astype(np.int64).sum()
                out['bbox_min'][e, l, a] = where[a].min()
                out['bbox_max'][e, l, a] = where[a].max()
            if image is not None:
                x = image[e][m]                                                                  # [count, C] float32
                x64 = x.astype(np.float64)
                out['sum'][e, l] = x64.sum(0)
                out['sumsq'][e, l] = (x64 ** 2).sum(0)
                out['abs_sum'][e, l] = np.abs(x64).sum(0)
                for c in range(channels):
                    col = x[:, c]
                    if not np.isnan(col).all():
                        out['min'][e, l, c] = np.nanmin(col)
                        out['max'][e, l, c] = np.nanmax(col)
    return out


def confusion(a, b, slots):
    """[B, L + 1, L + 1] int64 by a double loop over the slots; the last row / column: ids in no slot"""
    a, b = np.asarray(a), np.asarray(b)
    batch, n = a.shape[0], len(slots)
    out = np.zeros((batch, n + 1, n + 1), np.int64)
    for e in range(batch):
        none_a, none_b = ~np.isin(a[e], slots), ~np.isin(b[e], slots)
        for i in range(n + 1):
            mi = a[e] == slots[i] if i < n else none_a
            if not mi.any():
                continue
            sub = b[e][mi]                                                                       # b on the voxels of a's slot i
            for j in range(n):
                out[e, i, j] = (sub == slots[j]).sum()
            out[e, i, n] = none_b[mi].sum()
    return out


@functools.lru_cache(maxsize=None)
def confusion_case(shape, n, listed):
    """(slots, a, b, the definition's confusion matrix): a with ids in no slot, b blobs; computed once, shared"""
    slots, a, _ = case('outside', shape, n, listed)
    _, b, _ = case('blobs', shape, n, listed, seed=1)
    return slots, a, b, confusion(a, b, slots)


@functools.lru_cache(maxsize=None)
def case(kind, shape, n, listed, seed=0):
    """(slots, ids, the definition's integer statistics) of one test case; computed once, shared, not to be written to"""
    slots = slot_ids(n, listed)
    ids = make_ids(kind, shape, slots, outside_ids(n, listed), seed)
    ids.setflags(write=False)
    return slots, ids, stats(ids, None, slots)
