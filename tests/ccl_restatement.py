"""
The oracle of the connected-component tests (tests/test_ccl_abi.py, test_ccl_core_cpu.py, test_gpu_ccl.py): by DEFINITION, not by the
union-find of csrc/ccl.hip.
    label         a flood fill in raster order: the first unvisited foreground voxel opens component 1, 2, ... and takes every voxel that a
                  chain of neighbours with EQUAL ids reaches; neighbours are the offsets o of {-1, 0, 1}^nd with 0 < sum |o| <= connectivity
    table         per label slot the number of components and the size of the largest
    keep          the selections (largest per slot with ties to the lowest number, a minimum size, no voxel on the border of the volume)
    fill_holes    mask | (components of ~mask that do not touch the border)
and the shapes and patterns the tests share.
"""

import itertools

import numpy as np

SHAPES = [(1, 1, 1), (1, 7, 1), (5, 6, 7), (3, 65, 66), (130, 3, 5), (2, 2, 129), (17, 65), (64, 64), (1, 130)]
# the kernels have no spatial tile: a block takes CHUNK consecutive voxels of an entry's raster, so the seams lie in the linear index.
# CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 voxels, as one row and as rows that straddle the seam
CHUNK = 1024
CHUNK_SHAPES = [(1, 1023), (1, 1024), (1, 1025), (1, 2049), (1023, 1), (2049, 1), (3, 683), (1, 3, 683), (2, 32, 16), (41, 5, 5), (5, 5, 41),
                (1025, 2)]
# the scan of the chunk counts is one block of 256 threads per entry that loops with a carry: 257 chunks (above 262144 voxels) reach its
# second round
SCAN_SHAPE = (257, 1021)


_LABEL_CACHE = {}                                   # label() is pure and the tests ask for the same fill several times


def offsets(nd, connectivity):
    return [o for o in itertools.product((-1, 0, 1), repeat=nd) if 0 < sum(abs(v) for v in o) <= connectivity]


def foreground(x, labels=None):
    x = np.asarray(x)
    return x != 0 if labels is None else np.isin(x, np.asarray(list(labels), dtype=x.dtype))


def label(x, connectivity=1, labels=None):
    """x [*S]: a mask (labels None: nonzero is foreground, all one id) or an id map with the listed ids as foreground.
    Returns (components int32 [*S], count)."""
    x = np.asarray(x)
    memo = (x.tobytes(), x.shape, x.dtype.str, connectivity, None if labels is None else tuple(labels))
    if memo in _LABEL_CACHE:
        return _LABEL_CACHE[memo]
    fg = foreground(x, labels)
    key = np.where(fg, 1, 0) if labels is None else x
    shape, nd = x.shape, x.ndim
    # a border of background all round, so that no neighbour needs a bounds check
    pad_fg = np.pad(fg, 1)
    pad_key = np.pad(key, 1)
    pshape = pad_fg.shape
    strides = [int(np.prod(pshape[a + 1:])) for a in range(nd)]
    steps = [sum(o[a] * strides[a] for a in range(nd)) for o in offsets(nd, connectivity)]
    flat_fg, flat_key = pad_fg.reshape(-1), pad_key.reshape(-1)
    comp = np.zeros(flat_fg.size, dtype=np.int32)
    count = 0
    for v in np.flatnonzero(flat_fg):                                            # raster order
        if comp[v]:
            continue
        count += 1
        comp[v] = count
        k = flat_key[v]
        stack = [int(v)]
        while stack:
            p = stack.pop()
            for s in steps:
                q = p + s
                if flat_fg[q] and not comp[q] and flat_key[q] == k:
                    comp[q] = count
                    stack.append(q)
    comp = np.ascontiguousarray(comp.reshape(pshape)[tuple(slice(1, -1) for _ in range(nd))])
    _LABEL_CACHE[memo] = (comp, count)
    return comp, count


def on_border(shape):
    """bool [*S]: first or last along an axis"""
    b = np.zeros(shape, dtype=bool)
    for a in range(len(shape)):
        idx = [slice(None)] * len(shape)
        for i in (0, -1):
            idx[a] = i
            b[tuple(idx)] = True
    return b


def sizes_and_border(comp, count):
    sizes = np.bincount(comp.reshape(-1), minlength=count + 1)
    touches = np.zeros(count + 1, dtype=bool)
    touches[np.unique(comp[on_border(comp.shape)])] = True
    return sizes, touches


def slots(x, comp, count, labels=None):
    """the label slot of every component number (index 0 unused): 0 for a mask"""
    slot = np.zeros(count + 1, dtype=np.int64)
    if labels is not None:
        first = np.full(count + 1, -1, dtype=np.int64)
        flat = comp.reshape(-1)
        idx = np.flatnonzero(flat)
        first[flat[idx][::-1]] = idx[::-1]                                       # the first voxel of each component
        lab = list(labels)
        for c in range(1, count + 1):
            slot[c] = lab.index(int(np.asarray(x).reshape(-1)[first[c]]))
    return slot


def table(x, connectivity=1, labels=None):
    """int32 [L, 2]: components and the largest size per slot"""
    comp, count = label(x, connectivity, labels)
    sizes, _ = sizes_and_border(comp, count)
    slot = slots(x, comp, count, labels)
    L = 1 if labels is None else len(labels)
    out = np.zeros((L, 2), dtype=np.int32)
    for c in range(1, count + 1):
        out[slot[c], 0] += 1
        out[slot[c], 1] = max(out[slot[c], 1], sizes[c])
    return out


def keep(x, connectivity=1, labels=None, largest=False, min_size=None, border_free=False):
    """bool [*S]: the voxels of the components that pass every test asked for"""
    comp, count = label(x, connectivity, labels)
    sizes, touches = sizes_and_border(comp, count)
    ok = np.ones(count + 1, dtype=bool)
    ok[0] = False
    if largest:
        slot = slots(x, comp, count, labels)
        L = 1 if labels is None else len(labels)
        best = np.zeros(count + 1, dtype=bool)
        for l in range(L):
            s = np.where(slot == l, sizes, 0)
            s[0] = 0
            if s.max() > 0:
                best[int(np.argmax(s))] = True                                   # ties: the lowest number
        ok &= best
    if min_size is not None:
        ok &= sizes >= min_size
    if border_free:
        ok &= ~touches
    return ok[comp]


def select_ids(ids, labels, connectivity=1, fill=0, **tests):
    """the id map with the listed labels' rejected voxels set to fill"""
    ids = np.asarray(ids)
    kept = keep(ids, connectivity, labels, **tests)
    return np.where(foreground(ids, labels) & ~kept, np.asarray(fill, dtype=ids.dtype), ids)


def fill_holes(mask, connectivity=1):
    mask = np.asarray(mask) != 0
    return mask | keep(~mask, connectivity, border_free=True)


# ---- patterns ------------------------------------------------------------------------------------------------------------------------
def comb(shape):
    """a serpentine: in a slice every other row is full and the gaps are bridged at alternating ends; in 3-D every other slice holds such
    a comb and the slices between them one bridging voxel, alternately at the comb's end and at its start -- ONE component at every
    connectivity, a path whose length is a fixed fraction (about a half in 2-D, a quarter in 3-D) of the voxel count"""
    rows, n = shape[-2], shape[-1]
    m = np.zeros((rows, n), dtype=bool)
    m[0::2] = True
    for k, r in enumerate(range(1, rows, 2)):
        m[r, n - 1 if k % 2 == 0 else 0] = True
    if len(shape) == 2:
        return m
    last = (rows - 1) // 2 * 2                                                   # the last full row; the path ends at its far end
    ends = [(0, 0), (last, n - 1 if (last // 2) % 2 == 0 else 0)]
    if rows > 1 and rows % 2 == 0:                                               # (a bridge voxel hangs behind the last full row)
        ends[1] = (rows - 1, n - 1 if ((rows - 1) // 2) % 2 == 0 else 0)
    out = np.zeros(shape, dtype=bool)
    out[0::2] = m
    for k, z in enumerate(range(1, shape[0], 2)):
        out[(z,) + ends[(k + 1) % 2]] = True
    return out


def pattern(name, shape, seed=0):
    """a uint8 mask [*S]"""
    rng = np.random.default_rng(seed)
    if name == 'empty':
        m = np.zeros(shape, bool)
    elif name == 'full':
        m = np.ones(shape, bool)
    elif name == 'corners':
        m = np.zeros(shape, bool)
        m[tuple(np.ix_(*[[0, n - 1] for n in shape]))] = True
    elif name == 'checker':
        m = np.indices(shape).sum(0) % 2 == 0
    elif name == 'comb':
        m = comb(shape)
    elif name.startswith('random'):
        m = rng.random(shape) < float(name[6:])
    else:
        raise KeyError(name)
    return m.astype(np.uint8)


def two_combs(shape):
    """two combs with ids 3 and 7 interleaved along the first axis that is longer than one voxel (int32 ids; 0 elsewhere)"""
    a = comb(shape)
    ids = np.where(a, 3, 0).astype(np.int32)
    b = np.roll(a, 1, axis=len(shape) - 2) if shape[len(shape) - 2] > 1 else np.zeros(shape, bool)
    ids[b & ~a] = 7
    return ids


def random_ids(shape, nids, seed=0):
    """i.i.d. ids 0 .. nids - 1 (int32)"""
    return np.random.default_rng(seed).integers(0, nids, shape).astype(np.int32)
