"""
The definition the binary morphology, the box minimum / maximum filters and the box rank filters are tested against (not a test file),
in NumPy with np.pad and sliding_window_view and no scipy, and the case lists the tests share.
tests/test_morphology_restatement_cpu.py compares this definition with scipy.ndimage; the GPU tests and the word-core test use it alone.

binary:  with o = off - 1 over the set entries of the structure, one erosion step is out[p] = AND m[p + o] and one dilation step
         out[p] = OR m[p - o], on the volume padded by one voxel of border_value; n iterations are n steps; an opening is n erosions
         then n dilations, a closing n dilations then n erosions.
filters: the volume is padded by size // 2 per axis in the boundary mode (reflect = np.pad 'symmetric', mirror = np.pad 'reflect',
         nearest = 'edge', constant = cval converted to the dtype), then the minimum, the maximum or the k-th smallest of every window.
rank:    median k = N // 2; rank_filter k = rank (negative: from the end); percentile_filter k = int(N * p / 100.0), N - 1 at p = 100,
         a negative p meaning p + 100.
"""

import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

STEPS_PER_LAUNCH = 4                                          # csrc/morph.hip: kMbSteps; K + 1 iterations take a second launch
ASYMMETRIC_3D = np.array([[[0, 1, 0], [0, 0, 1], [0, 0, 0]],
                          [[0, 0, 0], [1, 0, 0], [0, 0, 1]],
                          [[0, 0, 0], [0, 0, 0], [1, 0, 0]]], dtype=bool)      # no centre, no symmetry
ASYMMETRIC_2D = np.array([[0, 1, 1], [0, 0, 0], [1, 0, 0]], dtype=bool)
MODES = ('reflect', 'mirror', 'nearest', 'constant')
CVAL = 0.25
_PAD = {'reflect': 'symmetric', 'mirror': 'reflect', 'nearest': 'edge', 'constant': 'constant'}


# ---- binary --------------------------------------------------------------------------------------------------------------------------
def structure_of(structure, nd):
    """None, a connectivity or an array -> bool (3,) * nd"""
    if structure is None:
        structure = 1
    if isinstance(structure, (int, np.integer)):
        return np.abs(np.indices((3,) * nd) - 1).sum(0) <= int(structure)
    out = np.asarray(structure) != 0
    assert out.shape == (3,) * nd
    return out


def structure_bits(structure, nd):
    """the 27-bit form: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); a 2-D structure lies in the plane dz = 0"""
    st = structure_of(structure, nd)
    if nd == 2:
        full = np.zeros((3, 3, 3), dtype=bool)
        full[1] = st
        st = full
    return int(sum(1 << i for i, v in enumerate(st.reshape(-1)) if v))


def binary_step(m, st, dilate, border):
    """one step on one volume m (bool [*S])"""
    nd = m.ndim
    win = sliding_window_view(np.pad(m, 1, constant_values=bool(border)), (3,) * nd)        # win[p][off] = m[p + off - 1]
    if dilate:
        return win[..., st[(slice(None, None, -1),) * nd]].any(-1)                           # m[p - o]: the reflected structure
    return win[..., st].all(-1)


def binary(m, structure=None, iterations=1, border=0, stages=(0,)):
    """m bool [B, *S]; stages: 0 an erosion stage, 1 a dilation stage, each of `iterations` steps"""
    st = structure_of(structure, m.ndim - 1)
    out = []
    for vol in m:
        for dilate in stages:
            for _ in range(iterations):
                vol = binary_step(vol, st, dilate, border)
        out.append(vol)
    return np.stack(out)


STAGES = {'erosion': (0,), 'dilation': (1,), 'opening': (0, 1), 'closing': (1, 0)}


def _smooth(x):
    for ax in range(1, x.ndim):
        pad = [(0, 0)] * x.ndim
        pad[ax] = (2, 2)
        x = sliding_window_view(np.pad(x, pad, mode='edge'), 5, axis=ax).mean(-1)
    return x


@functools.lru_cache(maxsize=None)
def mask(kind, shape, seed=0):
    """bool [B, *S].  blobs: thresholded smoothed noise, a third set; points: a few single voxels; dense: all but a few voxels"""
    rng = np.random.default_rng(seed + 31 * int(np.prod(shape)) + len(shape))
    if kind == 'blobs':
        field = _smooth(rng.random(shape))
        out = field > np.quantile(field, 0.65)
    else:
        out = rng.random(shape) < max(0.002, 1.5 / np.prod(shape[1:]))
        out[(slice(None),) + tuple(s // 2 for s in shape[1:])] = True
        if kind == 'dense':
            out = ~out
    out.setflags(write=False)
    return out


def _binary_case_keys():
    """(shape [B, *S], input kind, structure, iterations, border, op)"""
    keys = []
    main, wide, thick = (1, 7, 9, 67), (1, 5, 66, 70), (1, 12, 13, 70)
    for op in ('erosion', 'dilation'):
        for border in (0, 1):
            for conn in (1, 2, 3):
                keys.append((main, 'blobs', conn, 1, border, op))
            keys.append((main, 'blobs', 'asym', 1, border, op))
            keys.append((wide, 'blobs', 'asym', 2, border, op))
            keys.append(((1, 33, 65), 'blobs', 'asym', 1, border, op))
        # last-axis extents: one voxel, a word and its edges, two full words, three with a tail of two bits, the longest row
        for shape in ((1, 6, 9, 1), (1, 3, 5, 63), (1, 3, 5, 64), (1, 3, 5, 65), (1, 3, 5, 128), (1, 3, 5, 130), (1, 2, 3, 1024), (1, 3, 130),
                      (1, 1, 2, 65), (1, 260, 5)):
            # (at these sizes an erosion needs a mostly-set mask and, where an extent is below 3, a set outside to leave anything)
            kind, border = ('dense', 1) if op == 'erosion' else ('points', 0)
            keys.append((shape, kind, len(shape) - 1, 1, border, op))
            keys.append((shape, kind, 1, 2, border, op))
            if min(shape[1:]) >= 3:
                keys.append((shape, 'dense' if op == 'erosion' else 'blobs', 1, 1, 1 - border, op))
        keys.append(((3,) + main[1:], 'blobs', 1, 2, 0, op))                   # a halo must not read the next entry
        keys.append(((3,) + main[1:], 'blobs', 3, 1, 1, op))
        keys.append((wide, 'blobs', 2, 2, 0, op))
        keys.append(((1, 33, 65), 'blobs', 1, 1, 0, op))
        keys.append(((1, 33, 65), 'blobs', 2, 2, 1, op))
        # many iterations would leave nothing of blobs: erode a mostly-set mask, dilate a few voxels
        for n in (3, STEPS_PER_LAUNCH, STEPS_PER_LAUNCH + 1):
            kind = 'dense' if op == 'erosion' else 'points'
            keys.append((thick, kind, 1, n, 1 if op == 'erosion' else 0, op))
            keys.append(((1, 40, 70), kind, 2, n, 1 if op == 'erosion' else 0, op))
        keys.append((thick, 'dense' if op == 'erosion' else 'points', 1, STEPS_PER_LAUNCH + 1, 0, op))
        keys.append((thick, 'dense' if op == 'erosion' else 'points', 'asym', 2 * STEPS_PER_LAUNCH + 1, 1 if op == 'erosion' else 0, op))
    for op in ('opening', 'closing'):
        for border in (0, 1):
            keys.append((main, 'blobs', 1, 1, border, op))
            keys.append((wide, 'blobs', 2, 2, border, op))
            keys.append(((1, 33, 65), 'blobs', 'asym', 1, border, op))
        keys.append((thick, 'dense', 1, STEPS_PER_LAUNCH + 1, 1, op) if op == 'opening' else (thick, 'points', 1, STEPS_PER_LAUNCH + 1, 0, op))
    return keys


def structure_arg(structure, nd):
    """the structure of a case key as the functions take it"""
    if isinstance(structure, str):
        return ASYMMETRIC_3D if nd == 3 else ASYMMETRIC_2D
    return structure


@functools.lru_cache(maxsize=None)
def binary_cases():
    """every binary case with its input and expected output: (key, m, want).  No expected output is constant."""
    out = []
    for key in _binary_case_keys():
        shape, kind, structure, iterations, border, op = key
        m = mask(kind, shape)
        want = binary(m, structure_arg(structure, len(shape) - 1), iterations, border, STAGES[op])
        assert 0.0 < want.mean() < 1.0, (key, float(want.mean()))
        want.setflags(write=False)
        out.append((key, m, want))
    return out


# ---- filters -------------------------------------------------------------------------------------------------------------------------
def padded(x, sizes, mode, cval=0.0):
    """x [B, *S] padded by size // 2 along every spatial axis in the boundary mode"""
    pad = [(0, 0)] + [(s // 2, s // 2) for s in sizes]
    if mode == 'constant':
        return np.pad(x, pad, mode='constant', constant_values=np.asarray(cval).astype(x.dtype))
    return np.pad(x, pad, mode=_PAD[mode])


def windows(x, sizes, mode, cval=0.0):
    """[B, *S, N]: the samples of every voxel's box"""
    win = sliding_window_view(padded(x, sizes, mode, cval), tuple(sizes), axis=tuple(range(1, x.ndim)))
    return win.reshape(x.shape + (-1,))


def minmax_filter(x, sizes, mode, cval=0.0, stages=(0,)):
    for want_max in stages:
        win = windows(x, sizes, mode, cval)
        x = win.max(-1) if want_max else win.min(-1)
    return x


def rank_of(kind, n, arg=None):
    """the order statistic of the three rank filters for a box of n samples"""
    if kind == 'median':
        return n // 2
    if kind == 'rank':
        return arg + n if arg < 0 else arg
    p = arg + 100.0 if arg < 0 else float(arg)
    return n - 1 if p == 100.0 else int(n * p / 100.0)


def rank_filter(x, k, sizes, mode, cval=0.0):
    return np.sort(windows(x, sizes, mode, cval), axis=-1)[..., k]


FILTER_SHAPES = ((1, 5, 9, 67), (1, 1, 2, 5), (1, 33, 65), (3, 5, 9, 67))                     # [B, *S]
MINMAX_SIZES = {3: (3, 5, (1, 3, 5), (3, 1, 7), (1, 1, 31), (31, 1, 1)), 2: (3, 5, (3, 5), (7, 1), (1, 31), (31, 1))}
RANK_SIZES = {3: (3, (1, 3, 3), (1, 5, 5), (3, 1, 5)), 2: (3, 5, (1, 7))}
RANK_RULES = (('median', None), ('rank', 0), ('rank', -1), ('rank', 5), ('percentile', 0), ('percentile', 10), ('percentile', 75),
              ('percentile', 100), ('percentile', -25))


def box(size, nd):
    return (size,) * nd if isinstance(size, int) else tuple(size)


@functools.lru_cache(maxsize=None)
def image(kind, shape, seed=0):
    """float: normal values with +-inf and both zeros sprinkled in; ties: the integers 0 .. 3 as float32; int: int32 in -50 .. 50"""
    rng = np.random.default_rng(seed + 17 * int(np.prod(shape)) + len(shape))
    if kind == 'int':
        out = rng.integers(-50, 51, size=shape).astype(np.int32)
    elif kind == 'ties':
        out = rng.integers(0, 4, size=shape).astype(np.float32)
    else:
        out = rng.standard_normal(shape).astype(np.float32)
        special = np.array([np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
        where = rng.random(shape) < 0.04
        out[where] = rng.choice(special, size=int(where.sum()))
    out.setflags(write=False)
    return out
