"""
The project's definition of a percentile of image intensities, written down on np.sort; the case generators the CPU and
GPU tests share; and the percentile_norm expression in NumPy float32.  NumPy only.

For a population of n >= 1 values sorted ascending as s (NaN last, -0.0 == +0.0) and a fraction f (q / 100 in float64):
    pos = (n - 1) f in float64,  a = s[floor(pos)],  b = s[ceil(pos)],  t = pos - floor(pos)
    lower = a, higher = b, midpoint = float32((a64 + b64) / 2),
    linear = float32(a64 + (b64 - a64) t) if t < 0.5 else float32(b64 - (b64 - a64)(1 - t))
That is NumPy's formula: tests/test_percentile_abi.py checks that it equals np.percentile / np.nanpercentile of the float64 copy bit
for bit.  (On a float32 array NumPy 2 forms pos in float32, which loses the fractional rank above 2^24 elements: the comparison is
against the float64 copy on purpose.)  Without ignore_nan a NaN in the population makes every result NaN; with it the NaNs leave the
population.  An empty population gives NaN.  +-inf are ordinary values; inf - inf in the interpolation gives NaN, as in NumPy.
Results are compared by value with equal NaN positions (np.array_equal(..., equal_nan=True)): the sign of a zero is not compared.
"""

import numpy as np

METHODS = ('linear', 'lower', 'higher', 'midpoint')
QS = (0, 100, 50, 99, 0.5, 99.5, 33.3)                                             # the percentiles of the tests
Q8 = (0, 100, 50, 99, 0.5, 99.5, 33.3, 50)                                         # all 8 at once, with a duplicate
SIZES = (1, 2, 3, 63, 64, 65, 101, 4099)                                            # 1-D; 101 with q = 50: pos an exact integer
SHAPES = ((3, 37, 41), (41, 43, 41))                                                # 4551 and 72283 elements
DISTRIBUTIONS = ('normal', 'ties', 'last_pass', 'one_bin', 'negative', 'mixed_zeros', 'constant', 'zeros70', 'inf', 'denormal')


def population(x, mask=None, ignore_nan=False):
    """the values a percentile of x is taken over, float32, sorted ascending with NaN last"""
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    if mask is not None:
        v = v[np.asarray(mask).reshape(-1) != 0]
    if ignore_nan:
        v = v[~np.isnan(v)]
    return np.sort(v)


def ranks(n, f):
    """(floor(pos), ceil(pos), t) of fraction f in a population of n >= 1"""
    pos = np.float64(n - 1) * np.float64(f)
    lo = np.floor(pos)
    return int(lo), int(np.ceil(pos)), pos - lo


def from_sorted(s, f, method='linear'):
    """the definition on a sorted population s (float32, NaN last) -> (value, a, b) as float32 scalars"""
    nan = np.float32(np.nan)
    n = s.size
    if n == 0 or np.isnan(s[-1]):
        return nan, nan, nan
    lo, hi, t = ranks(n, f)
    a, b = s[lo], s[hi]
    a64, b64 = np.float64(a), np.float64(b)
    with np.errstate(invalid='ignore', over='ignore'):
        if method == 'lower':
            v = a
        elif method == 'higher':
            v = b
        elif method == 'midpoint':
            v = np.float32((a64 + b64) / 2.0)
        elif method == 'linear':
            v = np.float32(a64 + (b64 - a64) * t) if t < 0.5 else np.float32(b64 - (b64 - a64) * (1.0 - t))
        else:
            raise ValueError(method)
    return np.float32(v), np.float32(a), np.float32(b)


def percentile(x, q, mask=None, method='linear', ignore_nan=False):
    """the percentiles q (a sequence, in [0, 100]) of one entry -> (values, lower, upper: float32 [Q]; the population count)"""
    s = population(x, mask, ignore_nan)
    rows = [from_sorted(s, np.float64(v) / 100.0, method) for v in q]
    return tuple(np.array([r[k] for r in rows], np.float32) for k in range(3)) + (int(s.size),)


def rescale_clip(x, lo, hi, clip=True, out_range=(0, 1)):
    """percentile_norm's expression on given bounds, every operation rounded to float32 once"""
    x = np.asarray(x).astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        y = (x - lo) / (hi - lo)
        if hi == lo:
            y = np.zeros_like(x)
        if clip:
            y = np.where(y < 0, np.float32(0), np.where(y > 1, np.float32(1), y))              # (a NaN stays)
        if tuple(out_range) != (0, 1):
            a, b = np.float32(out_range[0]), np.float32(out_range[1])
            y = a + y * (b - a)
        if np.isnan(lo) or np.isnan(hi):
            y = np.full_like(x, np.nan)
    return y.astype(np.float32)


def draw(name, n, seed=0):
    """n float32 values of a named distribution"""
    rng = np.random.default_rng([seed, n, DISTRIBUTIONS.index(name) if name in DISTRIBUTIONS else 99])
    if name == 'normal':
        v = rng.standard_normal(n)
    elif name == 'ties':                                                            # integers 0 .. 7
        v = rng.integers(0, 8, n)
    elif name == 'last_pass':                                                       # 1 + k 2^-23, k < 1024: the last digit decides
        v = 1.0 + rng.integers(0, 1024, n).astype(np.float64) * 2.0 ** -23
    elif name == 'one_bin':                                                         # [1, 2): one bin of the first pass
        v = 1.0 + rng.random(n)
    elif name == 'negative':
        v = -np.abs(rng.standard_normal(n)) - 0.25
    elif name == 'mixed_zeros':
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.2] = 0.0
        v[rng.random(n) < 0.2] = -0.0
    elif name == 'constant':
        v = np.full(n, 3.25)
    elif name == 'zeros70':                                                         # 70 % exact zeros with a positive tail
        v = np.where(rng.random(n) < 0.7, 0.0, rng.gamma(2.0, 50.0, n))
    elif name == 'inf':
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.1] = np.inf
        v[rng.random(n) < 0.1] = -np.inf
    elif name == 'denormal':
        v = rng.standard_normal(n) * 1e-41
        v[::3] *= 1e3
    elif name == 'nan':
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.15] = np.nan
        v = v.astype(np.float32)
        if n > 1:
            v[n // 2] = np.float32(np.nan)
            v.view(np.uint32)[0] = 0xFFC00001                                       # a NaN with the sign bit set
        return v
    else:
        raise ValueError(name)
    return np.asarray(v).astype(np.float32)


def store(v, dtype):
    """float32 values as they come back from storage in `dtype` ('float32', 'bfloat16', 'float16'): (stored array for torch, float32)"""
    if dtype == 'float32':
        return v, v
    if dtype == 'float16':
        with np.errstate(over='ignore'):
            h = v.astype(np.float16)
        return h, h.astype(np.float32)
    bits = v.view(np.uint32)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)        # round to nearest even
    rounded = np.where(np.isnan(v), np.uint16(0x7FC0), rounded)
    return rounded, (rounded.astype(np.uint32) << 16).view(np.float32)
