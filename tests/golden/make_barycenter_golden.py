"""
Record what the REFERENCE's own `utils.barycenter` (neurite/tf/utils/utils.py:512-573) computes, into tests/golden/barycenter_small.npz,
together with its AST signature.

    python tests/golden/make_barycenter_golden.py PATH/TO/REFERENCE        # the directory that holds the reference's `neurite` package

TEST INFRASTRUCTURE, run once where a checkout of the reference exists; tests/test_barycenter_abi.py and tests/test_gpu_barycenter.py
read only the .npz.  The function runs on tests/golden/tf_shim.py unchanged but for one thing, which is wrapped here and not in the
shim: it passes a `range` as `axis` to tf.reduce_sum.

Keys are `<tag>__<field>` (conftest.golden_cases):
    x                  the input: uint8 for the integer-valued cases (values 0 .. 3, cast to float32 / bfloat16 / float16 by the tests;
                       every product and partial sum of these is exact in float32, so the outputs pin every element being counted
                       exactly once, bit for bit), float32 for the others
    axes               the `axes` argument in the order given; absent for axes=None
    y_n<N>_s<S>        the float32 output for normalize=N, shift_center=S
and `__signature__` holds the JSON of the AST signature (tests/golden/ast_signatures.py).
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tf_shim  # noqa: E402

tf_shim.install()
import ast_signatures  # noqa: E402

# (tag, shape, axes): the integer-valued cases.  Each gets one all-zero channel (an output that must be exactly 0, not NaN).
INT_CASES = [
    ('int_c5', (2, 9, 10, 33, 5), (1, 2, 3)),
    ('int_c8', (2, 9, 10, 33, 8), (1, 2, 3)),
    ('int_c68', (3, 7, 6, 5, 68), (1, 2, 3)),
    ('int_slabs', (1, 40, 40, 40, 4), (1, 2, 3)),
    ('int_trail', (3, 31, 32, 33), (1, 2, 3)),
    ('int_2d', (2, 3, 64, 64, 7), (2, 3)),
    ('int_all', (2, 5, 6, 7, 3), None),
    ('int_perm', (2, 5, 6, 7, 3), (3, 1)),
    ('int_one', (2, 5, 6, 7, 3), (2,)),
    ('int_long', (2, 4100, 3), (1,)),            # a reduced dimension longer than the kernels' coordinate table; values 0 .. 1
]
# a single spike at the first / at the last element of R (channels 0 / 1; the other channels stay empty)
SPIKE_CASES = [('spike_c5', (2, 9, 10, 33, 5), (1, 2, 3)), ('spike_trail', (3, 31, 32, 33), (1, 2, 3))]
# float data: the six argument sets of a [2, 5, 6, 7, 3] input
FLOAT_SHAPE = (2, 5, 6, 7, 3)
FLOAT_CASES = [('f_spatial', (1, 2, 3)), ('f_all', None), ('f_perm', (3, 1)), ('f_one', (2,)), ('f_trailing', (3, 4)), ('f_first', (0,))]


def main(ref_root):
    sys.path.insert(0, ref_root)
    import tensorflow as tf
    plain_sum = tf.reduce_sum
    tf.reduce_sum = lambda x, axis=None, keepdims=False: plain_sum(x, axis=tuple(axis) if isinstance(axis, range) else axis,
                                                                   keepdims=keepdims)
    import neurite as ne

    def run(x, axes, normalize, shift):
        y = ne.utils.barycenter(tf.constant(x.astype(np.float32)), axes=axes, normalize=normalize, shift_center=shift)
        y = np.asarray(y.numpy() if hasattr(y, 'numpy') else y)
        assert y.dtype == np.float32, y.dtype
        return y

    out = {}

    def record(tag, x, axes, flag_sets):
        out[tag + '__x'] = x
        if axes is not None:
            out[tag + '__axes'] = np.array(axes, np.int32)
        for n, s in flag_sets:
            out['%s__y_n%d_s%d' % (tag, n, s)] = run(x, axes, bool(n), bool(s))

    rng = np.random.default_rng(512)
    for tag, shape, axes in INT_CASES:
        x = rng.integers(0, 2 if tag == 'int_long' else 4, size=shape, dtype=np.uint8)
        kept = [ax for ax in range(len(shape)) if axes is not None and ax not in axes]
        if kept:                                                    # the last entry of the kept axes: an all-zero channel
            idx = [slice(None)] * len(shape)
            for ax in kept:
                idx[ax] = shape[ax] - 1
            x[tuple(idx)] = 0
        record(tag, x, axes, [(0, 0), (0, 1)])
        # unshifted, every term is >= 0 and the shifted coordinates are no larger in magnitude: no partial sum in any order exceeds this
        red = tuple(range(len(shape))) if axes is None else axes
        dens = x.sum(axis=red, dtype=np.float64)
        worst = max(float((out[tag + '__y_n0_s0'][..., j].astype(np.float64) * dens).max()) for j in range(len(red)))
        assert worst < 2 ** 23, (tag, worst)
    for tag, shape, axes in SPIKE_CASES:
        x = np.zeros(shape, np.uint8)
        first = [0] * len(shape)
        last = [0] + [shape[ax] - 1 for ax in axes] + ([1] if len(shape) > 1 + len(axes) else [])
        x[tuple(first)] = 3
        if len(shape) == 1 + len(axes):                             # no channel axis: the last element in the second batch entry
            last[0] = 1
        x[tuple(last)] = 2
        record(tag, x, axes, [(0, 0), (0, 1)])
    xf = rng.random(FLOAT_SHAPE, dtype=np.float32)
    for tag, axes in FLOAT_CASES:
        record(tag, xf, axes, [(0, 0), (0, 1), (1, 0), (1, 1)])

    sig = ast_signatures.signature(os.path.join(ref_root, 'neurite', 'tf', 'utils', 'utils.py'), 'barycenter')
    out['__signature__'] = np.array(json.dumps(sig, sort_keys=True))
    path = os.path.join(HERE, 'barycenter_small.npz')
    np.savez_compressed(path, **out)
    print('%-28s %7.1f KB  (%d arrays)' % ('barycenter_small.npz', os.path.getsize(path) / 1024, len(out)))


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'neurite', '__init__.py')):
        raise SystemExit('usage: python tests/golden/make_barycenter_golden.py PATH/TO/REFERENCE   (the directory holding the `neurite` package)')
    main(sys.argv[1])
