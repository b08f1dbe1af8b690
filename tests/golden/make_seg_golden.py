"""
Record what the REFERENCE's own `pred_to_label`, `prob_of_label` and `recode` (neurite/tf/utils/seg.py:230-356) compute, into
tests/golden/seg_small.npz, together with the AST signatures of the functions neurite_amd.seg restates.

    python tests/golden/make_seg_golden.py PATH/TO/REFERENCE        # the directory that holds the reference's `neurite` package

TEST INFRASTRUCTURE, run once where a checkout of the reference exists; tests/test_seg_abi.py and tests/test_gpu_seg.py read only the
.npz.  The three functions run on tests/golden/tf_shim.py unchanged.  `_quilt` (seg.py:363-374) cannot be recorded: it calls pystrum's
patchlib.quilt, which is not part of the reference tree (the shim's stub for pystrum is empty); tests/seg_restatement.py restates it.

Keys are `<tag>__<field>` (conftest.golden_cases):
    am_*      x       the probability map: uint8 for the integer-valued cases (values 0 .. 3: most voxels are ties; exact in bfloat16),
                      float32 for the others (the `am_bf_*` ones hold values that bfloat16 represents exactly)
              label   pred_to_label(x)[0], int64
    pl_*      x       non-negative float32 map (`pl_bf_*`: exact in bfloat16), label: int32 labels in range
              prob    prob_of_label(x.astype(float32), label) as the reference returns it (float32)
    rc_*      seg     int32 labels, keys / values (the mapping as two arrays; `is_list` = 1: the list form, keys only), max_label
                      (absent: None)
              out     recode(seg, mapping, max_label), float32
and `__signatures__` holds the JSON {name: AST signature} (tests/golden/ast_signatures.py).
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

SIGNED = ['predict_volumes', 'predict_volume_stack', 'prob_of_label', 'pred_to_label', 'recode', '_quilt']
CHANNELS = [1, 2, 3, 4, 5, 8, 20, 32, 33, 64, 100, 256]


def bf16_exact(x):
    """float32 values with the low 16 bits cleared: bfloat16 holds them exactly"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def main(ref_root):
    sys.path.insert(0, ref_root)
    import neurite as ne
    seg = ne.utils.seg

    def asnp(y):
        return np.asarray(y.numpy() if hasattr(y, 'numpy') else y)

    out = {}
    rng = np.random.default_rng(296)

    # ---- pred_to_label
    for C in CHANNELS:                                              # ties: integer values 0 .. 3
        x = rng.integers(0, 4, size=(65, C), dtype=np.uint8)
        out['am_tie_c%d__x' % C] = x
        out['am_tie_c%d__label' % C] = asnp(seg.pred_to_label(x.astype(np.float32))[0]).astype(np.int64)
    for C in (4, 5, 32):                                            # the 5-D case of the issue: [2, 5, 6, 7, C]
        x = bf16_exact(rng.standard_normal((2, 5, 6, 7, C)))
        out['am_bf_nd_c%d__x' % C] = x
        out['am_bf_nd_c%d__label' % C] = asnp(seg.pred_to_label(x)[0]).astype(np.int64)
    for C in (3, 8, 33, 64):                                        # NaN at the first, a middle and the last channel; ties among NaNs
        x = rng.standard_normal((63, C)).astype(np.float32)
        x[0:10, 0] = np.nan
        x[10:20, C // 2] = np.nan
        x[20:30, C - 1] = np.nan
        x[30:40, C // 2] = np.nan
        x[30:40, C - 1] = np.nan                                     # two NaNs: the first wins
        x[40:45, :] = np.nan
        out['am_nan_c%d__x' % C] = x
        out['am_nan_c%d__label' % C] = asnp(seg.pred_to_label(x)[0]).astype(np.int64)
    for n, C in ((4099, 5), (65, 32)):                              # the maximum in the last channel of the last voxel
        x = rng.random((n, C), dtype=np.float32)
        x[-1, :] = 0.25
        x[-1, C - 1] = 2.0
        out['am_last_c%d__x' % C] = x
        out['am_last_c%d__label' % C] = asnp(seg.pred_to_label(x)[0]).astype(np.int64)

    # ---- prob_of_label (the reference divides float32 by a float32 row sum)
    for C in (1, 3, 4, 20, 32, 33, 256):
        for tag, conv in (('pl', lambda a: a), ('pl_bf', bf16_exact)):
            x = conv(rng.random((3, 4, 5, C), dtype=np.float32) + np.float32(0.01))
            lab = rng.integers(0, C, size=(3, 4, 5), dtype=np.int32)
            out['%s_c%d__x' % (tag, C)] = x
            out['%s_c%d__label' % (tag, C)] = lab
            p = asnp(seg.prob_of_label(x, lab))
            assert p.dtype == np.float32 and p.shape == lab.shape, (p.dtype, p.shape)
            out['%s_c%d__prob' % (tag, C)] = p

    # ---- recode
    segvol = rng.integers(0, 42, size=(9, 10, 11), dtype=np.int32)
    cases = {
        'rc_dict': (dict((int(k), int(v)) for k, v in zip(rng.permutation(42)[:30], rng.integers(1, 9, 30))), None),
        'rc_dict_max': ({0: 0, 2: 5, 7: 1, 41: 3}, 60),
        'rc_list': ([int(v) for v in rng.permutation(42)], None),
        'rc_list_max': ([int(v) for v in rng.permutation(42)[:20]], 41),
    }
    for tag, (mapping, max_label) in cases.items():
        if not isinstance(mapping, list):                           # (the lookup must cover every label of seg: np.take in the shim)
            mapping = dict(mapping)
            if max_label is None:
                mapping.setdefault(41, 2)
        elif max_label is None:
            assert max(mapping) == 41
        out[tag + '__seg'] = segvol
        out[tag + '__is_list'] = np.array(int(isinstance(mapping, list)), np.int32)
        out[tag + '__keys'] = np.array(mapping if isinstance(mapping, list) else list(mapping.keys()), np.int64)
        if not isinstance(mapping, list):
            out[tag + '__values'] = np.array(list(mapping.values()), np.int64)
        if max_label is not None:
            out[tag + '__max_label'] = np.array(max_label, np.int64)
        r = asnp(seg.recode(segvol, mapping, max_label))
        assert r.dtype == np.float32 and r.shape == segvol.shape, (r.dtype, r.shape)
        out[tag + '__out'] = r

    path_py = os.path.join(ref_root, 'neurite', 'tf', 'utils', 'seg.py')
    sigs = {name: ast_signatures.signature(path_py, name) for name in SIGNED}
    out['__signatures__'] = np.array(json.dumps(sigs, sort_keys=True))
    path = os.path.join(HERE, 'seg_small.npz')
    np.savez_compressed(path, **out)
    print('%-28s %7.1f KB  (%d arrays)' % ('seg_small.npz', os.path.getsize(path) / 1024, len(out)))


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'neurite', '__init__.py')):
        raise SystemExit('usage: python tests/golden/make_seg_golden.py PATH/TO/REFERENCE   (the directory holding the `neurite` package)')
    main(sys.argv[1])
