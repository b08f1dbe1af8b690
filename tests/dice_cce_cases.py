"""
The case table of tests/test_gpu_dice_cce_arms.py, with the inputs and float64 references of every case (numpy only, so that
tests/test_dice_cce_oracle.py can check the table and its premises without a device).  An id is `<kernel instance> <what>`; the
instance is what oracle/dice_cce_oracle.py derives for every shape of the case.
"""

import collections
import zlib

import numpy as np

from oracle import dice_cce_oracle as dco

F, D = np.float32, np.float64
DTYPES = ('f32', 'bf16', 'f16')
VEC_L = (4, 8, 16, 32, 64, 128, 256, 12, 20, 36, 68, 132)        # every G with all lanes real, every G >= 4 with padded lanes
CAP_L = (4, 8, 16, 32, 64, 128, 256)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(' '.join(str(k) for k in key).encode()))


def tile(raw, V):
    """one period [B, P, ...] -> the whole map [B, V, ...]"""
    return dco.Tiled(raw, V).full()


# ------------------------------------------------------------------------------------------------------------------------------
# Dice from probability maps: nrt_dice_soft / nrt_dice_soft_f32 / nrt_sqdiff_sums_f32, nrt_dice_hard_prob / _f32 / _minmax_f32
# ------------------------------------------------------------------------------------------------------------------------------

# kind: 'soft' | 'hard'; normalize: 0 / 1 / 2 (soft), minmax: bool (hard); entry: the ABI entry point; shapes: ((V, B), ...);
# kinds: the runs ('exact', 'random'); off: byte offset of both maps from a 16-byte boundary
Case = collections.namedtuple('Case', 'id kind L dtype normalize minmax off entry shapes kinds')


def vec_unit(L):
    return 4 * (256 // dco.vec_group(L))


def vec_shapes(L):
    """through nblk = ceil(V / 4 NG): one voxel; one block; a second block of one voxel; 63 blocks with a partial last one, 64, 65 (the
    group edge of reduce_rows); 513 (9 groups: a partial second round of the finalize) -- each at batch 1 and 3"""
    u = vec_unit(L)
    return tuple((V, B) for V in (1, u, u + 1, 63 * u - 1, 64 * u, 64 * u + 1, 512 * u + 1) for B in (1, 3))


def cap_V(L):
    return 2048 * vec_unit(L) + 1


def _soft_instance(L, dtype, normalize, off=0):
    return dco.plan_soft(L, 1, 1, normalize, dtype, off)['instance']


def _hard_instance(L, dtype, minmax, off=0):
    return dco.plan_hard_prob(L, 1, 1, minmax, dtype, off)['instance']


def generic_soft_shapes(L):
    """one voxel; one pass of one block (R voxels); one more; two row groups; more voxels than the capped grid covers in one pass"""
    R, gz = 256 // min(L, 256), dco.cdiv(L, 256)
    return ((1, 1), (R, 3), (R + 1, 1), (64 * R + 1, 3), ((2048 // gz) * R + 2 * R + 1, 2))


def _soft_cases():
    out = []
    for L in VEC_L:
        for dt in DTYPES:
            for nz in (0, 1):
                out.append(Case('%s L%d' % (_soft_instance(L, dt, nz), L), 'soft', L, dt, nz, True, 0, 'nrt_dice_soft', vec_shapes(L), ('exact', 'random')))
    for L in CAP_L:                                              # the 2048-block cap: blocks with an empty range
        out.append(Case('%s L%d cap' % (_soft_instance(L, 'f32', 0), L), 'soft', L, 'f32', 0, True, 0, 'nrt_dice_soft', ((cap_V(L), 1),), ('exact',)))
    for L in (1, 3, 5, 100, 255, 257, 600):
        for dt in (DTYPES if L in (5, 257) else ('f32',)):
            off = 4 if dco.vec_labels(L) else 0                  # 100 = 4 x 25 is a vector count: the generic kernel takes it 4 bytes off
            for nz in (0, 1):
                out.append(Case('%s L%d%s' % (_soft_instance(L, dt, nz, off), L, ' maps 4 bytes off' if off else ''), 'soft', L, dt, nz, True, off,
                                'nrt_dice_soft_f32' if dt == 'f32' else 'nrt_dice_soft', generic_soft_shapes(L), ('exact', 'random')))
    out.append(Case('%s L4096 (workspace 201 MB)' % _soft_instance(4096, 'f32', 0), 'soft', 4096, 'f32', 0, True, 0, 'nrt_dice_soft_f32', ((5, 1),),
                    ('exact', 'random')))
    # a vectorisable label count on maps that are not aligned to four labels: the generic kernel; 8 bytes off in 16 bits: still vector
    for dt, off in (('f32', 4), ('bf16', 2), ('bf16', 4), ('f16', 2), ('f16', 4), ('bf16', 8), ('f16', 8)):
        for nz in (0, 1):
            out.append(Case('%s L32 maps %d bytes off' % (_soft_instance(32, dt, nz, off), off), 'soft', 32, dt, nz, True, off, 'nrt_dice_soft',
                            ((1, 1), (33, 3), (64 * 8 + 1, 2)), ('exact', 'random')))
    # nrt_sqdiff_sums_f32: the `diff` arm of the plain kernels
    for L in (4, 20, 256, 5, 257):
        shapes = ((vec_unit(L) + 1, 3), (64 * vec_unit(L) + 1, 1)) if dco.vec_labels(L) else generic_soft_shapes(L)[1:4]
        out.append(Case('%s L%d sqdiff' % (_soft_instance(L, 'f32', 2), L), 'soft', L, 'f32', 2, False, 0, 'nrt_sqdiff_sums_f32', shapes, ('exact', 'random')))
    return out


def _hard_cases():
    out = []
    for L in VEC_L:
        for dt in DTYPES:
            for mm in (False, True):
                out.append(Case('%s L%d' % (_hard_instance(L, dt, mm), L), 'hard', L, dt, 0, mm, 0, 'nrt_dice_hard_prob', vec_shapes(L), ('exact',)))
    for L in CAP_L:
        out.append(Case('%s L%d cap' % (_hard_instance(L, 'f32', False), L), 'hard', L, 'f32', 0, False, 0, 'nrt_dice_hard_prob_f32', ((cap_V(L), 1),), ('exact',)))
    # dice_hard_prob_generic: the widest row of every rung of the VP ladder (a partial last chunk; in float32 also a second grid-stride
    # pass, V > 1024 VP), and a few narrow rows
    for VP, L in sorted(dco.hard_prob_rungs().items(), reverse=True):
        for dt in DTYPES:
            shapes = ((2 * VP + 131, 2),) + (((1024 * VP + VP + 3, 1),) if dt == 'f32' else ())
            out.append(Case('%s L%d VP%d' % (_hard_instance(L, dt, False), L, VP), 'hard', L, dt, 0, False, 0,
                            'nrt_dice_hard_prob_f32' if dt == 'f32' else 'nrt_dice_hard_prob', shapes, ('exact',)))
    for L in (1, 3, 5):
        out.append(Case('%s L%d VP256' % (_hard_instance(L, 'f32', False), L), 'hard', L, 'f32', 0, False, 0, 'nrt_dice_hard_prob_f32',
                        ((1, 1), (256, 2), (257, 3)), ('exact',)))
    for dt, off in (('f32', 4), ('bf16', 2), ('f16', 4), ('bf16', 8), ('f16', 8)):
        out.append(Case('%s L32 maps %d bytes off' % (_hard_instance(32, dt, False, off), off), 'hard', 32, dt, 0, False, off, 'nrt_dice_hard_prob',
                        ((1, 1), (300, 2)), ('exact',)))
    # dice_hard_prob_direct: rows too wide for LDS (1117 labels is the last rung of the ladder)
    for L in (1118, 2000):
        for dt in DTYPES:
            out.append(Case('%s L%d' % (_hard_instance(L, dt, False), L), 'hard', L, dt, 0, False, 0, 'nrt_dice_hard_prob', ((1, 1), (300, 2)), ('exact',)))
    return out


SOFT, HARD = _soft_cases(), _hard_cases()


def case_plan(c, V, B):
    return dco.plan_soft(c.L, V, B, c.normalize, c.dtype, c.off) if c.kind == 'soft' else dco.plan_hard_prob(c.L, V, B, c.minmax, c.dtype, c.off)


def zero_label(c, V):
    """the one-block shape of a case has a label that is 0 in both maps (denominator 0: divide_no_nan)"""
    return c.L - 1 if c.L > 1 and len(c.shapes) > 1 and V == c.shapes[1][0] and c.normalize != 2 else None


def build(c, V, B, kind):
    """(one period of y_true and y_pred in the storage type [B, P, L], the reference)"""
    rng = rng_for(c.id, V, B, kind)
    if c.kind == 'soft':
        t, p = dco.draw_soft(rng, B, V, c.L, kind, c.normalize, zero_label(c, V), small=9 * V >= 2 ** 24)
    else:
        t, p, spikes = dco.draw_hard(rng, B, V, c.L)
    (traw, tw), (praw, pw) = dco.store(t, c.dtype), dco.store(p, c.dtype)
    if kind == 'exact':
        assert np.array_equal(tw, t.astype(D)) and np.array_equal(pw, p.astype(D))         # the storage type holds the draw exactly
    if c.kind == 'soft':
        return traw, praw, dco.soft_ref(tw, pw, V, c.normalize)
    r = dco.hard_ref(tw, pw, V, spikes)
    r['spikes'] = spikes
    return traw, praw, r


def whole_maps(c, traw, praw, r, V):
    """the two maps [B, V, L] in the storage type: the period tiled, then the spikes of a hard case (one voxel and label each)"""
    full = [tile(traw, V), tile(praw, V)]
    for k, b, v, l, val in r.get('spikes', ()):
        raw, wide = dco.store(np.array([val], F), c.dtype)
        assert wide[0] == val
        full[k][b, v, l] = raw[0]
    return full


# ------------------------------------------------------------------------------------------------------------------------------
# hard Dice from integer label maps: nrt_dice_hard_label_i32
# ------------------------------------------------------------------------------------------------------------------------------

LabelCase = collections.namedtuple('LabelCase', 'id L workspace shapes')


def _label_cases():
    def mk(L, ws, shapes, what=''):
        inst = {dco.plan_hard_label(L, V, B, ws)['instance'] for V, B in shapes}
        assert len(inst) == 1, (L, shapes, inst)
        return LabelCase('%s L%d%s' % (inst.pop(), L, what), L, ws, shapes)
    out = [mk(L, True, ((65536, 1), (65537, 2)), ' V65536, V65537 x 2 (the second entry unaligned: scalar loop)') for L in (1, 8, 40)]
    # the grid is min(ceil(V / 2048), 512 / B) blocks of 256 lanes; the four-in-flight loop runs where a lane's first quad index
    # + 3 grid strides is still inside V / 4: B = 3 -> 170 blocks, 4 x 43520 quads per round
    out.append(mk(8, True, ((700323, 3), (700324, 3)), ' four quads in flight and a tail'))
    out.append(mk(41, True, ((65541, 2),)))
    out.append(mk(8, True, ((65535, 1),), ' V65535'))
    out.append(mk(41, True, ((512 * 2048 + 2049, 1),), ' past the 512-block cap'))
    out.append(mk(5461, False, ((5000, 2),), ' no workspace, LDS histogram of 65532 bytes'))
    out.append(mk(5462, False, ((5000, 2),), ' no workspace, global atomics'))
    out.append(mk(8, False, ((70001, 2),), ' no workspace'))
    return out


LABEL = _label_cases()


def build_labels(c, V, B):
    rng = rng_for(c.id, V, B)
    t, p = rng.integers(-2, c.L + 3, (B, V)).astype(np.int32), rng.integers(-2, c.L + 3, (B, V)).astype(np.int32)
    same = rng.random((B, V)) < 0.5                              # half the voxels agree
    p[same] = t[same]
    return t, p, dco.label_ref(t, p, c.L)


# ------------------------------------------------------------------------------------------------------------------------------
# second stage on its own: nrt_dice_from_sums_f32, nrt_dice_mean_pair_f32, nrt_dice_mean_f32
# ------------------------------------------------------------------------------------------------------------------------------

MEAN = ((1, 1), (85, 3), (128, 2), (257, 1), (250, 4))         # (L, B): n = 1, 255, 256, 257, 1000


def build_mean(L, B):
    """dice values that are multiples of 2^-10 in [0, 1] and integer weights 0 .. 7: every product and the float64 sum are exact"""
    rng = rng_for('mean', L, B)
    dice = (rng.integers(0, 1025, (B, L)) / 1024.0).astype(F)
    return dice, rng.integers(0, 8, (L,)).astype(F), rng.integers(0, 8, (B, L)).astype(F)


# ------------------------------------------------------------------------------------------------------------------------------
# weighted categorical cross-entropy: nrt_wcce, nrt_wcce_mean
# ------------------------------------------------------------------------------------------------------------------------------

CceCase = collections.namedtuple('CceCase', 'id C dtype logits per_voxel off sizes')
COMBOS = tuple((w, s) for w in (False, True) for s in (0.0, 0.2))          # with / without label weights x label_smoothing


def cce_vec_sizes(C):
    """one voxel; one block; one block and a voxel; grids of exactly 7, 8, 9 and 17 blocks (the ticket's class edges), the last block
    with one voxel"""
    u = vec_unit(C)
    return (1, u, u + 1) + tuple((g - 1) * u + 1 for g in (7, 8, 9, 17))


def cce_generic_sizes(C):
    VP = dco.cce_vp(C)
    per = VP or 256
    sizes = (1, per, per + 1, 8 * per + 1)
    return sizes + ((2048 * 8 + 9,) if C == 385 else ())                       # VP = 8: a second grid-stride pass


def _cce_cases():
    out = []
    for C in VEC_L:
        for dt in ('f32', 'bf16'):
            for lg in (False, True):
                for pv in (False, True):
                    out.append(CceCase('%s C%d' % (dco.plan_cce(C, 1, dt, lg, pv)['instance'], C), C, dt, lg, pv, 0, cce_vec_sizes(C)))
    for C in (4, 256):                                                         # past the 2048-block cap: blocks with an empty range
        out.append(CceCase('%s C%d cap' % (dco.plan_cce(C, 1, 'f32', False, True)['instance'], C), C, 'f32', False, True, 0, (2048 * vec_unit(C) + 1,)))
    for C in (1, 2, 3, 24, 25, 49, 97, 193, 385, 768, 769):
        for dt in ('f32', 'bf16'):
            for lg in (False, True):
                off = (4 if dt == 'f32' else 8) if dco.vec_labels(C) else 0         # a vectorisable count on maps not 16-byte aligned
                out.append(CceCase('%s C%d VP%d%s' % (dco.plan_cce(C, 1, dt, lg, True, off)['instance'], C, dco.cce_vp(C), ' maps %d bytes off' % off if off else ''),
                                   C, dt, lg, True, off, cce_generic_sizes(C)))
    return out


CCE = _cce_cases()
TICKET_GRIDS = (2048, 1, 9, 8, 7, 2048)
TICKET_C = 4


def build_cce(c):
    """one period of both maps at the largest size of the case, in the storage type, and {(weights, smoothing): reference of the period};
    probabilities hold exact zeros (the clip is taken), every row has a positive entry; y_true is half zeros; weights 0.5 .. 1.5"""
    rng = rng_for(c.id)
    P = dco.period(max(c.sizes))
    t = rng.random((1, P, c.C)) * (rng.random((1, P, c.C)) < 0.5)
    if c.logits:
        p = 3.0 * rng.standard_normal((1, P, c.C))
    else:
        p = rng.random((1, P, c.C)) * (rng.random((1, P, c.C)) < 0.85)
        p[..., 0] = np.maximum(p[..., 0], 0.01)
    (traw, tw), (praw, pw) = dco.store(t.astype(F), c.dtype), dco.store(p.astype(F), c.dtype)
    w = np.linspace(0.5, 1.5, c.C).astype(F)
    refs = {(hw, s): dco.cce_ref(tw[0], pw[0], w if hw else None, s, c.logits) for hw, s in COMBOS}
    return traw, praw, w, refs


def tiled_prefix(x, n):
    """the first n voxels of per-voxel values [P] repeated with period P"""
    return np.concatenate([x] * dco.cdiv(n, x.shape[0]))[:n] if n else x[:0]
