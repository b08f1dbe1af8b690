"""
The table of cases of tests/test_gpu_warp_dice_arms.py (every dispatch arm of the fused warp + soft Dice forward, csrc/fused.hip and
csrc/fused_wc.h), their inputs and their references.  numpy only: tests/test_warp_dice_oracle.py checks the table and the premises of
the data without a device.

An id is `<instance> L<labels> B<batch> O<output shape> <geometry> [note]`: the instance and the geometry are what
oracle.warp_dice_oracle.plan derives for the call at 256 compute units (the x-march schedules depend on the count; the GPU file derives
them again for the device it runs on and asserts the same instance).

How a shape follows from its condition (NG = 256 / G lane groups per block, WZ = 64 / G of them in a wave):

  tile schedule      tile_geometry raises ltz to log2 WZ and lty until a tile holds NG voxels.  Default word: 8 x 8 x max(16, WZ) voxels,
                     npass = 16 (G = 1) .. 256 (G = 64), all beyond FUSED_SYNC = 8.  `one`: the smallest legal tile, exactly NG voxels,
                     one pass (odd: the second half-turn of the two-deep pipeline is dead), z_outer = 1.  `few`: 2 NG voxels, two passes.
                     Every output extent is the smallest odd o > tile extent with o - 1 no power of two (LINSPACE: O = 2 S - 1 has to
                     be odd, and a step (S - 1) / (O - 1) can only be non-dyadic if O - 1 is no power of two), so every side has a
                     partial tile wherever the tile extent exceeds 1; tiles in the (x, y) plane are never a multiple of 8, so some XCD
                     slab has idle tiles (t2 >= nT2).
  plane_major        G = 8 only: a pass is one z-plane of a 4 x 8 patch, npass = the z-chunk: 5 (odd) on 13 planes (chunks 5, 5, 3).
  2048-block cap     G = 64: tiles of 1 x 1 x 4 voxels, O = 13 x 29 x 22 -> 8 x 48 x 6 = 2304 tiles, blocks 0 .. 31 of an XCD walk two;
                     G = 16: 2 x 2 x 4, O = 27 x 45 x 28 -> 8 x 41 x 7 = 2296.
  x-march, equal     patches of 4 x max(8, WZ) voxels (G <= 8: one x-plane per pass, npass = the piece's planes: 7 and 3, 3, 1 are odd;
                     G = 16, 32, 64: 2, 4, 8 passes per plane), O[0] = 7 or 13 < 16; 3 pieces of 7 planes -> 3, 3, 1; 5 of 13 -> 3, 3, 3, 3, 1;
                     9 asked of 7 planes -> clamped to 7; regions of 2 x 2 and 2 x 1 patches over 3 x 2 patches -> padding columns.
                     A word that asks for a patch of fewer than NG voxels (1 x 8 or 2 x 8 at G = 1, 4, 8, 16) is widened along y by
                     fused_geom (`(widened)` in the id): pieces of 7 and of 3, 3, 1 planes, odd, so an unwidened patch loses planes.
  x-march, mixed     slots = 2 CUs / 8 = 64 columns per XCD and round.  Fewer than 64 columns per XCD: het_full = 0, every column in
                     P pieces (18 columns, 13 planes -> 8 pieces of 2, the eighth starts behind the volume: an empty piece).  cols = 528
                     = 33 entries x 16: cpx = 66 = 64 whole + 2 split into 5: the split columns 64, 65 (mod 66) fall into some entries
                     and not into others -> padding rows.  525 = 25 x 21: the last XCD's list is 3 columns short.  Default word
                     (tune 0) needs xmarch_applies: O[0] >= 16 and >= 512 columns: 8 x (16 x 32 x 64) = 512 columns = 64 per XCD ->
                     het_full = 0, one piece; 9 entries -> cpx 72 = 64 + 8 split into 8, entry 0 owns none of them.
  wave cache         32 float32 labels on 4 x 8 patches.  Persistent when 8 items_x > 2 CUs = 512: 5 x (7 x 51 x 63) = 5 x 104 columns
                     = 520 -> items_x = 65 (equal pieces, one per column) or 64 + 1 x 6 = 70 (mixed); 4 x 129 = 516 columns: the last
                     list has 4 empty items, its blocks go on to other lists early.

Data.  `exact`: maps of integers 0 .. 3 (0 .. 1 above 6500 voxels per entry: the premise assert_exact is checked on every reference),
locations on a lattice around the grid that maps the output onto the source: displacements from {-1, -.5, 0, .5, 1}, the axis
(voxel index mod 3) on a quarter step, 30 % of the voxels pushed outside along one axis; with a fill value the fill is 0.5.  Each map's
extrema are spikes in one voxel and label of the launch: the moving map's sit at interior source voxels which one output voxel samples
with weight 1 (every other voxel has a quarter-step axis and samples it with 0.75 at most; a clamped voxel only reaches border rows).
In the run without fill one label is zero in both maps (the zero denominator of `dice`).  LINSPACE has no field: S = (O + 1) / 2, every
step 1/2, and it never leaves the volume -- the only family that cannot meet the 0.15 - 0.75 share outside, by construction of the
mode.  `smooth`, `incoherent`, `lattice` (oracle.warp_fwd_oracle.make_field) and `grid` (LINSPACE with S = O + 1 or O + 3: a step
whose multiples do not repeat within O - 1 voxels): uniform [0, 1) maps rounded to the storage type.

The wave cache has three regimes per wave and pass: no orphan reference (every row served from its slot), 1 .. 16 orphans (overflow
rows) and more than 16 (the pass forgets the cache).  oracle.warp_dice_oracle.wc_orphans counts them from the locations;
tests/test_warp_dice_oracle.py asserts that every wave-cache id with per-voxel locations meets all three.  A regular grid with a step
near 1 meets only the first, so the small LINSPACE ids also run `coarse`: steps of 4 + 1 / (O - 1) along y and 5 + 1 / (O - 1) along z.
"""

import dataclasses
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from oracle import np_oracle as npo
from oracle import warp_dice_oracle as wdo
from oracle import warp_fwd_oracle as wfo
from oracle.warp_dice_oracle import ABSOLUTE, LINSPACE, SHIFT, Call, tune_word

F, D = np.float32, np.float64
CUS = 256
FILL_EXACT, FILL_RANDOM = 0.5, -7.5
NO_WC, WC = wdo.TUNE_NO_WC, wdo.TUNE_WC
Case = namedtuple('Case', 'id call kinds')
GS = (1, 2, 4, 8, 16, 32, 64)
PAD_L = {4: 12, 8: 20, 16: 36, 32: 68, 64: 132}
RANDOM_KINDS = ('smooth', 'incoherent', 'lattice')


def odd_above(e):
    """the smallest odd o > e with o - 1 no power of two and, where the extent allows, a partial tile"""
    o = e + 1
    while o % 2 == 0 or (o - 1) & (o - 2) == 0 or (e > 1 and o % e == 0):
        o += 1
    return o


def source_shape(c):
    """the exact run's source: a little smaller than the output and at least 6 per axis (an incoherent field on fewer leaves the volume
    on over 75 % of the voxels); LINSPACE: O = 2 S - 1"""
    if c.mode == LINSPACE:
        return tuple((o + 1) // 2 for o in c.O)
    return c.S


def default_S(O):
    return tuple(max(6, o - (1, 2, 0)[d]) for d, o in enumerate(O))


def grid_shape(O):
    """LINSPACE, random run: S - 1 = O or O + 2 over O - 1, coprime, so the step's multiples do not repeat within O - 1 voxels"""
    return tuple(o + 1 if math.gcd(o, o - 1) == 1 and (o - 1) & (o - 2) else o + 3 for o in O)


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------

def tile_word(G, variant):
    """the tune word of a tile-schedule variant and its tile extents"""
    NG, WZ = 256 // G, 64 // G
    if variant == 'default':
        return 0, (8, 8, max(16, WZ))
    lz = max(2, int(math.log2(WZ)))                     # z extent: a wave's run, at least 4
    rest = max(NG // (1 << lz), 1)                      # (x, y) voxels of a one-pass tile
    ly = int(math.log2(rest)) // 2
    lx = int(math.log2(rest)) - ly
    if (1 << (lx + ly + lz)) < NG:
        ly += 1
    if variant == 'few':
        ly += 1
    return tune_word(lx, ly, lz, z_outer=1 if variant == 'one' else 0), (1 << lx, 1 << ly, 1 << lz)


def xm_word(variant):
    """the tune word of an x-march variant (4 x 8 patches; tile_geometry widens z to a wave's run), O[0] and O[1]"""
    nseg, lry, lrz, O0, O1, lty = {'x1': (1, 0, 0, 7, 7, 2), 'x3': (3, 1, 1, 7, 11, 2), 'x5': (5, 1, 0, 13, 11, 2), 'clamp': (9, 0, 1, 7, 11, 2),
                                   'p8x8': (2, 0, 0, 7, 11, 3), 'mixed': (0, 0, 0, 13, 11, 2)}[variant]
    return tune_word(3, lty, 3, x_march=1, nseg=nseg, lry=lry, lrz=lrz), O0, O1


def _id(c, note=''):
    p = wdo.plan(c, CUS)
    assert 'instance' in p, (c, p)
    return '%s L%d B%d O%s %s%s' % (p['instance'], c.L, c.B, 'x'.join(map(str, c.O)), wdo.tags(p), ' ' + note if note else '')


def _case(cases, c, kinds, note=''):
    if c.mode == LINSPACE:
        kinds = tuple(dict.fromkeys('grid' if k in RANDOM_KINDS else k for k in kinds))
        if c.entry == 'dice' and wdo.plan(c, CUS)['wc'] and c.B * c.nout < 20000:
            kinds += ('coarse',)
    cases.append(Case(_id(c, note), c, kinds))


def _call(L, O, **kw):
    return Call(L, kw.pop('S', None) or default_S(O), tuple(O), **kw)


def build_table():
    cases = []
    n = 0
    # ---- every reachable warp_dice_tile / warp_dice_tile_pad instance: G x mode x STORE x schedule x storage type
    for G in GS:
        WZ = 64 // G
        for L in (4 * G,) + ((PAD_L[G],) if G in PAD_L else ()):
            for mode in (ABSOLUTE, SHIFT, LINSPACE):
                for dtype, store in (('f32', False), ('f32', True), ('bf16', False)):
                    k = mode + store + 2 * (dtype == 'bf16')
                    variant = ('default', 'one', 'few')[k % 3]
                    tune, ext = tile_word(G, variant)
                    O = tuple(odd_above(e) for e in ext)
                    _case(cases, _call(L, O, B=2, mode=mode, dtype=dtype, store=store, tune=tune), ('exact', RANDOM_KINDS[n % 3]), variant)
                    xv = ('x1', 'x3', 'x5')[k % 3]
                    tune, O0, O1 = xm_word(xv)
                    O = (O0, O1, odd_above(max(8, WZ)))
                    _case(cases, _call(L, O, B=2, mode=mode, dtype=dtype, store=store, tune=tune | NO_WC), ('exact', RANDOM_KINDS[(n + 1) % 3]), xv)
                    n += 1
    # ---- one more padded count per G where it differs: other live-lane counts Gr
    for L in (24, 28, 252):
        G = wdo.fused_group(L)
        for store in (False, True):
            tune, ext = tile_word(G, 'one')
            _case(cases, _call(L, tuple(odd_above(e) for e in ext), B=2, store=store, tune=tune), ('exact', 'lattice'), 'one')
            tune, O0, O1 = xm_word('x3')
            _case(cases, _call(L, (O0, O1, 11), B=2, store=store, tune=tune), ('exact', 'smooth'), 'x3')
    # ---- tile schedule: what the table above leaves
    for tz in (5, 4):
        _case(cases, _call(32, (7, 11, 13), B=2, tune=tune_word(plane_major=1, zchunk=tz)), ('exact', 'smooth'), 'z-chunk %d of 13 planes' % tz)
    _case(cases, _call(32, (7, 11, 13), B=2, store=True, tune=tune_word(plane_major=1, zchunk=5)), ('exact', 'incoherent'), 'z-chunk 5 of 13 planes')
    _case(cases, _call(16, (7, 7, 19), B=2, tune=tune_word(2, 2, 4, plane_major=1, zchunk=5)), ('exact', 'smooth'), 'plane_major asked for and ignored')
    _case(cases, _call(256, (13, 29, 22), tune=tune_word(0, 0, 2)), ('exact', 'smooth'), 'cap')
    _case(cases, _call(256, (13, 29, 22), B=2, store=True, tune=tune_word(0, 0, 2, z_outer=1)), ('exact', 'lattice'), 'cap')
    _case(cases, _call(64, (27, 45, 28), tune=tune_word(1, 1, 2)), ('exact', 'incoherent'), 'cap')
    for B, shared in ((1, False), (3, False), (3, True)):
        tune, ext = tile_word(4, 'few')
        _case(cases, _call(16, tuple(odd_above(e) for e in ext), B=B, shared_loc=shared, store=True, tune=tune), ('exact', 'smooth'), 'few' + ' loc_batch_stride 0' * shared)
        tune, O0, O1 = xm_word('x3')
        _case(cases, _call(16, (O0, O1, 19), B=B, shared_loc=shared, tune=tune), ('exact', 'lattice'), 'x3' + ' loc_batch_stride 0' * shared)
    _case(cases, _call(16, (7, 7, 19), B=2, minmax=False, tune=tile_word(4, 'few')[0] | WC), ('exact', 'smooth'), 'no extrema asked for, tune bit 29 ignored')
    # ---- x-march, equal pieces: the segment count clamped by O[0], 8 x 8 patches
    for G in (4, 8, 32):
        for xv in ('clamp', 'p8x8'):
            tune, O0, O1 = xm_word(xv)
            _case(cases, _call(4 * G, (O0, O1, odd_above(max(8, 64 // G))), B=2, tune=tune | NO_WC), ('exact', 'smooth'), xv)
    _case(cases, _call(20, (7, 11, 11), B=2, store=True, tune=xm_word('p8x8')[0]), ('exact', 'incoherent'), 'p8x8')
    # ---- x-march words whose (y,z) patch holds fewer voxels than a pass (2^(lty + ltz) < 256 / G): fused_geom widens the patch along y.
    # ---- Unwidened, npass = xlen patch / NG rounds down and the last planes of an odd piece are neither warped nor summed
    for L, dtype, lty, nowc in ((32, 'f32', 1, NO_WC), (32, 'f32', 1, 0), (32, 'bf16', 0, 0), (4, 'f32', 0, 0), (4, 'bf16', 1, 0), (12, 'f32', 1, 0),
                                (64, 'f32', 0, 0), (20, 'f32', 0, 0)):
        for nseg, store in ((1, dtype == 'f32'), (3, False)):
            O = (7, 7, odd_above(max(8, 64 // wdo.fused_group(L))))
            _case(cases, _call(L, O, B=2, dtype=dtype, store=store, tune=tune_word(3, lty, 3, x_march=1, nseg=nseg) | nowc), ('exact', 'smooth'),
                  'patch asked for 2^%d x 8' % lty)
    # ---- x-march, mixed lengths, explicit word: het_full = 0; het_full > 0 with entries that own split columns and entries that own none;
    # ---- the last XCD's list short
    for L, dtype, nowc in ((32, 'f32', NO_WC), (32, 'bf16', 0), (24, 'f32', 0), (28, 'bf16', 0), (64, 'f32', 0)):
        tune, O0, O1 = xm_word('mixed')
        _case(cases, _call(L, (O0, O1, 19), B=2, dtype=dtype, tune=tune | nowc), ('exact', 'smooth'), 'mixed')
        _case(cases, _call(L, (5, 14, 30), B=33, dtype=dtype, tune=tune | nowc), ('exact', 'lattice'), 'mixed, 2 of 66 columns split')
    _case(cases, _call(32, (5, 12, 56), B=25, tune=xm_word('mixed')[0] | NO_WC), ('exact', 'smooth'), 'mixed, last list short')
    _case(cases, _call(28, (5, 12, 56), B=25, store=True, tune=xm_word('mixed')[0]), ('exact', 'incoherent'), 'mixed, last list short')
    # ---- x-march, mixed lengths, default word (tune 0) where xmarch_applies
    # ---- (the float32 register kernel has no default word at 32 labels: bit 30 needs a word of its own)
    for L, dtype in ((32, 'bf16'), (24, 'f32'), (28, 'bf16')):
        _case(cases, _call(L, (16, 32, 64), S=(9, 10, 11), B=8, dtype=dtype), ('exact', 'smooth'), 'default word, 64 columns per XCD')
    _case(cases, _call(32, (16, 32, 64), S=(9, 10, 11), B=9, dtype='bf16'), ('exact', 'lattice'), 'default word, entry 0 owns no split column')
    # ---- the wave-cache kernel: 3 modes x STORE x MM x FILL, not persistent (small shapes, equal and mixed) and persistent
    n = 0
    for mode in (ABSOLUTE, SHIFT, LINSPACE):
        for store in (False, True):
            for mm in (False, True):
                for fill in (False, True):
                    xv = ('x1', 'x3', 'mixed', 'x5')[n % 4]
                    tune, O0, O1 = xm_word(xv)
                    _case(cases, _call(32, (O0, O1, 19), B=2, mode=mode, store=store, minmax=mm, fill=fill, tune=tune | (WC if n % 2 else 0)),
                          ('exact',) + RANDOM_KINDS, xv)
                    tune = xm_word('x1' if n % 2 else 'mixed')[0]
                    _case(cases, _call(32, (7, 51, 63), S=(9, 21, 23), B=5, mode=mode, store=store, minmax=mm, fill=fill, tune=tune),
                          ('exact', RANDOM_KINDS[n % 3]), 'x1' if n % 2 else 'mixed')
                    n += 1
    _case(cases, _call(32, (7, 12, 344), S=(9, 10, 41), B=4, tune=xm_word('x1')[0]), ('exact', 'incoherent'), 'x1, last list 4 items short')
    _case(cases, _call(32, (5, 14, 30), B=33, tune=xm_word('mixed')[0]), ('exact', 'lattice'), 'mixed, 2 of 66 columns split')
    _case(cases, _call(32, (5, 12, 56), B=25, store=True, tune=xm_word('mixed')[0]), ('exact', 'smooth'), 'mixed, last list short')
    _case(cases, _call(32, (16, 32, 64), S=(9, 10, 11), B=8), ('exact', 'smooth'), 'default word, 64 columns per XCD')
    _case(cases, _call(32, (16, 32, 64), S=(9, 10, 11), B=9, store=True), ('exact', 'lattice'), 'default word, entry 0 owns no split column')
    # ---- the wave-cache kernel without its Dice half: nrt_interpn_f32_ex variant 10 (default word: >= 512 columns of >= 16 planes)
    for mode in (ABSOLUTE, SHIFT, LINSPACE):
        for fill in (False, True):
            for O in ((16, 32, 64), (16, 32, 72)):
                _case(cases, _call(32, O, S=(9, 10, 11), B=8, mode=mode, fill=fill, store=True, minmax=False, entry='interpn'),
                      ('smooth', 'incoherent'), 'variant 10')
    assert len({c.id for c in cases}) == len(cases), [c.id for c in cases if [d.id for d in cases].count(c.id) > 1]
    return cases


CASES = build_table()
IDS = [c.id for c in CASES]


# the refused calls of the GPU file with the status warp_dice_soft_impl returns, the first the control: the same call without a fault
REFUSED = [
    ('control', Call(16, (9, 9, 9), (7, 7, 7)), wdo.OK),
    ('5 labels', Call(5, (9, 9, 9), (7, 7, 7)), wdo.ERR_UNSUPPORTED),
    ('2 labels', Call(2, (9, 9, 9), (7, 7, 7)), wdo.ERR_UNSUPPORTED),
    ('260 labels', Call(260, (9, 9, 9), (7, 7, 7)), wdo.ERR_UNSUPPORTED),
    ('moving 4 bytes off', Call(16, (9, 9, 9), (7, 7, 7), mov_off=4), wdo.ERR_INVALID_ARG),
    ('fixed 4 bytes off', Call(16, (9, 9, 9), (7, 7, 7), fix_off=4), wdo.ERR_INVALID_ARG),
    ('warped 4 bytes off', Call(16, (9, 9, 9), (7, 7, 7), store=True, warped_off=4), wdo.ERR_INVALID_ARG),
    ('sums NULL', Call(16, (9, 9, 9), (7, 7, 7), null=('sums',)), wdo.ERR_INVALID_ARG),
    ('dice NULL', Call(16, (9, 9, 9), (7, 7, 7), null=('dice',)), wdo.ERR_INVALID_ARG),
    ('fixed NULL', Call(16, (9, 9, 9), (7, 7, 7), null=('fixed',)), wdo.ERR_INVALID_ARG),
    ('workspace one byte short', Call(16, (9, 9, 9), (7, 7, 7), ws_short=1), wdo.ERR_WORKSPACE),
    ('workspace one byte short, wave cache', Call(32, (9, 9, 9), (7, 7, 19), tune=xm_word('x1')[0], ws_short=1), wdo.ERR_WORKSPACE),
    ('empty output', Call(16, (9, 9, 9), (7, 0, 7)), wdo.ERR_INVALID_ARG),
]


def inst_of(cid):
    return cid.split(' ')[0]


def coarse_shape(O):
    """LINSPACE on the wave-cache kernel: a regular grid with a step near 1 never has two rows in one cache slot.  Steps of
    4 + 1 / (O - 1) along y and 5 + 1 / (O - 1) along z (coprime again) put the y-neighbours of a wave 4 rows apart, which share a slot,
    and its z-neighbours 5 apart, of which those 8 apart do: passes with a few orphans and passes with more than 16"""
    return (grid_shape(O)[0], 4 * (O[1] - 1) + 2, 5 * (O[2] - 1) + 2)


def run_call(c, kind):
    """the call of one run of a case: the exact LINSPACE run has S = (O + 1) / 2, the random one a non-dyadic step"""
    if c.mode != LINSPACE:
        return c
    return dataclasses.replace(c, S=grid_shape(c.O) if kind == 'grid' else coarse_shape(c.O) if kind == 'coarse' else source_shape(c))


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and references (per shape and field, shared by the ids that differ in STORE, MM, the schedule or the storage type only)
# ------------------------------------------------------------------------------------------------------------------------------

Inputs = namedtuple('Inputs', 'mov fix loc warped ref absloc zero_label')


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def exact_positions(rng, S, O):
    """absolute locations [*O, 3] on the lattice of the module docstring"""
    n = int(np.prod(O))
    Sa = np.array(S, D)
    grid = np.stack(np.meshgrid(*[np.arange(o, dtype=D) for o in O], indexing='ij'), -1).reshape(n, 3)
    scale = np.array([(S[d] - 1) / max(O[d] - 1, 1) for d in range(3)])
    pos = np.clip(np.rint(grid * scale) + rng.choice(np.array([-1, -0.5, 0, 0.5, 1.0]), (n, 3)), 0, Sa - 1)
    i, qa = np.arange(n), np.arange(n) % 3
    pos[i, qa] = np.minimum(np.floor(pos[i, qa]), Sa[qa] - 2) + rng.choice(np.array([0.25, 0.75]), n)
    out = np.nonzero(rng.random(n) < 0.3)[0]
    ax, far = rng.integers(0, 3, out.size), rng.integers(0, 2, out.size)
    step = np.where(ax == qa[out], 0.25, 0.5) + rng.integers(0, 3, out.size)
    pos[out, ax] = np.where(far == 1, Sa[ax] - 1 + step, -step)
    return pos.reshape(tuple(O) + (3,)).astype(F)


@functools.lru_cache(maxsize=6)
def _build(L, S, O, B, mode, shared_loc, kind, fill, bf16):
    c = Call(L, S, O, B=B, mode=mode, shared_loc=shared_loc, fill=fill)
    rng = _rng(L, S, O, B, mode, shared_loc, kind, fill, bf16)
    nl = 1 if shared_loc else B
    zero_label = None
    if kind == 'exact':
        vmax = 3 if c.nout <= 6500 else 1
        mov = rng.integers(0, vmax + 1, (B,) + S + (L,)).astype(F)
        fix = rng.integers(0, vmax + 1, (B,) + O + (L,)).astype(F)
        loc = None if mode == LINSPACE else np.stack([exact_positions(rng, S, O) for _ in range(nl)])
        labels = rng.permutation(L)[:5]                       # the four spikes and the zero label: five different labels (L = 4: the last two coincide)
        big = vmax + 2
        # interior source voxels r (1 .. S - 2 per axis) for the moving map's spikes, sampled with weight 1 by one output voxel each
        r = [tuple(int(rng.integers(1, s - 1)) for s in S) for _ in range(2)]
        while r[1] == r[0]:
            r[1] = tuple(int(rng.integers(1, s - 1)) for s in S)
        q = [tuple(int(rng.integers(0, o)) for o in O) for _ in range(2)]
        while q[1] == q[0]:
            q[1] = tuple(int(rng.integers(0, o)) for o in O)
        if mode != LINSPACE:
            loc[0][q[0]] = r[0]
            loc[nl - 1][q[1]] = r[1]
        mov[(0,) + r[0] + (labels[0],)] = big
        mov[(B - 1,) + r[1] + (labels[1],)] = -big
        qf = [tuple(int(rng.integers(0, o)) for o in O) for _ in range(2)]
        fix[(0,) + qf[0] + (labels[2],)] = big
        fix[(B - 1,) + qf[1] + (labels[3 % len(labels)],)] = -1
        if not fill and L > 4:
            zero_label = int(labels[4])
            mov[..., zero_label] = 0
            fix[..., zero_label] = 0
        if mode == SHIFT:
            grid = np.stack(np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij'), -1)
            loc = (loc - grid).astype(F)
        fv = FILL_EXACT
    else:
        mov, fix = rng.random((B,) + S + (L,)).astype(F), rng.random((B,) + O + (L,)).astype(F)
        if bf16:
            mov, fix = npo.round_bf16(mov), npo.round_bf16(fix)
        loc = None if mode == LINSPACE else np.stack([wfo.make_field(rng, S, O, 1, kind, mode)[1] for _ in range(nl)])
        fv = FILL_RANDOM
    warped, absloc = wdo.warp_ref(c, mov, loc, fv)
    return Inputs(mov, fix, loc, warped, wdo.soft_ref(fix, warped), absloc, zero_label)


def inputs(c, kind, fill):
    """the tensors of one run -- mov [B, *S, L], fix [B, *O, L] (float32 arrays holding values of the storage type), loc [B or 1, *O, 3] or
    None -- with the reference's float32 `warped`, the float64 reference of the sums and the absolute locations.  Read-only: shared."""
    rc = run_call(c, kind)
    return _build(rc.L, tuple(rc.S), tuple(rc.O), rc.B, rc.mode, rc.shared_loc, kind, bool(fill), rc.dtype == 'bf16' and kind != 'exact')


def fill_value(kind):
    return FILL_EXACT if kind == 'exact' else FILL_RANDOM


def runs(cs):
    """(kind, fill, laplace_smoothing) of every launch of a case.  The register kernels take the fill at run time: the exact run without
    (smoothing 0, a label with denominator 0) and with (0.5), the random run alternating; FILL is a template argument of the wave-cache
    kernel: the case's own."""
    c = cs.call
    wc = inst_of(cs.id).startswith('warp_dice_wc')
    out = []
    for i, kind in enumerate(cs.kinds):
        if kind == 'exact':
            out += [('exact', c.fill, 0.0), ('exact', c.fill, 0.5)] if wc else [('exact', False, 0.0), ('exact', True, 0.5)]
        else:
            out.append((kind, c.fill if wc else bool((zlib.crc32(cs.id.encode()) + i) & 1), 0.5))
    return out


def storage(x, dtype):
    """the bytes of the storage type: float32, or the upper halves of float32 values that are bfloat16 values"""
    x = np.ascontiguousarray(x, F)
    if dtype == 'f32':
        return x
    bits = x.view(np.uint32)
    assert not (bits & 0xffff).any()
    return (bits >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------------
# premises, on the references alone
# ------------------------------------------------------------------------------------------------------------------------------

def outside_share(S, absloc):
    p = np.concatenate([np.asarray(a, D).reshape(-1, 3) for a in absloc])
    return float(((p < 0) | (p > np.array(S, D) - 1)).any(1).mean())


def unequal_weight_share(S, absloc):
    """per axis, the share of voxels whose two blend weights differ (corner_1d on the clipped location)"""
    p = np.concatenate([np.asarray(a, D).reshape(-1, 3) for a in absloc])
    mx = np.array(S, D) - 1
    cl = np.clip(p, 0, mx)
    w0 = np.minimum(np.floor(cl) + 1, mx) - cl
    return (w0 != 1 - w0).mean(0)
