"""
TEST INFRASTRUCTURE ONLY -- the restated dispatch of the warp forward (neurite_amd/csrc/interpn.hip, interpn_lean.hip, interpn_any.hip:
nrt_interpn_f32_ex, nrt_interpn_f32, nrt_interpn_add_f32, nrt_interpn_nearest_i32, nrt_interpn_any) and the bit-exact reference of
every call tests/test_gpu_warp_forward_arms.py makes.

`plan(call)` is written from the three .hip files: which template instance a call launches (in the spelling of
profiles/dispatch_arms/interpn*_kernels.txt after tools/arm_coverage.norm) or the status it returns before any launch, with the launch
geometry worth naming in a test id.  `reference` adds no arithmetic: float32 in 1..3-D is oracle.c_oracle.interpn on the float32
location the kernels form (oracle.warp_bwd_oracle.locations), every other type and rank oracle.np_oracle.interpn, bfloat16
np_oracle.interpn_emulated with round_bf16; the addend epilogue is the one float32 addition `addend + warped` of vxm's compose.

Fields (`make_field`): 'smooth' is the backward oracle's (noise of amplitude 1.5 around the grid that maps the output onto the source,
locations put on integers, on 0 and on the far border); 'incoherent' is uniform on [-1, S_d] per component (the backward's 'rough'
field leaves a 9 x 8 x 7 volume on 98 - 100 % of the voxels, useless with a fill value); 'lattice' adds displacements drawn from
{-3, -1, -0.5, 0, 0.5, 1, 2, 7.5} to the rounded grid: the exact halves round-half-even must get right (in 5 dimensions from
{-1, -0.5, 0, 0.5, 1}: with the whole set the large displacements alone mask 0.86 of the voxels).

Only tests/ may import this module.
"""

import dataclasses
import zlib
from collections import namedtuple

import numpy as np

from . import c_oracle as co
from . import np_oracle as npo
from . import warp_bwd_oracle as wbo

F = np.float32
ABSOLUTE, SHIFT, LINSPACE = 0, 1, 2
LINEAR, NEAREST = 0, 1
MODES = {'ABSOLUTE': ABSOLUTE, 'SHIFT': SHIFT, 'LINSPACE': LINSPACE}
OK, INVALID_ARG, UNSUPPORTED = 'NRT_OK', 'NRT_ERR_INVALID_ARG', 'NRT_ERR_UNSUPPORTED'
NXCD = 8
ELEM = {'f32': 4, 'f64': 8, 'f16': 2, 'bf16': 2, 'i32': 4}
TNAME = {'f32': 'float', 'f64': 'double', 'f16': 'HalfTag', 'bf16': 'Bf16Tag'}
LATTICE = np.array([-3, -1, -0.5, 0, 0.5, 1, 2, 7.5], F)
FILL_F, FILL_I = -7.5, -7                       # -7.5 is a value of every float type here
locations = wbo.locations


@dataclasses.dataclass(frozen=True)
class Call:
    """one call of the C ABI.  entry: 'f32_ex', 'f32', 'add', 'i32' (nrt_interpn_nearest_i32) or 'any'.  *_off: bytes between a
    32-byte boundary and the pointer; *_pad: elements added to the contiguous batch stride; shared_*: batch stride 0."""
    entry: str
    S: tuple
    O: tuple
    C: int
    mode: int = SHIFT
    method: int = LINEAR
    dtype: str = 'f32'
    B: int = 2
    variant: int = 0
    tune: int = 0
    vol_off: int = 0
    out_off: int = 0
    loc_off: int = 0
    add_off: int = 0
    vol_pad: int = 0
    loc_pad: int = 0
    add_pad: int = 0
    shared_vol: bool = False
    shared_loc: bool = False
    loc_f64: bool = False

    @property
    def D(self):
        return len(self.S)

    @property
    def rows(self):
        return int(np.prod(self.S))

    @property
    def nout(self):
        return int(np.prod(self.O))

    @property
    def vol_bs(self):
        return 0 if self.shared_vol else self.rows * self.C + self.vol_pad

    @property
    def loc_bs(self):
        return 0 if self.shared_loc else self.nout * self.D + self.loc_pad

    @property
    def add_bs(self):
        return self.nout * self.C + self.add_pad

    @property
    def has_loc(self):
        return self.mode != LINSPACE


Plan = namedtuple('Plan', 'names status tags')


def plan_id(p):
    return ('+'.join(p.names) if p.names else p.status) + (' ' + p.tags if p.tags else '')


def _refuse(status):
    return Plan((), status, '')


def cdiv(a, b):
    return (a + b - 1) // b


def xcd_grid(n):
    return NXCD * cdiv(n, NXCD)


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_core.h / interpn.hip
# ------------------------------------------------------------------------------------------------------------------------------

def fill_args_status(c, max_d=3):
    """fill_args: the argument checks every float32 / int32 entry point starts with"""
    if c.D < 1 or c.D > max_d or c.C < 1 or c.B < 1 or c.mode not in (0, 1, 2):
        return INVALID_ARG
    if c.B > 65535:
        return UNSUPPORTED
    if any(s < 1 for s in c.S) or any(o < 0 for o in c.O):
        return INVALID_ARG
    if c.rows * c.C >= 1 << 40 or c.nout >= 1 << 31:
        return UNSUPPORTED
    return None


def tile_geometry(O, G, tune, default_tune):
    """tile_geometry of interpn_core.h: the tile a block owns and the tile counts"""
    NG, WZ = 256 // G, 64 // G
    if tune <= 0:
        tune = default_tune
    ltx, lty, ltz, z_outer = tune & 15, (tune >> 4) & 15, (tune >> 8) & 15, (tune >> 12) & 1
    plane_major = bool((tune >> 13) & 1) and G == 8
    if plane_major:
        ltx, lty, ltz = 2, 3, 0
        tz = (tune >> 16) & 0xfff
        if tz <= 0 or tz > O[2]:
            tz = O[2]
    else:
        while (1 << ltz) < WZ:
            ltz += 1
        while (1 << (ltx + lty + ltz)) < NG:
            lty += 1
        tz = 1 << ltz
    nTx, nTy, nTz = cdiv(O[0], 1 << ltx), cdiv(O[1], 1 << lty), cdiv(O[2], tz)
    per2 = cdiv(nTx * nTy, NXCD)
    return dict(ltx=ltx, lty=lty, ltz=ltz, tz=tz, z_outer=z_outer, plane_major=plane_major, nT=(nTx, nTy, nTz), ntiles=NXCD * per2 * nTz,
                npass=tz if plane_major else (1 << (ltx + lty + ltz)) // NG)


TILE_DEFAULT = 2 | (2 << 4) | (4 << 8) | (1 << 12)
TILE_AUTO_C16 = 2 | (3 << 4) | (4 << 8) | (1 << 12)
ZRUN_AUTO = 20 | (1 << 16)
ZRUN_PATCH = {0: (2, 2), 1: (4, 2), 2: (4, 4), 3: (2, 4)}


def zrun_tune(LZ=0, zc_outer=0, patch=0, lreg=0, lds_kb=0):
    return LZ | zc_outer << 12 | patch << 16 | lreg << 20 | lds_kb << 24


def _plan_generic(c, T='float', addend=False):
    total = c.nout * c.C
    blocks = min(cdiv(total, 256), 4096)
    tags = 'passes%d' % cdiv(total, blocks * 256) + (' addend' if addend else '')
    return Plan(('interpn_generic<%d,%d,%d,%s>' % (c.D, c.mode, c.method, T),), None, tags)


def _plan_rows(c, tune):
    G = c.C // 4
    vpb = (256 // G) * (tune if tune > 0 else 4)
    nblk = cdiv(c.nout, vpb)
    return Plan(('interpn_rows<%d,%d,%d>' % (G, c.mode, c.method),), None, 'vpb%d blocks%d last%d' % (vpb, nblk, c.nout - (nblk - 1) * vpb))


def _plan_tile(c, tune):
    G = c.C // 4
    g = tile_geometry(c.O, G, tune, TILE_DEFAULT)
    ext = (1 << g['ltx'], 1 << g['lty'], g['tz'])
    partial = ''.join(n for n, o, e in zip('xyz', c.O, ext) if o % e)
    tags = 'tile%dx%dx%d passes%d tiles%dx%dx%d partial-%s%s%s' % (ext + (g['npass'],) + g['nT'] + (partial or 'none', ' z_outer' if g['z_outer'] else '',
                                                                   ' plane_major' if g['plane_major'] else ''))
    return Plan(('interpn_tile<%d,%d>' % (G, c.mode),), None, tags)


def _plan_zrun(c, tune):
    LZ, zc_outer, patch, lreg, lds_kb = tune & 0xfff, (tune >> 12) & 1, (tune >> 16) & 3, (tune >> 20) & 7, (tune >> 24) & 0x7f
    if LZ <= 0 or LZ > c.O[2]:
        LZ = c.O[2]
    WX, WY = ZRUN_PATCH[patch]
    nTx, nTy, nZc = cdiv(c.O[0], 2 * WX), cdiv(c.O[1], 4 * WY), cdiv(c.O[2], LZ)
    pad = 0
    if lreg > 0:
        R = 1 << lreg
        pad = cdiv(nTx, R) * cdiv(nTy, R) * R * R - nTx * nTy
    tags = 'patch%d LZ%d zchunks%d patches%dx%d zc_outer%d lreg%d pad%d lds%dK%s' % (patch, LZ, nZc, nTx, nTy, zc_outer, lreg, pad, lds_kb,
                                                                                  '(attr)' if lds_kb * 1024 > 48 * 1024 else '')
    return Plan(('interpn_zrun_c32<%d,%d,%d>' % (c.mode, WX, WY),), None, tags)


def xmarch_applies(O, B):
    return O[0] >= 16 and cdiv(O[1], 4) * cdiv(O[2], 8) * B >= 512


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_lean.hip
# ------------------------------------------------------------------------------------------------------------------------------

def lean_supported(c):
    if c.D != 3 or c.C < 1 or c.C > 4:
        return False
    if any(s < 1 or s >= 1 << 12 for s in c.S) or any(o < 1 or o >= 1 << 12 for o in c.O):
        return False
    if 4 * c.C * c.rows >= 1 << 32 or c.nout * 12 >= 1 << 32 or c.nout * 4 * c.C >= 1 << 32:
        return False
    if (c.vol_off | c.out_off | (c.loc_off if c.has_loc else 0)) & 15:
        return False
    return (c.vol_bs * 4) % (16 if c.C == 4 else 8 if c.C == 2 else 4) == 0


def _plan_lean(c, kind, addend=False):
    """nrt_lean_launch.  kind 0 linear, 1 nearest float32, 2 nearest int32.  Every call with per-voxel locations takes the tile form,
    so interpn_lean<C, VPL, ABSOLUTE | SHIFT> cannot be chosen."""
    C, O = c.C, c.O
    if c.mode != LINSPACE:
        ltz, lty = (4, 1) if (C >= 2 and kind == 0) else (5, 2)
        while ltz > 0 and (1 << (ltz - 1)) >= O[2]:
            ltz, lty = ltz - 1, lty + 1
        while lty > 0 and (1 << (lty - 1)) >= O[1]:
            lty -= 1
        ltx = 8 - ltz - lty
        ntiles = cdiv(O[0], 1 << ltx) * cdiv(O[1], 1 << lty) * cdiv(O[2], 1 << ltz)
        tpb = 4 if C == 1 else 1
        while tpb > 1 and (ntiles // tpb) * c.B < 2048:
            tpb >>= 1
        return Plan(('interpn_lean_tile<%d,%d,%d>' % (C, c.mode, kind),), None,
                    'ltz%d lty%d tpb%d tiles%d%s' % (ltz, lty, tpb, ntiles, ' addend' if addend else ''))
    if kind != 0:
        return _refuse(UNSUPPORTED)
    add_bs = c.add_bs if addend else 0
    out_bs = c.nout * C
    if C == 1:
        VPL = 4 if (O[2] % 4 == 0 and (c.loc_bs * 4) % 16 == 0 and (add_bs * 4) % 16 == 0) else 1
    elif C == 2:
        VPL = 4 if (O[2] % 4 == 0 and (out_bs * 4) % 16 == 0) else 2 if (O[2] % 2 == 0 and (c.loc_bs * 4) % 8 == 0 and (add_bs * 4) % 16 == 0) else 1
    elif C == 3:
        VPL = 4 if (O[2] % 4 == 0 and (out_bs * 4) % 16 == 0) else 1
    else:
        VPL = 4 if O[2] % 4 == 0 else 1
    lpr = O[2] // VPL
    return Plan(('interpn_lean<%d,%d,%d>' % (C, VPL, LINSPACE),), None, 'VPL%d lpr%d cpp%d%s' % (VPL, lpr, cdiv(O[1] * lpr, 256), ' addend' if addend else ''))


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_any.hip
# ------------------------------------------------------------------------------------------------------------------------------

def _plan_any(c, dtype):
    if c.D < 1 or c.D > 8 or c.C < 1 or c.B < 1 or c.mode not in (0, 1, 2) or c.method not in (0, 1):
        return _refuse(INVALID_ARG)
    if c.B > 65535:
        return _refuse(UNSUPPORTED)
    if c.loc_f64 and not (dtype == 'f64' and c.mode == ABSOLUTE):
        return _refuse(INVALID_ARG)
    if c.rows * c.C >= 1 << 40 or c.nout * c.C >= 1 << 40:
        return _refuse(UNSUPPORTED)
    if c.nout == 0:
        return Plan((), OK, 'nothing to do')
    near = 'true' if c.method == NEAREST else 'false'
    if dtype == 'i32':
        if c.method != NEAREST:
            return _refuse(UNSUPPORTED)
        return Plan(('interpn_any_nearest_i32',), None, 'rank%d' % c.D)
    if c.D <= 3:
        why = [w for w, bad in (('C%4', c.C % 4), ('stride%4', c.vol_bs % 4), ('ptr%32', (c.vol_off | c.out_off) & 31)) if bad]
        CG = 1 if why else 4
        return Plan(('interpn_any_nd<%s,%s,%d,%d>' % (TNAME[dtype], near, c.D, CG),), None, 'CG%d%s' % (CG, '(%s)' % ','.join(why) if why else ''))
    return Plan(('interpn_any<%s,%s>' % (TNAME[dtype], near),), None, 'rank%d' % c.D)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry points
# ------------------------------------------------------------------------------------------------------------------------------

def rows_supported(C):
    return C % 4 == 0 and C // 4 in (1, 2, 4, 8, 16, 32, 64)


def plan(c):
    """the instance(s) `c` launches, or the status it returns before any launch, and the geometry tags of the launch"""
    if c.entry == 'any':
        return _plan_any(c, c.dtype)
    st = fill_args_status(c)
    if st:
        return _refuse(st)
    if c.entry == 'add':
        if c.nout == 0:
            return Plan((), OK, 'nothing to do')
        if c.add_off % 16 == 0 and (c.add_bs * 4) % 16 == 0 and lean_supported(c):
            return _plan_lean(c, 0, addend=True)
        return _plan_generic(dataclasses.replace(c, method=LINEAR), addend=True)
    if c.entry == 'i32':
        if c.nout == 0:
            return Plan((), OK, 'nothing to do')
        c = dataclasses.replace(c, method=NEAREST)
        if c.mode != LINSPACE and lean_supported(c):
            return _plan_lean(c, 2)
        return _plan_generic(c, 'int')
    assert c.entry in ('f32', 'f32_ex'), c.entry
    variant, tune = (c.variant, c.tune) if c.entry == 'f32_ex' else (0, 0)
    if c.method not in (LINEAR, NEAREST):
        return _refuse(INVALID_ARG)
    if c.nout == 0:
        return Plan((), OK, 'nothing to do')
    aligned = ((c.vol_off | c.out_off) & 15) == 0 and (c.vol_bs * 4) % 16 == 0
    can_rows = rows_supported(c.C) and aligned and c.D == 3
    small = 4 * c.C * c.rows < 1 << 32
    can_zrun = can_rows and c.C == 32 and c.method == LINEAR and small
    can_lean = (c.mode == LINSPACE or c.has_loc) if c.method == LINEAR else (c.mode != LINSPACE and c.has_loc)
    can_lean = can_lean and lean_supported(c)
    if variant == 0:
        if can_zrun:
            if c.mode != LINSPACE and tune == 0 and xmarch_applies(c.O, c.B):
                return Plan(('not warp_fwd: the wave-cache kernel (variant 10) where wc_applies',), None, '')
            variant = 3
            tune = tune or ZRUN_AUTO
        elif can_lean:
            variant = 8
        elif can_rows and c.method == LINEAR and small and c.nout >= 4096:
            variant = 5
            if tune == 0:
                tune = TILE_AUTO_C16 if c.C <= 16 else 0
        elif can_rows:
            variant = 2
        elif c.C % 4 == 0 and aligned:
            return _plan_any(c, 'f32')
        else:
            variant = 1
    if variant == 3 and not can_zrun:
        return _refuse(UNSUPPORTED)
    if variant == 5 and not (can_rows and c.method == LINEAR and small):
        return _refuse(UNSUPPORTED)
    if variant == 2 and not can_rows:
        return _refuse(UNSUPPORTED)
    if variant == 1:
        return _plan_generic(c)
    if variant == 2:
        return _plan_rows(c, tune)
    if variant == 3:
        return _plan_zrun(c, tune)
    if variant == 5:
        return _plan_tile(c, tune)
    if variant == 8:
        return _plan_lean(c, 1 if c.method == NEAREST else 0) if can_lean else _refuse(UNSUPPORTED)
    if variant == 10:
        return Plan(('not warp_fwd: the wave-cache kernel (variant 10)',), None, '') if can_zrun else _refuse(UNSUPPORTED)
    return _refuse(INVALID_ARG)


# the instances no call can launch (profiles/dispatch_arms/README.md): nrt_lean_launch sends every call that is not LINSPACE to
# interpn_lean_tile, so the row form is only ever launched in LINSPACE mode
UNREACHABLE = sorted('interpn_lean<%d,%d,%d>' % (C, V, m) for C, Vs in ((1, (1, 4)), (2, (1, 2, 4)), (3, (1, 4)), (4, (1, 4))) for V in Vs for m in (0, 1))


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and the reference
# ------------------------------------------------------------------------------------------------------------------------------

def to_type(x, dtype):
    """values of the storage type, in the array type the oracles take (bfloat16: float32 arrays holding bfloat16 values)"""
    if dtype == 'bf16':
        return npo.round_bf16(np.asarray(x, F))
    return np.asarray(x).astype({'f32': F, 'f64': np.float64, 'f16': np.float16, 'i32': np.int32}[dtype])


def make_field(rng, S, O, C, kind, mode, dtype='f32'):
    """vol [*S, C] of `dtype` and the float32 location tensor of `mode` [*O, D] (None for LINSPACE)"""
    D = len(S)
    if kind in ('smooth', 'grid'):
        vol, loc, _ = wbo.make_field(rng, S, O, C, 'smooth', mode)
        for d in range(D):                                   # an axis with one sample: mid-volume, not on the border at 0
            if loc is not None and O[d] == 1:
                loc[..., d] = (loc[..., d] + F((S[d] - 1) // 2)).astype(F)
    else:
        vol = rng.standard_normal(tuple(S) + (C,)).astype(F)
        grid = np.stack(np.meshgrid(*[np.arange(o, dtype=F) for o in O], indexing='ij'), -1)
        if kind == 'incoherent':
            pos = (rng.random(tuple(O) + (D,)) * (np.array(S, np.float64) + 1.0) - 1.0).astype(F)
        else:
            assert kind == 'lattice', kind
            scale = np.array([(S[d] - 1) / max(O[d] - 1, 1) for d in range(D)], np.float64)
            centre = np.array([(S[d] - 1) / 2 if O[d] == 1 else 0.0 for d in range(D)])       # an axis with one sample: mid-volume, not on a border
            lat = LATTICE if D < 5 else LATTICE[np.abs(LATTICE) <= 1]      # 5-D: -3, 2 and 7.5 alone would mask 0.86 of the voxels
            pos = (np.rint(grid * scale + centre) + lat[rng.integers(0, len(lat), tuple(O) + (D,))]).astype(F)
        loc = None if mode == LINSPACE else pos if mode == ABSOLUTE else (pos - grid).astype(F)
    if dtype == 'i32':
        vol = rng.integers(-1000, 1000, vol.shape).astype(np.int32)
    elif dtype == 'f64':
        vol = vol.astype(np.float64) + rng.standard_normal(vol.shape) * 2.0 ** -30      # not float32 values
    return to_type(vol, dtype), loc


def reference(c, vol, loc, fill, addend=None):
    """vol [*S, C] of the call's type, loc: the absolute location [*O, D] (float32 from `locations`; float64 with loc_f64)"""
    method = 'nearest' if c.method == NEAREST else 'linear'
    fv = None if not fill else FILL_I if c.dtype == 'i32' else FILL_F
    if c.dtype == 'f32' and c.D <= 3:
        ref = co.interpn(vol, loc, method, fv, loc_mode=0)
    elif c.dtype == 'bf16':
        ref = npo.interpn_emulated(vol, loc, method, fv, npo.round_bf16)
    else:
        ref = npo.interpn(vol, loc, method, fv)
        assert ref.dtype == vol.dtype, (ref.dtype, vol.dtype)
    if addend is not None:
        ref = (addend + ref).astype(F)
    return ref


Inputs = namedtuple('Inputs', 'vol loc addend absloc refs')


def inputs(c, kind, fill, with_refs=True):
    """the tensors of one launch -- vol [Bv, *S, C], loc [Bl, *O, D] or None, addend [B, *O, C] or None -- with the absolute location
    and the reference of every batch entry.  Seeded by the call and the field alone."""
    rng = np.random.default_rng(zlib.crc32(repr((dataclasses.astuple(c), kind, fill)).encode()))
    Bv, Bl = 1 if c.shared_vol else c.B, 1 if c.shared_loc else c.B
    fields = [make_field(rng, c.S, c.O, c.C, kind, c.mode, c.dtype) for _ in range(max(Bv, Bl))]
    vol = np.stack([f[0] for f in fields[:Bv]])
    loc = None if c.mode == LINSPACE else np.stack([f[1] for f in fields[:Bl]])
    f64 = c.loc_f64 and loc is not None
    if f64:                                               # ABSOLUTE only: locations that are no float32 values (a lattice keeps its halves)
        loc = loc.astype(np.float64) + rng.standard_normal(loc.shape) * (0.0 if kind == 'lattice' else 2.0 ** -30)
    addend = rng.standard_normal((c.B,) + tuple(c.O) + (c.C,)).astype(F) if c.entry == 'add' else None
    absloc, refs = [], []
    for b in range(c.B):
        lb = None if loc is None else loc[0 if c.shared_loc else b]
        a = lb if f64 else locations(c.mode, c.S, c.O, lb)
        absloc.append(a)
        if with_refs:                                     # (a refused call has no reference)
            refs.append(reference(c, vol[0 if c.shared_vol else b], a, fill, None if addend is None else addend[b]))
    return Inputs(vol, loc, addend, absloc, refs)


def subcalls(c):
    """the launches of one id: every field x fill at the call's batch, then a shared location tensor, a shared volume and a single
    entry (a smooth field with a fill value).  LINSPACE has no field: with and without fill, a shared volume, a single entry.  In 4 and
    5 dimensions the smooth field (amplitude 1.5 in every component) leaves the volume on more than 75 % of the voxels of any shape
    small enough for a test; there the fields are the incoherent and the lattice one, the lattice of 5 dimensions with the displacements
    {-1, -0.5, 0, 0.5, 1} only."""
    kinds = ('grid',) if c.mode == LINSPACE else ('smooth', 'incoherent', 'lattice') if c.D <= 3 else ('incoherent', 'lattice')
    out = [(c, k, f) for k in kinds for f in (False, True)]
    if c.B > 1:
        if c.mode != LINSPACE:
            out.append((dataclasses.replace(c, shared_loc=True, loc_pad=0), kinds[0], True))
        if c.vol_pad == 0:
            out.append((dataclasses.replace(c, shared_vol=True), kinds[0], True))
        out.append((dataclasses.replace(c, B=1), kinds[0], True))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# premises, on the reference alone
# ------------------------------------------------------------------------------------------------------------------------------

def masked_share(c, absloc):
    """share of the output voxels with a component outside [0, S_d - 1]: filled with a fill value, clamped without"""
    p = np.asarray(absloc, np.float64).reshape(-1, c.D)
    mx = np.array(c.S, np.float64) - 1.0
    return float(((p < 0) | (p > mx)).any(1).mean())


def half_share(absloc):
    p = np.asarray(absloc, np.float64)
    return float((np.abs(p - np.floor(p) - 0.5) == 0).mean())


def inexact_share_f64(c, vol, absloc, limit=2000):
    """the same share for float64, which NumPy has no wider portable type for: the blend of `limit` output elements (all, if there are fewer) in exact
    rational arithmetic (the weights l1 - clip(p), 1 - w0 and their products times the volume values, summed over the 2^D corners),
    against its rounding to float64"""
    from fractions import Fraction
    import itertools
    p = np.asarray(absloc, np.float64).reshape(-1, c.D)
    v = np.asarray(vol, np.float64).reshape(-1, c.C)
    n, bad = min(limit, p.shape[0] * c.C), 0
    for e in np.linspace(0, p.shape[0] * c.C - 1, n).astype(np.int64):          # evenly spread over the output
        q, ch = divmod(int(e), c.C)
        i, w = [], []
        for d in range(c.D):
            mx = c.S[d] - 1
            cl = min(max(Fraction(p[q, d]), 0), mx)
            l0 = min(max(int(np.floor(p[q, d])), 0), mx)
            l1 = min(l0 + 1, mx)
            i.append((l0, l1))
            w.append((l1 - cl, 1 - (l1 - cl)))
        acc = Fraction(0)
        for k in itertools.product((0, 1), repeat=c.D):
            idx, wt = 0, Fraction(1)
            for d in range(c.D):
                idx, wt = idx * c.S[d] + i[d][k[d]], wt * w[d][k[d]]
            acc += wt * Fraction(v[idx, ch])
        bad += Fraction(float(acc)) != acc
    return bad / n


def inexact_share(c, vol, absloc):
    """share of the linear outputs of a narrow type that are not values of the type before the final rounding: the float64 blend of
    the rounded volume at the location cast to the type, against its rounding"""
    if c.dtype == 'f64':
        return inexact_share_f64(c, vol, absloc)
    loc_t = to_type(absloc, c.dtype).astype(np.float64)
    exact = npo.interpn_f64(np.asarray(vol, np.float64), loc_t)
    return float((to_type(exact, c.dtype).astype(np.float64) != exact).mean())
