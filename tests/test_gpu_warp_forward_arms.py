"""
Every dispatch arm of the warp forward (csrc/interpn.hip, interpn_lean.hip, interpn_any.hip: interpn, SpatialTransformer, Resize, VecInt
and compose), each under an id that starts with what oracle/warp_fwd_oracle.plan derives for the call: the template instance the
dispatcher takes (or the status it returns before any launch) and the geometry of the launch.  profiles/dispatch_arms/README.md says
how a kernel trace of this file and tools/arm_coverage.py --families warp_fwd confirm the names; tests/test_warp_fwd_oracle.py checks
without a GPU that every emitted instance of the nine families is named here or is one of the 18 documented unreachable ones, that
every case's written instance is what `plan` derives, and the premises below on every reference.

nrt_interpn_f32_ex, nrt_interpn_f32, nrt_interpn_add_f32, nrt_interpn_nearest_i32 and nrt_interpn_any are called directly on the
guarded buffers of tests/arm_buffers.py (Buf for the float32 entry points, Raw for the other element types, for pointers off their
alignment by more than a float and wherever "not one byte written" is asserted).  Every launched case is compared BIT FOR BIT, every
element, with the reference of oracle/warp_fwd_oracle.py; there is no tolerance in this file.

An id runs (oracle.warp_fwd_oracle.subcalls) smooth, incoherent and lattice fields, each with and without a fill value, on two batch
entries with a location tensor each; then a shared location tensor (loc_batch_stride = 0), a shared volume (vol_batch_stride = 0) and
a single entry.  LINSPACE (Resize) has no field: with and without fill, a shared volume, a single entry.  `light` ids (the large ones)
run two fields and no extras.  Base geometry: source (9, 8, 7) -> output (7, 6, 7) = 294 voxels, distinct extents, no multiple of any
256 / G.

Premises, checked on the references alone (tests/test_warp_fwd_oracle.py): between 15 % and 75 % of the output voxels of a field are
outside the volume (filled with a fill value, clamped without); linear and nearest results of an id differ on at least half of the
outputs (smooth and incoherent fields and regular grids without fill: a lattice field is integer in 5 of 8 components, and a fill
value makes both methods agree on the masked voxels); at least 20 % of a lattice field's location components are exact halves; at
least half of the linear float16 / bfloat16 / float64 outputs are no values of the type before the final rounding (float64: a sample
of the outputs blended in exact rational arithmetic; a smooth field in 1-D cannot have that share: a clamped location and one put on
an integer return a volume value unchanged, which leaves 0.58 at most; 0.50 - 0.56 is reached, 0.497 at bfloat16, and reported, and
the incoherent field of the same id holds 0.5).  In 4 and 5 dimensions the smooth field leaves every small volume on more than 75 %
of the voxels and is left out; the lattice of 5 dimensions draws from {-1, -0.5, 0, 0.5, 1}.

No non-finite locations: test_gpu_interpn.py::test_non_finite_locations_are_memory_safe and its lean test keep that ground.

Which strides a caller can vary: vol_batch_stride and loc_batch_stride on every entry point, addend_batch_stride on
nrt_interpn_add_f32.  The output stride is always prod(O) C, so the `out_bs` conditions of interpn_lean's vector widths hold whenever
O[2] % 4 == 0 does; the width is walked through O[2] % 4, O[2] % 2, the location stride (a number only: LINSPACE has no location tensor)
and the addend stride, which must be a multiple of 4 floats for the lean kernels to be taken at all.

Not covered: the 65536 x 16 block cap of interpn_any_nd / interpn_any needs more than 2^28 threads.  The wave-cache kernel (variant
10, fused_wc.h) and the fused warp + Dice kernels have their own tests.
"""

import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

from arm_buffers import Buf, Raw, call
from conftest import bits_equal
from neurite_amd import _lib
from oracle import warp_fwd_oracle as wfo
from oracle.warp_fwd_oracle import ABSOLUTE, LINEAR, LINSPACE, NEAREST, SHIFT, Call

pytestmark = pytest.mark.gpu
F = np.float32
S3, O3 = (9, 8, 7), (7, 6, 7)
MODES3 = (ABSOLUTE, SHIFT, LINSPACE)
MNAME = {ABSOLUTE: 'ABSOLUTE', SHIFT: 'SHIFT', LINSPACE: 'LINSPACE'}
METH = {LINEAR: 'linear', NEAREST: 'nearest'}
CS = (4, 8, 16, 32, 64, 128, 256)
UNSUPPORTED, INVALID_ARG = wfo.UNSUPPORTED, wfo.INVALID_ARG

# want: the instance (or status) the case is written for; call: the call; label: what the id adds to the plan; light: two fields, no extras
Case = namedtuple('Case', 'want call label light')
CASES = []


def case(want, call_, label='', light=False):
    CASES.append(Case(want, call_, label, light))


def ex(S, O, C, variant, mode=SHIFT, method=LINEAR, tune=0, **kw):
    return Call('f32_ex', tuple(S), tuple(O), C, mode, method, variant=variant, tune=tune, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_rows<G, MODE, METHOD>: variant 2 forced
# ------------------------------------------------------------------------------------------------------------------------------
for C in CS:
    for mode in MODES3:
        for method in (LINEAR, NEAREST):
            case('interpn_rows<%d,%d,%d>' % (C // 4, mode, method), ex(S3, O3, C, 2, mode, method), '%s %s' % (MNAME[mode], METH[method]))
for tune in (1, 7):                                          # passes per block
    case('interpn_rows<4,1,0>', ex(S3, O3, 16, 2, tune=tune), 'tune %d' % tune)
case('interpn_rows<1,1,0>', ex(S3, (5, 59, 1), 4, 2, tune=1), '295 voxels')                      # 256 + 39: the last block is partial
case(UNSUPPORTED, ex(S3, O3, 12, 2), 'rows C=12')
case(UNSUPPORTED, ex((9, 8), (7, 6), 32, 2), 'rows rank 2')
case(UNSUPPORTED, ex(S3, O3, 32, 2, vol_off=4), 'rows vol+4B')
case(UNSUPPORTED, ex(S3, O3, 32, 2, out_off=4), 'rows out+4B')
case(UNSUPPORTED, ex(S3, O3, 32, 2, vol_pad=1), 'rows vol stride rows C + 1')

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_tile<G, MODE>: variant 5 forced; a partial tile on every side for the G's geometry (tz = 64 / G at least, 16 by default)
# ------------------------------------------------------------------------------------------------------------------------------
# (sources whose LINSPACE steps 5/4, 5/8 and 19/16 do not repeat within a tile: with (6, 5, 19) the step 1/2 in y gives two passes of a tile
# the same weights)
TILE_SHAPE = {4: ((6, 6, 70), (5, 9, 66)), 8: ((6, 6, 40), (5, 9, 38))}
TILE_OTHER = ((6, 6, 20), (5, 9, 17))
for C in CS:
    S, O = TILE_SHAPE.get(C, TILE_OTHER)
    for mode in MODES3:
        case('interpn_tile<%d,%d>' % (C // 4, mode), ex(S, O, C, 5, mode), MNAME[mode])
    # z outermost, the smallest tile the G allows: ONE pass per tile (the pipeline takes two per loop turn)
    case('interpn_tile<%d,1>' % (C // 4), ex(S, O, C, 5, tune=1 << 12), 'single pass')
case('interpn_tile<8,1>', ex(*TILE_OTHER, 32, 5, tune=1 | (2 << 4) | (3 << 8)), 'z fastest')
for mode in MODES3:                                                                               # plane_major: G = 8 only, tz passes: 5, 5, 5, 2
    case('interpn_tile<8,%d>' % mode, ex(*TILE_OTHER, 32, 5, mode, tune=(1 << 13) | (5 << 16)), MNAME[mode] + ' z-chunks of 5')
case('interpn_tile<8,1>', ex(*TILE_OTHER, 32, 5, tune=1 << 13), '17 passes')
case('interpn_tile<2,1>', ex(*TILE_SHAPE[8], 8, 5, tune=(1 << 13) | (5 << 16)), 'plane_major ignored at G=2')
case(UNSUPPORTED, ex(S3, O3, 32, 5, method=NEAREST), 'tile nearest')
for C in (8, 16):                                             # the auto choice: tiles from 4096 output voxels on, rows below
    case('interpn_tile<%d,1>' % (C // 4), Call('f32', (12, 10, 14), (16, 16, 16), C), 'auto 4096 voxels')
    case('interpn_rows<%d,1,0>' % (C // 4), Call('f32', (12, 10, 14), (7, 9, 65), C), 'auto 4095 voxels')

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_zrun_c32<MODE, WX, WY>: variant 3 forced
# ------------------------------------------------------------------------------------------------------------------------------
Z = (13, 10, 27)
ZT = wfo.zrun_tune
for patch, (WX, WY) in wfo.ZRUN_PATCH.items():
    for mode in MODES3:                                       # (Resize from another shape: on the identity grid linear is nearest)
        case('interpn_zrun_c32<%d,%d,%d>' % (mode, WX, WY), ex((9, 8, 14) if mode == LINSPACE else Z, Z, 32, 3, mode, tune=ZT(patch=patch)), MNAME[mode])
    case('interpn_zrun_c32<1,%d,%d>' % (WX, WY), ex((5, 7, 11), (3, 5, 9), 32, 3, tune=ZT(patch=patch)), 'smaller than a patch')
    for LZ, zo in ((5, 0), (5, 1), (40, 0)):                 # 27 = 5 x 5 + 2; 40 > O[2]: the whole z
        case('interpn_zrun_c32<1,%d,%d>' % (WX, WY), ex(Z, Z, 32, 3, tune=ZT(LZ, zo, patch)), 'tune LZ %d' % LZ)
for patch, lreg, B in ((3, 1, 1), (3, 1, 3), (3, 2, 3), (1, 2, 1), (1, 2, 3), (0, 2, 3), (2, 1, 3)):  # region order: the batch folded into grid.x
    WX, WY = wfo.ZRUN_PATCH[patch]
    case('interpn_zrun_c32<1,%d,%d>' % (WX, WY), ex(Z, Z, 32, 3, tune=ZT(5, 0, patch, lreg), B=B), 'B%d' % B)
for patch, lds_kb in ((0, 40), (0, 64), (2, 40), (2, 64)):                                        # the dynamic-LDS cap; > 48 KB: hipFuncSetAttribute
    WX, WY = wfo.ZRUN_PATCH[patch]
    case('interpn_zrun_c32<1,%d,%d>' % (WX, WY), ex(Z, Z, 32, 3, tune=ZT(5, 0, patch, 1, lds_kb)), '')
case('interpn_zrun_c32<2,4,2>', Call('f32', S3, (13, 11, 9), 32, LINSPACE), 'auto Resize')
case(UNSUPPORTED, ex(S3, O3, 16, 3), 'z-run C=16')
case(UNSUPPORTED, ex(S3, O3, 32, 3, method=NEAREST), 'z-run nearest')

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_generic<D, MODE, METHOD, T>: variant 1 forced, the auto fallbacks, nrt_interpn_nearest_i32
# ------------------------------------------------------------------------------------------------------------------------------
LOW = {1: ((6,), (4093,)), 2: ((9, 8), (7, 6)), 3: (S3, O3)}
for D in (1, 2, 3):
    for mode in MODES3:
        for method in (LINEAR, NEAREST):
            case('interpn_generic<%d,%d,%d,float>' % (D, mode, method), ex(*LOW[D], 5, 1, mode, method), '%s %s' % (MNAME[mode], METH[method]))
        case('interpn_generic<%d,%d,1,int>' % (D, mode), Call('i32', *LOW[D], 5, mode, NEAREST, 'i32'), MNAME[mode] + ' int32 C=5')
case('interpn_generic<3,1,0,float>', Call('f32', S3, O3, 5), 'auto C=5')
case('interpn_generic<3,1,0,float>', Call('f32', S3, O3, 32, vol_off=4), 'auto C=32 vol+4B')
case('interpn_generic<3,1,1,int>', Call('i32', S3, O3, 2, SHIFT, NEAREST, 'i32', loc_off=4), 'int32 C=2 loc+4B')
case('interpn_generic<3,2,1,int>', Call('i32', S3, (13, 11, 9), 2, LINSPACE, NEAREST, 'i32'), 'int32 C=2 LINSPACE')
# past the grid cap of 4096 blocks: 1.31 M elements, every thread of the first 1024 blocks takes a second one
case('interpn_generic<3,1,0,float>', Call('f32', (20, 20, 20), (64, 64, 64), 5, B=1), 'second pass', light=True)

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_lean_tile<C, MODE, METHOD>: auto at 1..4 channels, nrt_interpn_nearest_i32, nrt_interpn_add_f32
# ------------------------------------------------------------------------------------------------------------------------------
for C in (1, 2, 3, 4):
    for mode in (ABSOLUTE, SHIFT):
        case('interpn_lean_tile<%d,%d,0>' % (C, mode), ex(S3, O3, C, 8, mode), MNAME[mode] + ' variant 8')
        case('interpn_lean_tile<%d,%d,1>' % (C, mode), Call('f32', S3, O3, C, mode, NEAREST), MNAME[mode] + ' auto')
        case('interpn_lean_tile<%d,%d,2>' % (C, mode), Call('i32', S3, O3, C, mode, NEAREST, 'i32'), MNAME[mode] + ' int32')
# the ltz / lty trade of short extents (ltz starts at 5 for C = 1, at 4 for linear C >= 2)
for O in ((5, 37, 70), (7, 6, 17), (7, 6, 16), (7, 6, 3), (7, 6, 1), (7, 2, 7), (7, 1, 7)):
    for C in (1, 3):
        case('interpn_lean_tile<%d,1,0>' % C, Call('f32', (9, 10, 7) if O[1] == 2 else S3, O, C), '%dx%dx%d' % O)   # (two y samples sit on both borders)
# tiles per block of C = 1: 4 while (ntiles / tpb) batch >= 2048, else halved; 1395 tiles, an odd count: the last block is short
for B in (8, 4):
    case('interpn_lean_tile<1,1,0>', Call('f32', (13, 12, 14), (62, 60, 65), 1, B=B, shared_loc=True), 'B%d shared loc' % B, light=True)
# the addend epilogue (compose / VecInt); an addend stride that is no multiple of 4 floats goes to interpn_generic with the addend
for C in (1, 2, 3, 4):
    for pad in (0, 2):
        lean = (294 * C + pad) % 4 == 0
        case('interpn_lean_tile<%d,1,0>' % C if lean else 'interpn_generic<3,1,0,float>', Call('add', S3, O3, C, add_pad=pad), 'C=%d addend stride %d' % (C, 294 * C + pad))
case('interpn_lean_tile<2,0,0>', Call('add', S3, O3, 2, ABSOLUTE), 'ABSOLUTE')
case('interpn_generic<3,1,0,float>', Call('add', S3, O3, 4, add_off=4), 'C=4 addend+4B')
case('interpn_generic<2,1,0,float>', Call('add', (9, 8), (7, 6), 2), 'rank 2')
case('interpn_generic<3,2,0,float>', Call('add', S3, (13, 11, 9), 5, LINSPACE), 'C=5 LINSPACE')

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_lean<C, VPL, LINSPACE>: Resize of 1..4 channels
# ------------------------------------------------------------------------------------------------------------------------------
VPL_OF = {8: {1: 4, 2: 4, 3: 4, 4: 4}, 6: {1: 1, 2: 2, 3: 1, 4: 1}, 7: {1: 1, 2: 1, 3: 1, 4: 1}}
for z in (8, 6, 7):
    for C in (1, 2, 3, 4):
        case('interpn_lean<%d,%d,2>' % (C, VPL_OF[z][C]), Call('f32', S3, (13, 11, z), C, LINSPACE), 'up')
for C in (1, 2, 3, 4):
    case('interpn_lean<%d,4,2>' % C, Call('f32', (17, 15, 16), (9, 8, 8), C, LINSPACE), 'down')
    case('interpn_lean<%d,4,2>' % C, Call('f32', (8, 8, 9), (3, 3, 4), C, LINSPACE), 'one group per row')          # lpr == 1
    case('interpn_lean<%d,4,2>' % C, Call('f32', (4, 50, 5), (3, 130, 8), C, LINSPACE), 'two chunks per plane')    # cpp == 2
    case('interpn_lean<%d,1,2>' % C, Call('f32', (4, 50, 5), (3, 40, 7), C, LINSPACE), 'two chunks per plane')
    case('interpn_lean<%d,1,2>' % C, Call('f32', (8, 8, 3), (5, 6, 1), C, LINSPACE), 'one group per row')
case('interpn_lean<2,2,2>', Call('f32', (8, 8, 4), (5, 6, 2), 2, LINSPACE), 'one group per row')
case('interpn_lean<1,1,2>', Call('f32', S3, (13, 11, 8), 1, LINSPACE, loc_pad=1), 'location stride % 4 = 3')
case('interpn_lean<2,1,2>', Call('f32', S3, (13, 11, 6), 2, LINSPACE, loc_pad=1), 'location stride odd')
for C, z in ((1, 8), (3, 8), (2, 6), (4, 7)):
    case('interpn_lean<%d,%d,2>' % (C, VPL_OF[z][C]), Call('add', S3, (13, 11, z), C, LINSPACE), '')
case('interpn_generic<3,2,0,float>', Call('add', S3, (13, 11, 7), 2, LINSPACE), 'C=2 addend stride 2002')

# ------------------------------------------------------------------------------------------------------------------------------
# interpn_any_nd<T, NEAREST, D, CG>, interpn_any<T, NEAREST>, interpn_any_nearest_i32: nrt_interpn_any
# ------------------------------------------------------------------------------------------------------------------------------
TN = wfo.TNAME
NEAR = {LINEAR: 'false', NEAREST: 'true'}
R4, R5 = ((12, 11, 10, 9), (6, 5, 6, 5)), ((10, 9, 8, 7, 9), (5, 4, 5, 4, 5))
R4_ONE = (R4[0], (6, 5, 1, 5))                                # an output axis of one sample: linspace gives 0 there
REASONS = (('vol+16B', dict(vol_off=16)), ('out+16B', dict(out_off=16)), ('vol stride rows C + 2', dict(vol_pad=2)))
for dt in ('f32', 'f64', 'f16', 'bf16'):
    for method in (LINEAR, NEAREST):
        for D in (1, 2, 3):
            # CG = 4 with a shift and on a regular grid; CG = 1 for each reason with absolute locations or a shift: every instance sees the fields
            case('interpn_any_nd<%s,%s,%d,4>' % (TN[dt], NEAR[method], D), Call('any', *LOW[D], 8, SHIFT, method, dt), 'C=8 SHIFT ' + METH[method])
            case('interpn_any_nd<%s,%s,%d,4>' % (TN[dt], NEAR[method], D), Call('any', *LOW[D], 8, LINSPACE, method, dt), 'C=8 LINSPACE ' + METH[method])
            case('interpn_any_nd<%s,%s,%d,1>' % (TN[dt], NEAR[method], D), Call('any', *LOW[D], 6, ABSOLUTE, method, dt), 'C=6 ABSOLUTE ' + METH[method])
            for label, kw in REASONS:
                case('interpn_any_nd<%s,%s,%d,1>' % (TN[dt], NEAR[method], D), Call('any', *LOW[D], 8, SHIFT, method, dt, **kw), 'C=8 %s %s' % (label, METH[method]))
        case('interpn_any_nd<%s,%s,3,1>' % (TN[dt], NEAR[method]), Call('any', S3, (13, 11, 9), 6, LINSPACE, method, dt), 'C=6 LINSPACE ' + METH[method])
    for (S, O), method in ((R4, LINEAR), (R5, NEAREST), (R4, NEAREST), (R5, LINEAR)):
        mode = ABSOLUTE if len(S) == 4 else SHIFT
        case('interpn_any<%s,%s>' % (TN[dt], NEAR[method]), Call('any', S, O, 3, mode, method, dt), '%s %s' % (MNAME[mode], METH[method]))
    case('interpn_any<%s,false>' % TN[dt], Call('any', *R4, 3, LINSPACE, LINEAR, dt), 'LINSPACE linear')
    case('interpn_any<%s,true>' % TN[dt], Call('any', *R4_ONE, 3, LINSPACE, NEAREST, dt), 'LINSPACE nearest')
    case('interpn_any<%s,false>' % TN[dt], Call('any', *R4_ONE, 3, LINSPACE, LINEAR, dt), 'LINSPACE linear, one sample on an axis')
case('interpn_any_nd<double,false,3,4>', Call('any', S3, O3, 8, ABSOLUTE, LINEAR, 'f64', loc_f64=True), 'float64 locations')
case('interpn_any_nd<double,true,2,1>', Call('any', (9, 8), (7, 6), 3, ABSOLUTE, NEAREST, 'f64', loc_f64=True), 'float64 locations')
case(INVALID_ARG, Call('any', S3, O3, 8, ABSOLUTE, LINEAR, 'f32', loc_f64=True), 'float64 locations, float32 volume')
case(INVALID_ARG, Call('any', S3, O3, 8, SHIFT, LINEAR, 'f64', loc_f64=True), 'float64 locations, SHIFT')
case(INVALID_ARG, Call('any', S3, O3, 8, LINSPACE, LINEAR, 'f64', loc_f64=True), 'float64 locations, LINSPACE')
for C in (12, 20):                                            # the auto route of nrt_interpn_f32 for multiples of 4 off the row kernels
    for method in (LINEAR, NEAREST):
        case('interpn_any_nd<float,%s,3,4>' % NEAR[method], Call('f32', S3, O3, C, SHIFT, method), 'auto C=%d %s' % (C, METH[method]))
case('interpn_any_nearest_i32', Call('any', *R4, 3, SHIFT, NEAREST, 'i32'), '')
case('interpn_any_nearest_i32', Call('any', S3, O3, 3, ABSOLUTE, NEAREST, 'i32'), '')
case('interpn_any_nearest_i32', Call('any', *R4_ONE, 3, LINSPACE, NEAREST, 'i32'), 'LINSPACE')
case(UNSUPPORTED, Call('any', *R4, 3, SHIFT, LINEAR, 'i32'), 'int32 linear')

IDS = [(wfo.plan_id(wfo.plan(c.call)) + ' ' + c.label).strip() for c in CASES]


def subcalls(c):
    """the launches of a case: (call, field kind, fill)"""
    if c.light:
        return [(c.call, 'smooth', True), (c.call, 'incoherent', False)]
    return wfo.subcalls(c.call)


# ------------------------------------------------------------------------------------------------------------------------------
# buffers, the launch, the comparison
# ------------------------------------------------------------------------------------------------------------------------------
NPDT = {'f32': F, 'f64': np.float64, 'f16': np.float16, 'bf16': np.uint16, 'i32': np.int32}
DT = {'f32': _lib.DT_F32, 'f64': _lib.DT_F64, 'f16': _lib.DT_F16, 'bf16': _lib.DT_BF16, 'i32': _lib.DT_I32}
STATUS = {UNSUPPORTED: _lib.NRT_ERR_UNSUPPORTED, INVALID_ARG: _lib.NRT_ERR_INVALID_ARG}
GAP = 77                                        # what the elements between two batch entries of a padded stride hold


def storage(a, dtype):
    """the oracle's array as the bytes the kernel reads (bfloat16: the upper halves of the float32 values)"""
    a = np.ascontiguousarray(a)
    return (a.view(np.uint32) >> 16).astype(np.uint16) if dtype == 'bf16' else a.astype(NPDT[dtype])


def strided(x, bs, dt):
    """x [B, ...] laid out with batch stride bs (0: a single entry)"""
    n = x[0].size
    flat = np.full((x.shape[0] - 1) * bs + n, GAP, dt)
    for b in range(x.shape[0]):
        flat[b * bs:b * bs + n] = x[b].reshape(-1)
    return flat


class Mem:
    """a guarded device buffer whose payload starts `off` bytes (0 .. 31) after a 32-byte boundary: arm_buffers.Buf for float32 at
    0 or 4 bytes, else arm_buffers.Raw (from 16 bytes on its first 16 payload bytes become guard bytes too)"""

    def __init__(self, dev, data=None, nbytes=0, off=0, raw=False):
        if data is not None:
            nbytes = data.nbytes
        self.buf = None
        if not raw and off in (0, 4) and (data is None or data.dtype == F):
            self.buf = Buf(dev, nbytes // 4, off // 4, data)
            self.addr = self.buf.t.data_ptr()
        else:
            self.lead = 16 if off >= 16 else 0
            if data is not None:
                data = np.concatenate([np.full(self.lead, Raw.MARK, np.uint8), np.frombuffer(data.tobytes(), np.uint8)])
            self.raw = Raw(dev, nbytes + self.lead, off - self.lead, data)
            self.addr = self.raw.t.data_ptr() + self.lead
        assert self.addr % 32 == off, (self.addr, off)

    @property
    def p(self):
        return ctypes.c_void_p(self.addr)

    def get(self, dtype, shape):
        if self.buf is not None:
            return self.buf.get(shape)
        b = self.raw.get(np.uint8)
        assert (b[:self.lead] == Raw.MARK).all(), 'a write outside the output'
        return np.frombuffer(b[self.lead:].tobytes(), dtype).reshape(shape)

    def untouched(self):
        return self.raw.untouched()


def launch(dev, c, inp, fill, expect=None):
    """the call on guarded buffers; returns the output [B, *O, C] in the oracle's array type, or (expect: a status) asserts that the
    call returns it and that not one byte of the output was written"""
    raw = c.entry in ('any', 'i32') or expect is not None
    dt = NPDT[c.dtype]
    vb = Mem(dev, strided(storage(inp.vol, c.dtype), c.vol_bs, dt), off=c.vol_off, raw=raw)
    lb = None
    if inp.loc is not None:
        lb = Mem(dev, strided(inp.loc, c.loc_bs, np.float64 if c.loc_f64 else F), off=c.loc_off, raw=raw)
    ab = None if inp.addend is None else Mem(dev, strided(inp.addend, c.add_bs, F), off=c.add_off, raw=raw)
    ob = Mem(dev, nbytes=c.B * c.nout * c.C * dt().itemsize, off=c.out_off, raw=raw)
    head = (vb.p, None if lb is None else lb.p)
    shape = (c.D, _lib.ints(c.S), _lib.ints(c.O), c.C, c.B, c.vol_bs, c.loc_bs)
    if c.entry in ('f32', 'f32_ex'):
        name = 'nrt_interpn_' + c.entry
        args = head + (ob.p,) + shape + (c.mode, c.method, int(fill), wfo.FILL_F) + ((c.variant, c.tune) if c.entry == 'f32_ex' else ())
    elif c.entry == 'add':
        name = 'nrt_interpn_add_f32'
        args = head + (ab.p, ob.p) + shape + (c.add_bs, c.mode, int(fill), wfo.FILL_F)
    elif c.entry == 'i32':
        name = 'nrt_interpn_nearest_i32'
        args = head + (ob.p,) + shape + (c.mode, int(fill), wfo.FILL_I)
    else:
        name = 'nrt_interpn_any'
        args = head + (ob.p, DT[c.dtype]) + shape + (c.mode, int(c.loc_f64), c.method, int(fill), float(wfo.FILL_I if c.dtype == 'i32' else wfo.FILL_F))
    if expect is not None:
        with torch.cuda.device(dev):
            assert getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev)) == STATUS[expect]
            torch.cuda.synchronize(dev)
        assert ob.untouched(), 'a refused call wrote to the output'
        return None
    call(dev, name, *args)
    got = ob.get(dt, (c.B,) + tuple(c.O) + (c.C,))
    return (got.astype(np.uint32) << 16).view(F) if c.dtype == 'bf16' else got


def same_bits(got, ref):
    if ref.dtype == F:
        return bits_equal(got, ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)


@pytest.mark.parametrize('n', range(len(CASES)), ids=IDS)
def test_arm(dev, n):
    """ids: see the module docstring; the case table above says what each one is there for"""
    cs = CASES[n]
    p = wfo.plan(cs.call)
    if p.status:
        assert p.status == cs.want
        launch(dev, cs.call, wfo.inputs(cs.call, 'grid' if cs.call.mode == LINSPACE else 'smooth', True, with_refs=False), True, expect=p.status)
        return
    assert p.names == (cs.want,), (p, cs.want)
    for c, kind, fill in subcalls(cs):
        inp = wfo.inputs(c, kind, fill)
        got = launch(dev, c, inp, fill)
        for b in range(c.B):
            ref = inp.refs[b]
            if not same_bits(got[b], ref):
                bad = np.argwhere(~((got[b] == ref) | (np.isnan(got[b].astype(np.float64)) & np.isnan(ref.astype(np.float64)))))
                raise AssertionError('%s: %s fill %d B %d shared loc %d vol %d, entry %d: %d of %d elements differ, first at %s: got %r, reference %r'
                                     % (IDS[n], kind, fill, c.B, c.shared_loc, c.shared_vol, b, len(bad), ref.size, tuple(bad[0]) if len(bad) else '(sign of zero)',
                                        got[b][tuple(bad[0])] if len(bad) else None, ref[tuple(bad[0])] if len(bad) else None))
