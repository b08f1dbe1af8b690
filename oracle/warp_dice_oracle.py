"""
TEST INFRASTRUCTURE ONLY -- the host dispatch of the fused warp + soft Dice forward (neurite_amd/csrc/fused.hip, fused_wc.h and the
schedules of interpn_core.h: fused_geom, tile_geometry, xmarch_setup, xmarch_setup_mixed, fused_choose / wc_applies, wc_persistent),
restated, and the float64 reference of what the kernels return, for tests/test_gpu_warp_dice_arms.py and
tests/test_warp_dice_oracle.py.  numpy only; the number of compute units is an argument (the schedules of the x-march depend on it).

plan(call, cus) returns {'status': ...} for a call the entry point refuses before any launch, or

  instance      the template instance as tools/arm_coverage.norm spells the profiler's name: warp_dice_tile<G,MODE,STORE,MINW,ST>,
                warp_dice_tile_pad<...> (Gr = L / 4 live lanes of G) or warp_dice_wc<MODE,STORE,MM,FILL,DICE,PERSIST>
  schedule      'tile', 'xmarch' (equal pieces, xmarch_setup) or 'mixed' (whole columns and pieces, xmarch_setup_mixed)
  tile          ext (tile extents), npass, z_outer, plane_major, tz, nT (tiles per axis), tiles (8 per2 nTz, idle ones included),
                idle (tiles of the XCD slabs with t2 >= nT2), grid, per_block (tiles a block walks: > 1 under the 2048-block cap),
                partial (the axes with a partial tile)
  xmarch/mixed  patch (widened: fused_geom raised lty until the patch holds the 256 / G voxels of a pass), region, ncol, padcol
                (padding columns of the regions: empty blocks), nseg, seglen, ragged (planes of the last piece), het_cpx, het_full, items_x, prows, padrows (per batch entry: rows xmarch_zero_rows has to fill), short
                (columns missing from the last XCD's list), passes_per_plane, wc, persist, grid
  nblocks       partial rows per batch entry: what sizes the workspace
  ws            workspace_bytes(nblocks, L, B)

`tags(plan)` is the text an id carries after the instance.

Reference (soft_ref).  The kernels claim: warped = the float32 blend of interpn.hip, bit for bit (oracle.warp_fwd_oracle.reference,
which adds no arithmetic to oracle.c_oracle.interpn), then sum t p, sum t^2, sum p^2 over the voxels of a batch entry
(neurite/tf/metrics.py:476-477) and the extrema of both maps over the whole launch.  soft_ref forms these sums in float64 from `fixed`
and the REFERENCE's float32 `warped`: nothing of it comes from the device.

Bound of the random run (u = 2^-24, first order in u as in oracle/dice_cce_oracle.py).  An element of `sums` is a sum of n terms,
n = the voxels of a batch entry.  A term is ONE float32 product of two float32 values (t and the float32 warped value p, which the
device holds with the reference's bits -- asserted wherever it is stored): one rounding, u |term|, so k = 1.  The terms are then added
in float32 in some tree: lane accumulators, the xor-shuffle tree of a wave, four waves through LDS -- at most n - 1 additions of
non-zero values whatever the schedule, each rounding a partial sum that is at most A = sum |term| (dead lanes of the padded kernels,
clamped voxels of partial tiles and padding rows add +0, which rounds nothing).  The block partials are added in float64 (reduce_rows
and dice_soft_finalize: no rounding that matters at 2^-53) and the result is converted to float32 once.  Together
    |got - ref| <= (n - 1 + 1 + k) u A = (n + 1) u A,      k = 1,
the bound of the unfused soft Dice.  The bfloat16 entry point widens stored values exactly and runs the same float32 arithmetic: the
same bound on the widened maps.

Exact run.  Maps of small integers, locations on a lattice with dyadic weights (one axis of a voxel on a quarter step, the others on
half steps or integers): every weight product is a multiple of 2^-4, p of 2^-4, t p of 2^-4 and p^2 of 2^-8, every partial sum of the
blend and of the Dice terms is exact while the sum of absolute terms stays below 2^24 units of 2^-8 (assert_exact), and then `sums`
equals the float64 reference bit for bit in any order of addition.
"""

import dataclasses

import numpy as np

from . import warp_fwd_oracle as wfo

F, D = np.float32, np.float64
U = 2.0 ** -24
ABSOLUTE, SHIFT, LINSPACE = 0, 1, 2
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
NXCD, MAX_BLOCKS, RED_ROWS = 8, 2048, 64
FUSED_SYNC, FUSED_MINW = 8, 3
FUSED_DEFAULT = 3 | (3 << 4) | (4 << 8)                         # 8 x 8 x 16 tiles
XM_DEFAULT = 3 | (2 << 4) | (3 << 8) | (1 << 14) | (3 << 24) | (1 << 27)
TUNE_WC, TUNE_NO_WC = 1 << 29, 1 << 30
ST = {'f32': 'float', 'bf16': 'unsignedshort'}
ELEM = {'f32': 4, 'bf16': 2}
cdiv = wfo.cdiv


def tune_word(ltx=3, lty=3, ltz=4, z_outer=0, plane_major=0, x_march=0, nseg=0, lry=0, lrz=0, zchunk=0):
    """the tune word of the fused entry points; bits 16.. are the z-chunk of plane_major or the segment count of the x-march"""
    return ltx | lty << 4 | ltz << 8 | z_outer << 12 | plane_major << 13 | x_march << 14 | (zchunk if plane_major else nseg) << 16 | lry << 24 | lrz << 27


@dataclasses.dataclass(frozen=True)
class Call:
    """one call of nrt_warp_dice_soft_f32 / _bf16 (entry 'dice') or of nrt_interpn_f32_ex variant 10 (entry 'interpn': the wave-cache
    kernel without its Dice half).  *_off: bytes between a 16-byte boundary and the pointer; null: names of pointers passed as NULL;
    ws_short: bytes missing from the workspace"""
    L: int
    S: tuple
    O: tuple
    B: int = 1
    mode: int = SHIFT
    dtype: str = 'f32'
    store: bool = False
    minmax: bool = True
    fill: bool = False
    tune: int = 0
    shared_loc: bool = False
    entry: str = 'dice'
    mov_off: int = 0
    fix_off: int = 0
    warped_off: int = 0
    null: tuple = ()
    ws_short: int = 0

    @property
    def nout(self):
        return int(np.prod(self.O))

    @property
    def rows(self):
        return int(np.prod(self.S))


def fused_group(L):
    if L < 4 or L > 256 or L % 4:
        return 0
    g = 1
    while g < L // 4:
        g <<= 1
    return g


def fused_fits(S, O, L, elem):
    if S[0] * S[1] >= 1 << 24 or S[2] >= 1 << 24 or O[0] * O[1] >= 1 << 24 or O[2] >= 1 << 24:
        return False
    return int(np.prod(S, dtype=object)) * L * elem < 1 << 32 and int(np.prod(O, dtype=object)) * L * 4 < 1 << 32


def workspace_bytes(nblocks, L, B):
    """fused_ws_bytes: the float32 partial rows and their extrema, 16 bytes of alignment, the float64 group sums and their extrema"""
    rows, grp = B * nblocks, B * cdiv(nblocks, RED_ROWS)
    return rows * 3 * L * 4 + rows * 4 * 4 + 16 + grp * 3 * L * 8 + grp * 4 * 4 + 256


def xmarch_applies(O, B):
    return wfo.xmarch_applies(O, B)


def split_before(het_cpx, het_full, c):
    cl = c % het_cpx
    return (c // het_cpx) * (het_cpx - het_full) + (cl - het_full if cl > het_full else 0)


def _xm_common(O, B, t, g):
    lry, lrz = (t >> 24) & 7, (t >> 27) & 7
    RY, RZ = 1 << lry, 1 << lrz
    nTy, nTz = g['nT'][1], g['nT'][2]
    ncol = cdiv(nTy, RY) * cdiv(nTz, RZ) * RY * RZ
    return dict(lry=lry, lrz=lrz, ncol=ncol, padcol=ncol - nTy * nTz)


def xmarch_setup(O, B, t, g):
    """equal pieces (an explicit segment count; the auto count of xmarch_setup is not reachable from fused_geom)"""
    x = _xm_common(O, B, t, g)
    nseg = (t >> 16) & 0xff
    assert nseg > 0
    nseg = min(nseg, O[0])
    seglen = cdiv(O[0], nseg)
    nseg = cdiv(O[0], seglen)
    x.update(nseg=nseg, seglen=seglen, het_cpx=0, het_full=0, items_x=cdiv(x['ncol'] * nseg * B, NXCD), prows=x['ncol'] * nseg,
             padrows=(0,) * B, short=0)
    return x


PS = (1, 2, 3, 4, 5, 6, 8)
OVH = tuple(F(v) for v in (0.0, 0.07, 0.11, 0.15, 0.17, 0.19, 0.22))


def xmarch_setup_mixed(O, B, t, g, cus):
    """whole columns for the full rounds of 2 CUs / 8 blocks per XCD, pieces for the rest: the cost model in its float32 arithmetic"""
    x = _xm_common(O, B, t, g)
    cols = x['ncol'] * B
    cpx = cdiv(cols, NXCD)
    slots = max(1, 2 * cus // NXCD)
    best, bF, bP = F(1e30), 0, 1
    for Fw in range(0, cpx + 1, slots):
        rem = cpx - Fw
        for i, P in enumerate(PS):
            if P > O[0]:
                break
            cost = F(Fw // slots) + (F(F(F(cdiv(rem * P, slots)) / F(P)) * F(F(1) + OVH[i])) if rem else F(0))
            if cost < F(best - F(1e-6)):
                best, bF, bP = cost, Fw, P
            if not rem:
                break
    seglen = cdiv(O[0], bP)
    sp = [split_before(cpx, bF, min((b + 1) * x['ncol'], cols)) - split_before(cpx, bF, b * x['ncol']) for b in range(B)]
    prows = x['ncol'] + max(sp) * (bP - 1)
    x.update(nseg=bP, seglen=seglen, het_cpx=cpx, het_full=bF, items_x=bF + (cpx - bF) * bP, prows=prows,
             padrows=tuple(prows - (x['ncol'] + s * (bP - 1)) for s in sp), split=tuple(sp), short=NXCD * cpx - cols)
    return x


def fused_geom(O, G, B, tune, cus):
    """fused_geom: the geometry and the partial rows per batch entry"""
    g = wfo.tile_geometry(O, G, tune, FUSED_DEFAULT)
    nblocks = min(g['ntiles'], MAX_BLOCKS)
    t = 0 if tune <= 0 else tune
    if t == 0 and G == 8 and xmarch_applies(O, B):
        t = XM_DEFAULT
        g = wfo.tile_geometry(O, G, t, t)
        nblocks = g['ntiles']
    widened = False
    if (t >> 14) & 1 and not g['plane_major']:
        # a pass is 256 / G voxels of one patch: a patch that holds fewer is widened along y (else npass = xlen patch / NG rounds down)
        lty = g['lty']
        while (1 << (lty + g['ltz'])) < 256 // G:
            lty += 1
        if lty != g['lty']:
            t = (t & ~((15 << 4) | (15 << 8))) | lty << 4 | g['ltz'] << 8
            g = wfo.tile_geometry(O, G, t, t)
            nblocks = min(g['ntiles'], MAX_BLOCKS)
            widened = True
    g['widened'] = widened
    xm = None
    if (t >> 14) & 1 and not g['plane_major'] and O[0] > 0:
        if (t >> 16) & 0xff == 0:
            xm = dict(xmarch_setup_mixed(O, B, t, g, cus), schedule='mixed')
        else:
            xm = dict(xmarch_setup(O, B, t, g), schedule='xmarch')
        nblocks = xm['prows']
    return g, xm, nblocks


def wc_applies(g, xm, G, S):
    return xm is not None and G == 8 and g['lty'] == 2 and g['ltz'] == 3 and not g['plane_major'] and S[0] * S[1] * S[2] * 128 < 0xffffff00


def _b(v):
    return 'true' if v else 'false'


def _status(c):
    """the checks of warp_dice_soft_impl in their order (the workspace comes last, in plan)"""
    if {'fixed', 'sums', 'dice'} & set(c.null):
        return ERR_INVALID_ARG
    if not fused_group(c.L):
        return ERR_UNSUPPORTED
    if 'moving' in c.null or c.B < 1 or c.mode not in (0, 1, 2) or (c.mode != LINSPACE and 'loc' in c.null):
        return ERR_INVALID_ARG
    if c.B > 65535:
        return ERR_UNSUPPORTED
    if any(s < 1 for s in c.S) or any(o < 0 for o in c.O):
        return ERR_INVALID_ARG
    if c.rows * c.L >= 1 << 40 or c.nout >= 1 << 31:
        return ERR_UNSUPPORTED
    if not fused_fits(c.S, c.O, c.L, ELEM[c.dtype]):
        return ERR_UNSUPPORTED
    if c.dtype != 'f32' and c.store:
        return ERR_UNSUPPORTED
    if (c.mov_off | c.fix_off | (c.warped_off if c.store else 0)) & 15:
        return ERR_INVALID_ARG
    if c.nout == 0:
        return ERR_INVALID_ARG
    return None


def plan(c, cus=256):
    if c.entry == 'interpn':
        return _plan_interpn(c, cus)
    st = _status(c)
    if st is not None:
        return dict(status=st)
    G, Gr = fused_group(c.L), c.L // 4
    allow_wc = not (c.tune > 0 and c.tune & TUNE_NO_WC)
    tune = c.tune & ~(TUNE_NO_WC | TUNE_WC) if c.tune > 0 else c.tune
    g, xm, nblocks = fused_geom(c.O, G, c.B, tune, cus)
    ws = workspace_bytes(nblocks, c.L, c.B)
    if c.ws_short > 0:
        return dict(status=ERR_WORKSPACE, ws=ws)
    p = dict(G=G, Gr=Gr, nblocks=nblocks, ws=ws, n=c.nout)
    wc = G == 8 and Gr == 8 and c.dtype == 'f32' and allow_wc and wc_applies(g, xm, G, c.S)
    NG = 256 // G
    if xm is None:
        ext = (1 << g['ltx'], 1 << g['lty'], g['tz'])
        nT2 = g['nT'][0] * g['nT'][1]
        per = cdiv(nT2, NXCD) * g['nT'][2]
        p.update(schedule='tile', ext=ext, npass=g['npass'], z_outer=g['z_outer'], plane_major=g['plane_major'], tz=g['tz'], nT=g['nT'],
                 tiles=g['ntiles'], idle=g['ntiles'] - nT2 * g['nT'][2], grid=nblocks, per_block=cdiv(per, nblocks // NXCD),
                 partial=''.join(n for n, o, e in zip('xyz', c.O, ext) if o % e), wc=False, persist=False)
    else:
        patch = (1 << g['lty']) * (1 << g['ltz'])
        assert patch % NG == 0                                   # (fused_geom has widened a smaller patch)
        persist = wc and NXCD * xm['items_x'] > 2 * cus
        grid = (NXCD * cdiv(2 * cus, NXCD) if persist else NXCD * xm['items_x']) if (wc or xm['het_cpx']) else NXCD * cdiv(nblocks * c.B, NXCD)
        p.update(xm, patch=(1 << g['lty'], 1 << g['ltz']), region=(1 << xm['lry'], 1 << xm['lrz']), nT=g['nT'],
                 ragged=c.O[0] - (xm['nseg'] - 1) * xm['seglen'], passes_per_plane=patch // NG, widened=g['widened'], wc=wc, persist=persist, grid=grid,
                 partial=''.join(n for n, o, e in zip('yz', c.O[1:], (1 << g['lty'], 1 << g['ltz'])) if o % e))
    if Gr != G:
        p['instance'] = 'warp_dice_tile_pad<%d,%d,%s,%d,%s>' % (G, c.mode, _b(c.store), FUSED_MINW if xm else 1, ST[c.dtype])
    elif wc:
        p['instance'] = 'warp_dice_wc<%d,%s,%s,%s,true,%s>' % (c.mode, _b(c.store), _b(c.minmax), _b(c.fill), _b(p['persist']))
    else:
        p['instance'] = 'warp_dice_tile<%d,%d,%s,%d,%s>' % (G, c.mode, _b(c.store), FUSED_MINW if xm else 1, ST[c.dtype])
    return p


def _plan_interpn(c, cus):
    """nrt_interpn_f32_ex with variant 10: fill_args, then can_zrun and nrt_wc_interpn_supported, then the mixed schedule of the default
    x-march tune word"""
    if c.B < 1 or c.mode not in (0, 1, 2) or any(s < 1 for s in c.S):
        return dict(status=ERR_INVALID_ARG)
    if c.nout == 0:
        return dict(status=OK)
    can_zrun = c.L == 32 and not ((c.mov_off | c.warped_off) & 15) and 4 * c.L * c.rows < 1 << 32
    ok = can_zrun and xmarch_applies(c.O, c.B) and c.nout * 128 < 1 << 32 and fused_fits(c.S, c.O, 32, 4)
    if not ok:
        return dict(status=ERR_UNSUPPORTED)
    g = wfo.tile_geometry(c.O, 8, XM_DEFAULT, XM_DEFAULT)
    xm = dict(xmarch_setup_mixed(c.O, c.B, XM_DEFAULT, g, cus), schedule='mixed')
    if not wc_applies(g, xm, 8, c.S):
        return dict(status=ERR_UNSUPPORTED)
    persist = NXCD * xm['items_x'] > 2 * cus
    p = dict(xm, G=8, Gr=8, n=c.nout, patch=(4, 8), region=(1 << xm['lry'], 1 << xm['lrz']), nT=g['nT'], ragged=c.O[0] - (xm['nseg'] - 1) * xm['seglen'],
             passes_per_plane=1, widened=False, wc=True, persist=persist, grid=NXCD * cdiv(2 * cus, NXCD) if persist else NXCD * xm['items_x'],
             partial=''.join(n for n, o, e in zip('yz', c.O[1:], (4, 8)) if o % e), nblocks=xm['prows'], ws=0)
    p['instance'] = 'warp_dice_wc<%d,true,false,%s,false,%s>' % (c.mode, _b(c.fill), _b(persist))
    return p


def tags(p):
    """the geometry an id carries"""
    if 'status' in p:
        return ''
    if p['schedule'] == 'tile':
        return 'tile%dx%dx%d passes%d tiles%dx%dx%d idle%d grid%d x%d partial-%s%s%s' % (
            p['ext'] + (p['npass'],) + p['nT'] + (p['idle'], p['grid'], p['per_block'], p['partial'] or 'none',
                                                  ' z_outer' if p['z_outer'] else '', ' plane_major' if p['plane_major'] else ''))
    s = '%s patch%dx%d%s region%dx%d ncol%d+%d seg%dx%d ragged%d' % ((p['schedule'],) + p['patch'] + ('(widened)' if p['widened'] else '',) + p['region'] +
                                                                 (p['ncol'] - p['padcol'], p['padcol'], p['nseg'], p['seglen'], p['ragged']))
    if p['schedule'] == 'mixed':
        s += ' cpx%d full%d short%d prows%d padrows%s' % (p['het_cpx'], p['het_full'], p['short'], p['prows'], '/'.join(map(str, sorted(set(p['padrows'])))))
    s += ' items%d grid%d partial-%s' % (p['items_x'], p['grid'], p['partial'] or 'none')
    return s + (' persist' if p['persist'] else '')


# the instances no call can launch (profiles/dispatch_arms/README.md).  78: nrt_warp_dice_soft_bf16 has no `warped` parameter (it passes
# nullptr) and warp_dice_soft_impl refuses `warped` for 16-bit storage, so STORE = true never meets ST = unsigned short.  18 more: the
# padded entry point at G = 2 -- fused_group gives G = 2 for 8 labels only, where Gr = 2 = G, so launch_fused_any<2> never takes its
# padded branch (the other 6 of the 24 warp_dice_tile_pad<2, ...> are bfloat16 STORE = true already)
UNREACHABLE = sorted(['warp_dice_tile<%d,%d,true,%d,unsignedshort>' % (G, m, w) for G in (1, 2, 4, 8, 16, 32, 64) for m in (0, 1, 2) for w in (1, 3)] +
                     ['warp_dice_tile_pad<%d,%d,true,%d,unsignedshort>' % (G, m, w) for G in (4, 8, 16, 32, 64) for m in (0, 1, 2) for w in (1, 3)] +
                     ['warp_dice_tile_pad<2,%d,%s,%d,%s>' % (m, s, w, t) for m in (0, 1, 2) for s in ('false', 'true') for w in (1, 3) for t in ('float', 'unsignedshort')])


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------

def warp_ref(c, mov, loc, fill_value):
    """the bit-exact float32 warp of every batch entry: mov [B, *S, L] float32 values (bfloat16 storage: the widened values), loc
    [B or 1, *O, 3] or None"""
    out = []
    for b in range(c.B):
        lb = None if loc is None else loc[0 if c.shared_loc else b]
        a = wfo.locations(c.mode, c.S, c.O, lb)
        out.append((wfo.co.interpn(mov[b], a, 'linear', fill_value if c.fill else None, loc_mode=0), a))
    return np.stack([o[0] for o in out]), [o[1] for o in out]


def soft_ref(fixed, warped):
    """fixed, warped [B, *O, L] float32 values -> sums [B, 3, L] and A (sums of absolute terms) in float64, n, the extrema of the launch,
    and the per-voxel terms"""
    B, L = fixed.shape[0], fixed.shape[-1]
    sums, A, dyadic = [], [], True
    for b in range(B):                                                    # (entry by entry: the persistent cases have 10^5 voxels)
        t, p = fixed[b].astype(D).reshape(-1, L), warped[b].astype(D).reshape(-1, L)
        terms = np.stack([t * p, t * t, p * p])                           # [3, n, L]
        sums.append(terms.sum(1))
        A.append(np.abs(terms).sum(1))
        dyadic = dyadic and bool((terms * 256.0 == np.round(terms * 256.0)).all())
    return dict(sums=np.stack(sums), A=np.stack(A), n=int(np.prod(fixed.shape[1:-1])), k=1, dyadic=dyadic,
                minmax=np.array([fixed.min(), fixed.max(), warped.min(), warped.max()], D))


def assert_exact(r):
    """the premise of the exact run: every term a multiple of 2^-8, every sum of absolute terms below 2^24 of these units"""
    assert r['dyadic']
    assert (r['A'] * 256.0 < 2 ** 24).all(), r['A'].max() * 256.0


def extrema_unique(fixed, warped):
    """each of the four extrema sits in one voxel and label of the whole launch"""
    return all(int((m == f(m)).sum()) == 1 for m in (fixed, warped) for f in (np.min, np.max))


# ------------------------------------------------------------------------------------------------------------------------------
# the wave-private row cache of warp_dice_wc, modelled from the locations alone
# ------------------------------------------------------------------------------------------------------------------------------

DZT = (0, 2, 3, 1)


def wc_orphans(S, O, absloc, pieces):
    """orphan references per wave and pass of the wave-cache kernel on one batch entry (fused_wc.h, M1a - M1c): absloc [*O, 3] float32,
    pieces: the (x0, xlen) every column is marched in.  A wave owns a 2 x 4 sub-patch of a 4 x 8 patch, one voxel per 8-lane group and
    pass, lane p of a group the corner p of its voxel; slot = (ix & 3, iy & 3, iz & 7) of a direct-mapped cache of 128 rows that lives
    for one piece.  A reference whose slot names its row is served; the others claim the slot (the highest lane's claim stays) and
    whoever then finds another row's name there is an orphan.  More than 16 orphans: the pass forgets the cache.  Returns the counts."""
    mx = np.array(S, D) - 1
    out = []
    for cy in range(cdiv(O[1], 4)):
        for cz in range(cdiv(O[2], 8)):
            for wave in range(4):
                ys = [min(4 * cy + 2 * (wave >> 1) + (g >> 2), O[1] - 1) for g in range(8)]
                zs = [min(8 * cz + 4 * (wave & 1) + DZT[g & 3], O[2] - 1) for g in range(8)]
                for x0, xlen in pieces:
                    tags = {}
                    for x in range(x0, x0 + max(xlen, 0)):
                        cl = np.clip(absloc[x, ys, zs].astype(D), 0, mx)                       # [8, 3]
                        l0 = np.floor(cl)
                        l1 = np.minimum(l0 + 1, mx)
                        refs = []
                        for g in range(8):
                            for p in range(8):
                                i = [int((l1 if p & b else l0)[g, d]) for d, b in enumerate((4, 2, 1))]
                                refs.append(((i[0] * S[1] + i[1]) * S[2] + i[2], (i[0] & 3) << 5 | (i[1] & 3) << 3 | (i[2] & 7)))
                        before = dict(tags)
                        for rid, slot in refs:                                                  # claims in lane order: the last stays
                            if before.get(slot) != rid:
                                tags[slot] = rid
                        no = sum(tags[slot] != rid for rid, slot in refs)
                        if no > 16:
                            tags = {}
                        out.append(no)
    return np.array(out)
