// interpn, linear, 3-D, 1..4 channels (images, displacement fields): the instruction-lean kernel (variant 8).
//
// With 4..16 bytes per voxel the warp of an image or of a flow field (SpatialTransformer on C = 1 images, Resize(2) of the
// C = 3 deformation at neurite/tf/models.py:804, VecInt / compose) is not bound by HBM but by instruction issue: the
// LDS-staged kernel (variant 6) spends ~450 issue slots per voxel on bounding boxes, the box copy with its divisions and
// 64-bit addresses (0.23-0.25 of the HBM roof at 160^3, profiles/archive/r01_session50).  Here nothing is staged: the source of a
// few-channel volume is small (16 MB at 160^3 x 1) and neighbouring lanes read neighbouring addresses, so the 8 corner
// reads are L1 / L2 hits; what is left is the reference's arithmetic, strength-reduced:
//   * a lane owns VPL consecutive-z output voxels (4 at C = 1, 2 at C = 2): x, y and their corner arithmetic are
//     computed once per lane, the location is read with 16-byte loads, the result written with one 16-byte store;
//   * blocks are laid out over (x-plane, chunk of the plane): the only division left is one multiply-high per lane;
//   * tf.clip_by_value is one v_med3_f32, every corner address a 32-bit byte offset from a uniform base (one add per
//     corner), channels of a corner one 4/8/12/16-byte load.
// Same float32 op sequence as interpn_generic (one rounding per op, corners in itertools.product order) => bit-identical
// results (tests/test_gpu_interpn.py); optional fill and addend epilogue (VecInt / compose).

#include "interpn_core.h"
#include "lean.h"
#include "lean_core.h"

namespace {

template <int C, int VPL, int MODE>
__global__ __launch_bounds__(256) void interpn_lean(InterpArgs a, unsigned lpr, unsigned m_lpr, unsigned cpp, unsigned nblk) {
    const unsigned logical = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (logical >= nblk) return;
    const unsigned x = logical / cpp, chunk = logical - x * cpp;          // uniform: scalar ALU
    // XPOSE (more than 16 contiguous bytes per lane, e.g. 3 channels x 4 voxels = 48): the results leave through LDS so that every store
    // instruction writes 16 consecutive bytes per lane -- stored straight from the lanes, the 16-byte pieces are 48 bytes apart,
    // every line is written by three instructions and Resize(2) of 4 x 80^3 x 3 ran at 0.089 ms instead of 0.072
    constexpr int NF = VPL * C;                                           // floats a lane produces
    constexpr bool XPOSE = NF > 4 && NF % 4 == 0;
    __shared__ __attribute__((aligned(16))) float s_out[XPOSE ? 256 * NF : 4];
    const unsigned glim = (unsigned)a.O[1] * lpr;
    unsigned g = chunk * 256u + threadIdx.x;                              // group of VPL voxels inside the x-plane
    const bool lane_valid = g < glim;
    if (!XPOSE && !lane_valid) return;
    if (!lane_valid) g = glim - 1u;                                       // XPOSE: the lane computes a repeat and stores nothing
    const unsigned y = lpr == 1u ? g : __umulhi(g, m_lpr);                // g / lpr, exact for g * lpr < 2^32 (checked on the host)
    const unsigned z0 = (g - y * lpr) * (unsigned)VPL;
    const int b = blockIdx.y;
    const char *vol = (const char *)((const float *)a.vol + (long long)b * a.vol_bs);
    const float *locb = a.loc ? a.loc + (long long)b * a.loc_bs : nullptr;
    float *out = (float *)a.out + (long long)b * a.out_bs;
    const unsigned q0 = nrt_mad24(nrt_mad24(x, (unsigned)a.O[1], y), (unsigned)a.O[2], z0);

    // ---- locations of the VPL voxels -----------------------------------------------------------------------------
    float raw[VPL * 3];
    if (MODE != NRT_LOC_LINSPACE) {
        const float *lp = locb + (size_t)q0 * 3u;
        if constexpr (VPL == 4) {
            const nrt_f4 t0 = ((const nrt_f4 *)lp)[0], t1 = ((const nrt_f4 *)lp)[1], t2 = ((const nrt_f4 *)lp)[2];
            raw[0] = t0[0]; raw[1] = t0[1]; raw[2] = t0[2]; raw[3] = t0[3];
            raw[4] = t1[0]; raw[5] = t1[1]; raw[6] = t1[2]; raw[7] = t1[3];
            raw[8] = t2[0]; raw[9] = t2[1]; raw[10] = t2[2]; raw[11] = t2[3];
        } else if constexpr (VPL == 2) {
            const nrt_f2 t0 = ((const nrt_f2 *)lp)[0], t1 = ((const nrt_f2 *)lp)[1], t2 = ((const nrt_f2 *)lp)[2];
            raw[0] = t0[0]; raw[1] = t0[1]; raw[2] = t1[0]; raw[3] = t1[1]; raw[4] = t2[0]; raw[5] = t2[1];
        } else {
            raw[0] = lp[0]; raw[1] = lp[1]; raw[2] = lp[2];
        }
    }
    // ---- x and y: shared by the lane's voxels unless the location is per voxel ---------------------------------------
    const float mxx = (float)(a.S[0] - 1), mxy = (float)(a.S[1] - 1), mxz = (float)(a.S[2] - 1);
    const unsigned SY = (unsigned)a.S[1], SZ = (unsigned)a.S[2];
    const unsigned str_x = SY * SZ * (unsigned)(C * 4), str_y = SZ * (unsigned)(C * 4), str_z = (unsigned)(C * 4);
    float res[VPL][C];
    auto linspace = [&](int d, int qv) -> float {        // tf.linspace(0, S - 1, O): the ends exact, delta * i between them
        return (qv == 0) ? 0.0f : ((qv == a.O[d] - 1) ? (float)(a.S[d] - 1) : nrt_mul(a.delta[d], (float)qv));
    };
    // regular grids: the lane's voxels share x and y -- their corner arithmetic, x*y weight products and row base are formed once
    // (written out: the compiler does not merge the copies of the unrolled loop)
    float spx = 0.0f, spy = 0.0f, sw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned sbase = 0u, ssx = 0u, ssy = 0u;
    if (MODE == NRT_LOC_LINSPACE) {
        spx = linspace(0, (int)x);
        spy = linspace(1, (int)y);
        int ix, iy, ux, uy;
        float w0x, w1x, w0y, w1y;
        lean_corner(spx, mxx, a.S[0] - 1, ix, ux, w0x, w1x);
        lean_corner(spy, mxy, a.S[1] - 1, iy, uy, w0y, w1y);
        sw[0] = nrt_mul(w0x, w0y); sw[1] = nrt_mul(w0x, w1y); sw[2] = nrt_mul(w1x, w0y); sw[3] = nrt_mul(w1x, w1y);
        sbase = nrt_mad24(nrt_mad24((unsigned)ix, SY, (unsigned)iy), SZ, 0u) * (unsigned)(C * 4);
        ssx = ux ? str_x : 0u;
        ssy = uy ? str_y : 0u;
    }
    // regular grids, several voxels per lane: the z locations of a lane's voxels rise monotonically, so consecutive voxels sit in the
    // same source cell or in the next one; the (x, y) rows' values at z = c_lo and z = c_hi stay in registers and only what changed
    // is loaded (Resize(2): 12 corner loads per 4 voxels instead of 32 -- the texture-address unit is what these kernels wait for)
    constexpr bool ZCACHE = MODE == NRT_LOC_LINSPACE && VPL > 1;
    float c_lo[4][C], c_hi[4][C];
    int z_lo = -1, z_hi = -1, zp_held = -1;
    float c_pair[4][2 * C];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        const int qd[3] = {(int)x, (int)y, (int)z0 + k};
        float p[3];
        int iz, uz;
        float w0z, w1z, wxy[4];
        unsigned base, sx, sy;
        if (MODE == NRT_LOC_LINSPACE) {
            p[0] = spx; p[1] = spy; p[2] = linspace(2, qd[2]);
            lean_corner(p[2], mxz, a.S[2] - 1, iz, uz, w0z, w1z);
            base = sbase + (unsigned)iz * (unsigned)(C * 4);
            sx = ssx; sy = ssy;
#pragma unroll
            for (int j = 0; j < 4; ++j) wxy[j] = sw[j];
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) p[d] = MODE == NRT_LOC_ABSOLUTE ? raw[3 * k + d] : nrt_add((float)qd[d], raw[3 * k + d]);
            int ix, iy, ux, uy;
            float w0x, w1x, w0y, w1y;
            lean_corner(p[0], mxx, a.S[0] - 1, ix, ux, w0x, w1x);
            lean_corner(p[1], mxy, a.S[1] - 1, iy, uy, w0y, w1y);
            lean_corner(p[2], mxz, a.S[2] - 1, iz, uz, w0z, w1z);
            base = nrt_mad24(nrt_mad24((unsigned)ix, SY, (unsigned)iy), SZ, (unsigned)iz) * (unsigned)(C * 4);
            sx = ux ? str_x : 0u; sy = uy ? str_y : 0u;
            // (w_x * w_y) * w_z: the x*y products are shared by the two z corners (the rounding sequence of prod_n)
            wxy[0] = nrt_mul(w0x, w0y); wxy[1] = nrt_mul(w0x, w1y); wxy[2] = nrt_mul(w1x, w0y); wxy[3] = nrt_mul(w1x, w1y);
        }
        const unsigned sz = uz ? str_z : 0u;
        float v[8][C];
        bool paired = false;
        if constexpr (C <= 2) paired = a.S[2] >= 2;                      // uniform; a 1-voxel z extent has no pair to load
        if (paired) {
            // the two z corners of an (x, y) row by ONE load of 2 C floats (as the tile form below does): half the lane accesses
            // the texture-address unit has to serve.  At the upper border the pair starts one voxel earlier.
            const unsigned izp = (unsigned)min(iz, a.S[2] - 2);
            const bool second = (unsigned)iz != izp;
            const unsigned pbase = base - ((unsigned)iz - izp) * (unsigned)(C * 4);
            if (!ZCACHE || (int)izp != zp_held) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    load_c<(C <= 2 ? 2 * C : C)>(vol, pbase + ((r & 2) ? sx : 0u) + ((r & 1) ? sy : 0u),
                                                 (float (&)[(C <= 2 ? 2 * C : C)])c_pair[r]);
                zp_held = (int)izp;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float lo_v = second ? c_pair[r][C + c] : c_pair[r][c];
                    v[2 * r][c] = lo_v;
                    v[2 * r + 1][c] = uz ? c_pair[r][C + c] : lo_v;
                }
        } else if (ZCACHE) {
            const int zu = iz + uz;                                      // the upper corner's plane
            if (iz != z_lo) {
                if (iz == z_hi) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < C; ++c) c_lo[r][c] = c_hi[r][c];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) load_c<C>(vol, base + ((r & 2) ? sx : 0u) + ((r & 1) ? sy : 0u), c_lo[r]);
                }
                z_lo = iz;
            }
            if (zu != z_hi) {
                if (zu == z_lo) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < C; ++c) c_hi[r][c] = c_lo[r][c];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) load_c<C>(vol, base + ((r & 2) ? sx : 0u) + ((r & 1) ? sy : 0u) + sz, c_hi[r]);
                }
                z_hi = zu;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c) { v[2 * r][c] = c_lo[r][c]; v[2 * r + 1][c] = c_hi[r][c]; }
        } else {
#pragma unroll
            for (int corner = 0; corner < 8; ++corner)
                load_c<C>(vol, base + ((corner & 4) ? sx : 0u) + ((corner & 2) ? sy : 0u) + ((corner & 1) ? sz : 0u), v[corner]);
        }
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;                       // :160
        // (channel pairs as 2-vectors -- v_pk_mul_f32 / v_pk_add_f32 -- were measured: 10-14 % fewer instructions, no gain at C = 2 / 3
        // and 68 -> 76 us at C = 4)
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const float wt = nrt_mul(wxy[corner >> 1], (corner & 1) ? w1z : w0z);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = nrt_add(acc[c], nrt_mul(wt, v[corner][c]));     // :191
        }
        if (a.has_fill) {
            const bool oob = (p[0] < 0.0f) || (p[0] > mxx) || (p[1] < 0.0f) || (p[1] > mxy) || (p[2] < 0.0f) || (p[2] > mxz);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = apply_fill(acc[c], oob, a.fill_f);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) res[k][c] = acc[c];
    }
    // ---- epilogue: optional addend, one vector store per lane ---------------------------------------------------------
    float *po = out + (size_t)q0 * (unsigned)C;
    if (a.addend) {
        const float *pa = a.addend + (long long)b * a.addend_bs + (size_t)q0 * (unsigned)C;
#pragma unroll
        for (int k = 0; k < VPL; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) res[k][c] = nrt_add(pa[k * C + c], res[k][c]);
    }
    if constexpr (XPOSE) {
        // the block's groups are consecutive in memory: lane t's NF floats are floats [NF t, NF (t + 1)) of the block's run
        const float *r = &res[0][0];
#pragma unroll
        for (int j = 0; j < NF / 4; ++j)
            ((nrt_f4 *)s_out)[threadIdx.x * (unsigned)(NF / 4) + j] = (nrt_f4){r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]};
        __syncthreads();
        const unsigned first = chunk * 256u;                              // first group of the block
        const unsigned ngrp = min(256u, glim - first);
        const unsigned y0b = lpr == 1u ? first : __umulhi(first, m_lpr);
        const unsigned qb = nrt_mad24(nrt_mad24(x, (unsigned)a.O[1], y0b), (unsigned)a.O[2], (first - y0b * lpr) * (unsigned)VPL);
        nrt_f4 *ob = (nrt_f4 *)(out + (size_t)qb * (unsigned)C);
#pragma unroll
        for (int j = 0; j < NF / 4; ++j) {
            const unsigned e = threadIdx.x + 256u * (unsigned)j;          // 16-byte chunk of the run
            if (e < ngrp * (unsigned)(NF / 4)) __builtin_nontemporal_store(((const nrt_f4 *)s_out)[e], ob + e);
        }
    } else if constexpr (VPL * C == 4) {
        const float *r = &res[0][0];
        *(nrt_f4 *)po = (nrt_f4){r[0], r[1], r[2], r[3]};
    } else if constexpr (VPL * C == 2) {
        *(nrt_f2 *)po = (nrt_f2){res[0][0], res[VPL - 1][C - 1]};
    } else if constexpr ((VPL * C) % 4 == 0) {
        const float *r = &res[0][0];                                     // e.g. 4 voxels x 3 channels: 48 contiguous bytes
#pragma unroll
        for (int j = 0; j < VPL * C / 4; ++j) ((nrt_f4 *)po)[j] = (nrt_f4){r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]};
    } else {
#pragma unroll
        for (int k = 0; k < VPL; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) po[k * C + c] = res[k][c];
    }
}

// ---- tile form (per-voxel locations: ABSOLUTE / SHIFT) ---------------------------------------------------------------------
// With a displacement field every voxel has its own location, so several voxels per lane share nothing, and lanes that are
// 4 voxels apart in z make every corner read touch 2.5x the cache lines (measured: 0.29 ms against 0.18 ms of the LDS kernel
// for 4 x 160^3 x 1).  Here a lane owns ONE voxel and a block a compact 2 x 4 x 32 (x, y, z) tile: a wave reads two 32-voxel
// z-runs per corner (3-4 lines), and the tile's source box is ~110 lines that stay in L1 / L2 for the tile's 8 corner reads.
// METHOD: 0 linear; 1 nearest on float32 data; 2 nearest on int32 data (utils.py:193-204: one gathered element per channel; the
// fill arithmetic runs in the volume's dtype)
template <int C, int MODE, int METHOD = 0>
__global__ __launch_bounds__(256) void interpn_lean_tile(InterpArgs a, int ltz, int lty, unsigned nTy, unsigned nTz, unsigned ntiles,
                                                         unsigned tpb, unsigned nblk) {
    // a block walks `tpb` consecutive tiles (z fastest): the scalar set-up is paid once, the tile index advances without
    // divisions, and the location of the next tile's voxel is requested before the current tile's corners are blended
    const unsigned blk = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (blk >= nblk) return;
    const int ltx = 8 - ltz - lty;
    unsigned tile = blk * tpb;
    const unsigned tend = min(tile + tpb, ntiles);
    unsigned tzi = tile % nTz, t2 = tile / nTz;                              // uniform: scalar ALU, once per block
    unsigned tyi = t2 % nTy, txi = t2 / nTy;
    const unsigned l = threadIdx.x;
    const int lx = (int)(l >> (ltz + lty)), ly = (int)((l >> ltz) & ((1u << lty) - 1u)), lz = (int)(l & ((1u << ltz) - 1u));
    const int b = blockIdx.y;
    const char *vol = (const char *)((const float *)a.vol + (long long)b * a.vol_bs);
    const char *locb = (const char *)(a.loc + (long long)b * a.loc_bs);
    float *out = (float *)a.out + (long long)b * a.out_bs;
    const float *addb = a.addend ? a.addend + (long long)b * a.addend_bs : nullptr;
    const float mxx = (float)(a.S[0] - 1), mxy = (float)(a.S[1] - 1), mxz = (float)(a.S[2] - 1);
    const unsigned SY = (unsigned)a.S[1], SZ = (unsigned)a.S[2];
    const unsigned str_x = SY * SZ * (unsigned)(C * 4), str_y = SZ * (unsigned)(C * 4), str_z = (unsigned)(C * 4);
    const int O0 = a.O[0], O1 = a.O[1], O2 = a.O[2];

    auto coords = [&](unsigned cx, unsigned cy, unsigned cz, int (&qd)[3], bool &valid) {
        qd[0] = (int)(cx << ltx) + lx; qd[1] = (int)(cy << lty) + ly; qd[2] = (int)(cz << ltz) + lz;
        valid = qd[0] < O0 && qd[1] < O1 && qd[2] < O2;
        qd[0] = min(qd[0], O0 - 1); qd[1] = min(qd[1], O1 - 1); qd[2] = min(qd[2], O2 - 1);            // loads stay unconditional
    };
    auto flat = [&](const int (&qd)[3]) {
        return nrt_mad24(nrt_mad24((unsigned)qd[0], (unsigned)O1, (unsigned)qd[1]), (unsigned)O2, (unsigned)qd[2]);
    };
    int qd[3];
    bool valid;
    coords(txi, tyi, tzi, qd, valid);
    unsigned q = flat(qd);
    float pn[3];
    {
        const float *lp = (const float *)(locb + (size_t)(nrt_times3(q) << 2));
        pn[0] = lp[0]; pn[1] = lp[1]; pn[2] = lp[2];
    }
    for (; tile < tend; ++tile) {
        float p[3] = {pn[0], pn[1], pn[2]};
        const int cq[3] = {qd[0], qd[1], qd[2]};
        const unsigned cqf = q;
        const bool cvalid = valid;
        // next tile (clamped to the last one of this block: its location load is then a repeat, never out of range)
        if (tile + 1 < tend) {
            if (++tzi == nTz) { tzi = 0; if (++tyi == nTy) { tyi = 0; ++txi; } }
            coords(txi, tyi, tzi, qd, valid);
            q = flat(qd);
        }
        {
            const float *lp = (const float *)(locb + (size_t)(nrt_times3(q) << 2));
            pn[0] = lp[0]; pn[1] = lp[1]; pn[2] = lp[2];
        }
        if (MODE == NRT_LOC_SHIFT) {
#pragma unroll
            for (int d = 0; d < 3; ++d) p[d] = nrt_add((float)cq[d], p[d]);
        }
        if constexpr (METHOD != 0) {
            const unsigned ri = nrt_mad24(nrt_mad24((unsigned)nearest_1d(p[0], a.S[0]), SY, (unsigned)nearest_1d(p[1], a.S[1])), SZ,
                                          (unsigned)nearest_1d(p[2], a.S[2])) * (unsigned)(C * 4);
            float v[C];
            load_c<C>(vol, ri, v);
            if (a.has_fill) {
                const bool oob = (p[0] < 0.0f) || (p[0] > mxx) || (p[1] < 0.0f) || (p[1] > mxy) || (p[2] < 0.0f) || (p[2] > mxz);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if (METHOD == 1) v[c] = apply_fill(v[c], oob, a.fill_f);
                    else v[c] = __int_as_float(__float_as_int(v[c]) * (oob ? 0 : 1) + (oob ? 1 : 0) * a.fill_i);
                }
            }
            if (cvalid) {
                float *po = out + (size_t)cqf * (unsigned)C;
                if constexpr (C == 4) __builtin_nontemporal_store((nrt_f4){v[0], v[1], v[2], v[3]}, (nrt_f4 *)po);
                else if constexpr (C == 2) __builtin_nontemporal_store((nrt_f2){v[0], v[1]}, (nrt_f2 *)po);
                else {
#pragma unroll
                    for (int c = 0; c < C; ++c) __builtin_nontemporal_store(v[c], po + c);
                }
            }
            continue;
        }
        int ix, iy, iz, ux, uy, uz;
        float w0x, w1x, w0y, w1y, w0z, w1z;
        lean_corner(p[0], mxx, a.S[0] - 1, ix, ux, w0x, w1x);
        lean_corner(p[1], mxy, a.S[1] - 1, iy, uy, w0y, w1y);
        lean_corner(p[2], mxz, a.S[2] - 1, iz, uz, w0z, w1z);
        const float wxy[4] = {nrt_mul(w0x, w0y), nrt_mul(w0x, w1y), nrt_mul(w1x, w0y), nrt_mul(w1x, w1y)};
        const unsigned sx = ux ? str_x : 0u, sy = uy ? str_y : 0u, sz = uz ? str_z : 0u;
        float v[8][C];
        bool paired = false;
        if constexpr (C <= 2) paired = a.S[2] >= 2;                      // uniform; a 1-voxel z extent has no pair to load
        if (paired) {
            // The texture-address unit spends ~1 cycle per LANE of a gather whose lanes are not consecutive (measured: 8.07 cache
            // accesses per voxel, TA busy 88 %, profiles/archive/r02_smallc): the two z corners of an (x, y) row are neighbours in
            // memory, so ONE load of 2 C floats fetches both -- 4 lane accesses per voxel instead of 8.  At the upper border
            // (z1 == z0 == SZ - 1) the pair starts one voxel earlier and both corners take its second half.
            const unsigned izp = (unsigned)min(iz, a.S[2] - 2);
            const bool second = (unsigned)iz != izp;                     // the lower corner is the pair's upper half
            const unsigned base = nrt_mad24(nrt_mad24((unsigned)ix, SY, (unsigned)iy), SZ, izp) * (unsigned)(C * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t[2 * C];
                load_c<(C <= 2 ? 2 * C : C)>(vol, base + ((r & 2) ? sx : 0u) + ((r & 1) ? sy : 0u), (float (&)[(C <= 2 ? 2 * C : C)])t);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float lo_v = second ? t[C + c] : t[c];
                    v[2 * r][c] = lo_v;
                    v[2 * r + 1][c] = uz ? t[C + c] : lo_v;
                }
            }
        } else {
            const unsigned base = nrt_mad24(nrt_mad24((unsigned)ix, SY, (unsigned)iy), SZ, (unsigned)iz) * (unsigned)(C * 4);
#pragma unroll
            for (int corner = 0; corner < 8; ++corner)
                load_c<C>(vol, base + ((corner & 4) ? sx : 0u) + ((corner & 2) ? sy : 0u) + ((corner & 1) ? sz : 0u), v[corner]);
        }
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;                       // :160
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const float wt = nrt_mul(wxy[corner >> 1], (corner & 1) ? w1z : w0z);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = nrt_add(acc[c], nrt_mul(wt, v[corner][c]));     // :191
        }
        if (a.has_fill) {
            const bool oob = (p[0] < 0.0f) || (p[0] > mxx) || (p[1] < 0.0f) || (p[1] > mxy) || (p[2] < 0.0f) || (p[2] > mxz);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = apply_fill(acc[c], oob, a.fill_f);
        }
        if (addb) {
            const float *pa = addb + (size_t)cqf * (unsigned)C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = nrt_add(pa[c], acc[c]);
        }
        if (cvalid) {
            float *po = out + (size_t)cqf * (unsigned)C;
            if constexpr (C == 4) __builtin_nontemporal_store((nrt_f4){acc[0], acc[1], acc[2], acc[3]}, (nrt_f4 *)po);
            else if constexpr (C == 2) __builtin_nontemporal_store((nrt_f2){acc[0], acc[1]}, (nrt_f2 *)po);
            else {
                // C = 3: three 4-byte stores measured faster than one 12-byte store (0.331 vs 0.347 ms, 4 x 160^3 x 3)
#pragma unroll
                for (int c = 0; c < C; ++c) __builtin_nontemporal_store(acc[c], po + c);
            }
        }
    }
}

template <int C>
void launch_lean_tile(const InterpArgs &a, int batch, int mode, int method_kind, hipStream_t st) {
    // 2 x 4 x 32 tiles (a wave: two 32-voxel z-runs); linear interpolation of 2..4 channels: 8 x 2 x 16 (a wave: 2 x 2 x 16), whose
    // corner loads touch fewer distinct lines per instruction (measured at 4 x 160^3: C = 2 0.206 -> 0.186 ms,
    // C = 3 0.299 -> 0.263, C = 4 0.344 -> 0.297; C = 1 0.117 -> 0.136).  Short z extents trade z for y / x
    int ltz = 5, lty = 2;
    if (C >= 2 && method_kind == 0) { ltz = 4; lty = 1; }
    while (ltz > 0 && (1 << (ltz - 1)) >= a.O[2]) { --ltz; ++lty; }
    while (lty > 0 && (1 << (lty - 1)) >= a.O[1]) --lty;
    const int ltx = 8 - ltz - lty;
    const unsigned nTx = (a.O[0] + (1 << ltx) - 1) >> ltx, nTy = (a.O[1] + (1 << lty) - 1) >> lty, nTz = (a.O[2] + (1 << ltz) - 1) >> ltz;
    const unsigned ntiles = nTx * nTy * nTz;
    // tiles per block, measured at 4 x 160^3: C = 1 0.176 / 0.169 / 0.173 ms at 1 / 4 / 8; C = 3 0.298 / 0.323 / 0.331
    unsigned tpb = C == 1 ? 4u : 1u;
    while (tpb > 1 && (ntiles / tpb) * (unsigned)batch < 2048u) tpb >>= 1;     // keep the chip full on small volumes
    const unsigned nblk = (ntiles + tpb - 1) / tpb;
    dim3 grid(nrt_xcd_grid(nblk), batch), blk(256);
#define NRT_TILE_LAUNCH(MODE)                                                                                                    \
    switch (method_kind) {                                                                                                       \
        case 1: hipLaunchKernelGGL((interpn_lean_tile<C, MODE, 1>), grid, blk, 0, st, a, ltz, lty, nTy, nTz, ntiles, tpb, nblk); break; \
        case 2: hipLaunchKernelGGL((interpn_lean_tile<C, MODE, 2>), grid, blk, 0, st, a, ltz, lty, nTy, nTz, ntiles, tpb, nblk); break; \
        default: hipLaunchKernelGGL((interpn_lean_tile<C, MODE, 0>), grid, blk, 0, st, a, ltz, lty, nTy, nTz, ntiles, tpb, nblk); break; \
    }
    if (mode == NRT_LOC_ABSOLUTE) { NRT_TILE_LAUNCH(NRT_LOC_ABSOLUTE) }
    else { NRT_TILE_LAUNCH(NRT_LOC_SHIFT) }
#undef NRT_TILE_LAUNCH
}

template <int C, int VPL>
void launch_lean_cv(const InterpArgs &a, int batch, int mode, hipStream_t st) {
    const unsigned lpr = (unsigned)a.O[2] / VPL;
    const unsigned m_lpr = lpr == 1 ? 0u : (unsigned)(0x100000000ull / lpr) + 1u;
    const unsigned groups = (unsigned)a.O[1] * lpr;
    const unsigned cpp = (groups + 255u) / 256u;
    const unsigned nblk = cpp * (unsigned)a.O[0];
    dim3 grid(nrt_xcd_grid(nblk), batch), blk(256);
    if (lpr == 1) {
        // g / 1: the multiply-high constant would overflow; lpr == 1 means one group per row (y = g)
        switch (mode) {
            case NRT_LOC_ABSOLUTE: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_ABSOLUTE>), grid, blk, 0, st, a, 1u, 0u, cpp, nblk); break;
            case NRT_LOC_SHIFT: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_SHIFT>), grid, blk, 0, st, a, 1u, 0u, cpp, nblk); break;
            default: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_LINSPACE>), grid, blk, 0, st, a, 1u, 0u, cpp, nblk); break;
        }
        return;
    }
    switch (mode) {
        case NRT_LOC_ABSOLUTE: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_ABSOLUTE>), grid, blk, 0, st, a, lpr, m_lpr, cpp, nblk); break;
        case NRT_LOC_SHIFT: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_SHIFT>), grid, blk, 0, st, a, lpr, m_lpr, cpp, nblk); break;
        default: hipLaunchKernelGGL((interpn_lean<C, VPL, NRT_LOC_LINSPACE>), grid, blk, 0, st, a, lpr, m_lpr, cpp, nblk); break;
    }
}

}  // namespace

// the kernel addresses the source with 32-bit byte offsets and 24-bit multiplies, and divides the in-plane group index by a
// multiply-high that is exact while groups * lanes-per-row < 2^32
bool nrt_lean_supported(const int *vol_shape, const int *out_shape, int channels, int ndim, const void *vol, const void *loc,
                        const void *out, long long vol_bs, long long loc_bs) {
    if (ndim != 3 || channels < 1 || channels > 4) return false;
    unsigned long long vbytes = 4ull * channels;
    for (int d = 0; d < 3; ++d) {
        if (vol_shape[d] < 1 || out_shape[d] < 1 || vol_shape[d] >= (1 << 12) || out_shape[d] >= (1 << 12)) return false;
        vbytes *= (unsigned long long)vol_shape[d];
    }
    if (vbytes >= (1ull << 32)) return false;
    // 32-bit byte offsets into the location field (12 B per output voxel) and into the output / addend rows (4 C B per voxel)
    const unsigned long long nout = (unsigned long long)out_shape[0] * out_shape[1] * out_shape[2];
    if (nout * 12ull >= (1ull << 32) || nout * 4ull * (unsigned long long)channels >= (1ull << 32)) return false;
    // vector accesses: C floats per source voxel, VPL * C per output group, VPL * 3 per location group.  Bases must be
    // 16-byte aligned; the batch strides keep the alignment the channel count needs (the per-lane vector widths over z are
    // chosen at launch from the z extent and the location stride)
    if ((((uintptr_t)vol | (uintptr_t)out | (uintptr_t)loc) & 15) != 0) return false;
    const int valign = channels == 4 ? 16 : (channels == 2 ? 8 : 4);
    if ((vol_bs * 4) % valign != 0) return false;
    (void)loc_bs;
    return true;
}

int nrt_lean_launch(const void *args, int batch, int mode, int method_kind, void *stream) {
    const InterpArgs &a = *(const InterpArgs *)args;
    hipStream_t st = nrt_stream(stream);
    if (mode != NRT_LOC_LINSPACE) {           // per-voxel locations: one voxel per lane, compact tiles
        switch (a.C) {
            case 1: launch_lean_tile<1>(a, batch, mode, method_kind, st); break;
            case 2: launch_lean_tile<2>(a, batch, mode, method_kind, st); break;
            case 3: launch_lean_tile<3>(a, batch, mode, method_kind, st); break;
            default: launch_lean_tile<4>(a, batch, mode, method_kind, st); break;
        }
        NRT_CHECK_LAUNCH();
        return NRT_OK;
    }
    if (method_kind != 0) return NRT_ERR_UNSUPPORTED;      // the row form (regular grids) is linear only
    switch (a.C) {
        case 1:
            // 4 voxels per lane: 16-byte location loads and stores need z % 4 == 0 (then nout % 4 == 0 and the contiguous batch
            // strides of loc / out / addend are multiples of 16 bytes too; a foreign loc stride is checked)
            if (a.O[2] % 4 == 0 && (a.loc_bs * 4) % 16 == 0 && (a.addend_bs * 4) % 16 == 0) launch_lean_cv<1, 4>(a, batch, mode, st);
            else launch_lean_cv<1, 1>(a, batch, mode, st);
            break;
        case 2:
            if (mode == NRT_LOC_LINSPACE && a.O[2] % 4 == 0 && (a.out_bs * 4) % 16 == 0) launch_lean_cv<2, 4>(a, batch, mode, st);
            else if (a.O[2] % 2 == 0 && (a.loc_bs * 4) % 8 == 0 && (a.addend_bs * 4) % 16 == 0) launch_lean_cv<2, 2>(a, batch, mode, st);
            else launch_lean_cv<2, 1>(a, batch, mode, st);
            break;
        // C = 2 .. 4 on regular grids: four voxels per lane (the x / y corner arithmetic is shared), results transposed through LDS
        case 3:
            if (mode == NRT_LOC_LINSPACE && a.O[2] % 4 == 0 && (a.out_bs * 4) % 16 == 0) launch_lean_cv<3, 4>(a, batch, mode, st);
            else launch_lean_cv<3, 1>(a, batch, mode, st);
            break;
        default:
            if (mode == NRT_LOC_LINSPACE && a.O[2] % 4 == 0) launch_lean_cv<4, 4>(a, batch, mode, st);
            else launch_lean_cv<4, 1>(a, batch, mode, st);
            break;
    }
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
