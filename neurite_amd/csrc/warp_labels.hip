// Fused SpatialTransformer('linear') + soft Dice on integer LABEL MAPS, and its backward wrt the field.
//
// With M = one_hot(moving, L), F = one_hot(fixed, L) (float32; an id outside [0, L) gives an all-zero row) the results are those of
// nrt_warp_dice_soft_f32 / nrt_warp_dice_bwd_f32 on M and F, but neither one-hot tensor exists.  The tri-linear blend of
// utils.py:159-191 on 0/1 data is, per label, the sum of the weights of the corners that carry the label, added in corner order
// 000 ... 111 starting from 0 (fl(wt * 1) = wt, adding +0 changes nothing), so a voxel has at most 8 non-zero values: they follow
// from 8 gathered int32 ids and the 8 weights fl(fl(wx wy) wz).  Per output voxel that is 12 B of field, 4 B of fixed id and 8 id
// reads from a volume that fits the Infinity Cache, against 3 rows of L floats.
//
// forward (warp_labels_fwd)  one lane per output voxel, a block walks a contiguous range of voxels in steps of 256.  A lane merges equal
//   ids in corner order into at most 8 (id, p) slots (slot o belongs to the first corner with its id).  What is accumulated per (batch,
//   label) is sum p^2, sum t p (the slot whose id is the fixed id) and the count of the fixed id.  No atomics:
//     * every wave owns a table of 3 L floats in LDS.  Per step the wave loops over the DISTINCT ids among its lanes (ballot + readlane),
//       adds the matching lanes' terms by a butterfly (a fixed cross-lane order), and the k-th distinct id's totals are kept by lane k;
//       after the loop the lanes add their entries into the table side by side (the ids of one step are distinct: no two lanes meet).
//       Counts of the fixed id are popcounts of ballots (integers below 2^24: exact in float32 in any order).
//     * fast path: while all 64 lanes see eight equal corners of ONE id (the interior of every structure) the terms stay in per-lane
//       accumulators that belong to that id; they are added across the wave and into the table only when the id changes.
//     * the four wave tables are added in wave order into the block's workspace row; dice_reduce.h's second stage adds the rows in a
//       fixed order in float64 and forms dice.
//   Which path a step takes and when an accumulator is flushed depend on the data and the shapes only, so results are run-to-run
//   bit-identical.  An id outside [0, L) never indexes a table; gather indices come from corner_1d and are clamped by construction.
//   STORE: the dense warped row [L] per voxel from the same slots (bit-identical to interpn on the one-hot map).
// backward (warp_labels_bwd)  one lane per output voxel, the per-label coefficients of d dice / d p (two floats per label) in LDS.
//   d/d loc_d = sum over corners c of g(id_c) d wt_c / d loc_d with g(l) = ca_l [fixed == l] + cb_l p_l; no reduction.
#include "dice_reduce.h"
#include "wl_core.h"

namespace {

constexpr int WL_WAVES = WL_BLOCK / NRT_WAVE;
constexpr int WL_MAX_BLOCKS = 2048;          // per batch entry: 8 blocks per CU
constexpr int WL_MIN_STEPS = 4;              // a block walks at least this many steps of 256 voxels (where the volume has them)
constexpr int WL_MAX_LABELS = 256;

inline unsigned wl_num_blocks(unsigned nout) {
    unsigned long long nb = ((unsigned long long)nout + WL_BLOCK * WL_MIN_STEPS - 1) / (WL_BLOCK * WL_MIN_STEPS);
    if (nb > WL_MAX_BLOCKS) nb = WL_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    return (unsigned)nb;
}

inline size_t wl_ws_bytes(unsigned nblk, int L, int batch) {
    const size_t ngrp = (nblk + RED_ROWS - 1) / RED_ROWS;
    return (size_t)batch * nblk * 3 * L * sizeof(float) + 16 + (size_t)batch * ngrp * 3 * L * sizeof(double);
}

// grid (nrt_xcd_grid(nblk), batch); dynamic LDS WL_WAVES * 3 L floats; part [batch][nblk][3][L]
template <int MODE, bool STORE>
__global__ __launch_bounds__(WL_BLOCK) void warp_labels_fwd(InterpArgs a, const int *__restrict__ fixed, float *__restrict__ part, int L,
                                                            unsigned nblk, unsigned per, long long vol_n) {
    extern __shared__ float wl_tab[];                           // [WL_WAVES][3 L]: sum t p, count of t, sum p^2
    const unsigned blk = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (blk >= nblk) return;                                    // (block-uniform; such a block owns no row)
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (NRT_WAVE - 1), wave = tid / NRT_WAVE;
    const int L3 = 3 * L;
    for (int i = tid; i < WL_WAVES * L3; i += WL_BLOCK) wl_tab[i] = 0.0f;
    __syncthreads();
    volatile float *tab = wl_tab + wave * L3;
    const int *mov = (const int *)a.vol + (long long)b * vol_n;
    const float *locb = a.loc + (long long)b * a.loc_bs;
    const int *fixb = fixed + (long long)b * a.nout;
    float *outb = STORE ? (float *)a.out + (long long)b * a.nout * L : nullptr;

    const unsigned long long beg64 = (unsigned long long)blk * per;
    const unsigned beg = beg64 < a.nout ? (unsigned)beg64 : a.nout;
    const unsigned end = (unsigned long long)beg + per < a.nout ? beg + per : a.nout;

    int cur = -1;                                               // the id the per-lane accumulators belong to (wave-uniform)
    float acc_pp = 0.0f, acc_tp = 0.0f;
    auto flush = [&]() {
        if ((unsigned)cur < (unsigned)L) {
            const float pp = nrt_dpp_wave_sum(acc_pp), tp = nrt_dpp_wave_sum(acc_tp);
            if (lane == 0) {
                tab[cur] += tp;
                tab[2 * L + cur] += pp;
            }
        }
        acc_pp = 0.0f;
        acc_tp = 0.0f;
    };

    for (unsigned q0 = beg; q0 < end; q0 += WL_BLOCK) {         // (block-uniform trip count: every lane of a wave runs every step)
        const unsigned qq = q0 + (unsigned)tid;
        const bool live = qq < end;
        const unsigned q = live ? qq : a.nout - 1;
        int lab[8];
        float w0[3], w1[3], wt[8], p[NRT_MAXD];
        bool oob;
        wl_corners<MODE>(a, locb, mov, q, lab, w0, w1, p, oob);
        int fl = fixb[q];
        if (!live || (unsigned)fl >= (unsigned)L) fl = -1;
        wl_weights(w0, w1, wt);
        const bool zero = oob || !live;                         // fill 0: an out-of-bounds voxel has p = 0 for every label

        bool eq8 = true;
#pragma unroll
        for (int c = 1; c < 8; ++c) eq8 = eq8 && lab[c] == lab[0];
        const int l0u = __builtin_amdgcn_readfirstlane(lab[0]);
        const bool fast = __all(eq8 && lab[0] == l0u);

        float P[8];                                             // P[o]: the warped value of id lab[o] where corner o owns a slot
        unsigned own;
        if (fast) {
            float s = wt[0];
#pragma unroll
            for (int c = 1; c < 8; ++c) s = nrt_add(s, wt[c]);
            P[0] = zero ? 0.0f : s;
#pragma unroll
            for (int c = 1; c < 8; ++c) P[c] = 0.0f;
            own = 1u;
        } else {
            own = 0u;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                float s = wt[o];
                bool first = true;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    if (c < o) first = first && lab[c] != lab[o];
                    if (c > o) s = (lab[c] == lab[o]) ? nrt_add(s, wt[c]) : s;
                }
                P[o] = zero ? 0.0f : s;
                own |= first ? (1u << o) : 0u;
            }
        }

        if (STORE) {
            if (live) {
                float *row = outb + (long long)q * L;
                for (int c = 0; c < L; ++c) {
                    float v = 0.0f;
#pragma unroll
                    for (int o = 0; o < 8; ++o) v = (((own >> o) & 1u) && lab[o] == c) ? P[o] : v;
                    row[c] = v;
                }
            }
        }

        // ---- counts of the fixed id: the k-th distinct id of the step is kept by lane k ----
        {
            unsigned long long fm = __ballot(fl >= 0);
            int k = 0, kl = -1;
            float kc = 0.0f;
            while (fm) {
                const int src = __ffsll((long long)fm) - 1;
                const int l = __builtin_amdgcn_readlane(fl, src);
                const unsigned long long m = __ballot(fl == l);
                if (lane == k) { kl = l; kc = (float)__popcll(m); }
                ++k;
                fm &= ~m;
            }
            if (kl >= 0) tab[L + kl] += kc;
        }

        if (fast) {
            if (l0u != cur) {
                flush();
                cur = l0u;
            }
            if ((unsigned)l0u < (unsigned)L) {
                acc_pp = nrt_add(acc_pp, nrt_mul(P[0], P[0]));
                acc_tp = nrt_add(acc_tp, fl == l0u ? P[0] : 0.0f);
            }
        } else {
            // slots that are still to be added: sl[o] = id, or -1 (not an owner, an id outside [0, L), or done)
            int sl[8];
            unsigned pend = 0u;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const bool in = !zero && ((own >> o) & 1u) && (unsigned)lab[o] < (unsigned)L;
                sl[o] = in ? lab[o] : -1;
                pend |= in ? (1u << o) : 0u;
            }
            unsigned long long act = __ballot(pend != 0u);
            int k = 0, kl = -1;
            float kpp = 0.0f, ktp = 0.0f;
            while (act) {
                const int src = __ffsll((long long)act) - 1;
                const int firstslot = __ffs((int)pend) - 1;
                int ml = -1;
#pragma unroll
                for (int o = 0; o < 8; ++o) ml = (firstslot == o) ? sl[o] : ml;
                const int l = __builtin_amdgcn_readlane(ml, src);             // in [0, L): lane src has a pending slot
                float pl = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const bool h = sl[o] == l;
                    pl = h ? P[o] : pl;
                    sl[o] = h ? -1 : sl[o];
                    pend = h ? (pend & ~(1u << o)) : pend;
                }
                const float pp = nrt_dpp_wave_sum(nrt_mul(pl, pl));
                const float tp = nrt_dpp_wave_sum(fl == l ? pl : 0.0f);
                if (lane == k) { kl = l; kpp = pp; ktp = tp; }
                if (++k == NRT_WAVE) {                                        // 64 distinct ids so far: add them and start over
                    if (kl >= 0) { tab[kl] += ktp; tab[2 * L + kl] += kpp; }
                    kl = -1;
                    k = 0;
                }
                act = __ballot(pend != 0u);
            }
            if (kl >= 0) { tab[kl] += ktp; tab[2 * L + kl] += kpp; }
        }
    }
    flush();
    __syncthreads();
    float *row = part + ((long long)b * nblk + blk) * L3;
    for (int i = tid; i < L3; i += WL_BLOCK) {
        float s = wl_tab[i];
#pragma unroll
        for (int w = 1; w < WL_WAVES; ++w) s += wl_tab[w * L3 + i];
        row[i] = s;
    }
}

// grid (blocks, batch); dynamic LDS 2 L floats
template <int MODE>
__global__ __launch_bounds__(WL_BLOCK) void warp_labels_bwd(InterpArgs a, const int *__restrict__ fixed, const float *__restrict__ sums,
                                                            const float *__restrict__ gdice, float *__restrict__ gloc, float eps, int L,
                                                            unsigned per, long long vol_n) {
    extern __shared__ float wl_coef[];                          // [L][2]: d dice_l / d p_l = ca_l t_l + cb_l p_l
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    {
        const float *s = sums + (long long)b * 3 * L;
        for (int l = tid; l < L; l += WL_BLOCK) {
            const float num = 2.0f * s[l] + eps, den = s[L + l] + s[2 * L + l] + eps;
            const float gd = gdice[(long long)b * L + l];
            float ca = 0.0f, cb = 0.0f;
            if (den != 0.0f) { ca = 2.0f * gd / den; cb = -2.0f * gd * num / (den * den); }
            wl_coef[2 * l] = ca;
            wl_coef[2 * l + 1] = cb;
        }
    }
    __syncthreads();
    const int *mov = (const int *)a.vol + (long long)b * vol_n;
    const float *locb = a.loc + (long long)b * a.loc_bs;
    const int *fixb = fixed + (long long)b * a.nout;
    float *gl = gloc + (long long)b * a.nout * 3;
    const unsigned long long beg64 = (unsigned long long)blockIdx.x * per;
    const unsigned beg = beg64 < a.nout ? (unsigned)beg64 : a.nout;
    const unsigned end = (unsigned long long)beg + per < a.nout ? beg + per : a.nout;
    for (unsigned q0 = beg; q0 < end; q0 += WL_BLOCK) {
        const unsigned qq = q0 + (unsigned)tid;
        const bool live = qq < end;
        const unsigned q = live ? qq : a.nout - 1;
        int lab[8];
        float w0[3], w1[3], p[NRT_MAXD];
        bool oob;
        wl_corners<MODE>(a, locb, mov, q, lab, w0, w1, p, oob);
        const int fl = fixb[q];
        bool eq8 = true;
#pragma unroll
        for (int c = 1; c < 8; ++c) eq8 = eq8 && lab[c] == lab[0];
        float g[3] = {0.0f, 0.0f, 0.0f};
        // eight equal corners: p does not depend on the location (the weights add up to one), the gradient is 0
        if (!__all(eq8 || oob || !live)) {
            float wt[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) wt[c] = ((c & 4) ? w1[0] : w0[0]) * ((c & 2) ? w1[1] : w0[1]) * ((c & 1) ? w1[2] : w0[2]);
            float m[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) m[d] = (p[d] >= 0.0f && p[d] <= (float)(a.S[d] - 1)) ? 1.0f : 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float pc = 0.0f;                                // the warped value of corner c's id
#pragma unroll
                for (int c2 = 0; c2 < 8; ++c2) pc += (lab[c2] == lab[c]) ? wt[c2] : 0.0f;
                float gq = 0.0f;
                if ((unsigned)lab[c] < (unsigned)L) {
                    const float ca = wl_coef[2 * lab[c]], cb = wl_coef[2 * lab[c] + 1];
                    gq = (fl == lab[c] ? ca : 0.0f) + cb * pc;
                }
                const float wx = (c & 4) ? w1[0] : w0[0], wy = (c & 2) ? w1[1] : w0[1], wz = (c & 1) ? w1[2] : w0[2];
                g[0] += gq * ((c & 4) ? m[0] : -m[0]) * wy * wz;
                g[1] += gq * wx * ((c & 2) ? m[1] : -m[1]) * wz;
                g[2] += gq * wx * wy * ((c & 1) ? m[2] : -m[2]);
            }
            if (oob || eq8) { g[0] = 0.0f; g[1] = 0.0f; g[2] = 0.0f; }
        }
        if (live) {
            float *dst = gl + (long long)q * 3;
            dst[0] = g[0]; dst[1] = g[1]; dst[2] = g[2];
        }
    }
}

// argument checks shared by the entry points: NRT_OK with `a` filled, or the refusal
inline int wl_check(InterpArgs &a, long long &vol_n, const void *moving, const float *loc, const void *fixed, const int *vol_shape,
                    const int *out_shape, int nlabels, int batch, long long loc_batch_stride, int loc_mode, int has_fill) {
    if (!moving || !loc || !fixed || !vol_shape || !out_shape) return NRT_ERR_INVALID_ARG;
    if (nlabels < 1 || nlabels > WL_MAX_LABELS || batch < 1 || loc_batch_stride < 0) return NRT_ERR_INVALID_ARG;
    if (loc_mode != NRT_LOC_ABSOLUTE && loc_mode != NRT_LOC_SHIFT) return NRT_ERR_INVALID_ARG;
    unsigned long long nin = 1;
    for (int d = 0; d < 3; ++d) {
        if (vol_shape[d] < 1 || out_shape[d] < 0) return NRT_ERR_INVALID_ARG;
        nin *= (unsigned long long)vol_shape[d];
        if (nin >= (1ull << 31)) return NRT_ERR_UNSUPPORTED;
    }
    float dummy;
    const int rc = fill_args(a, moving, loc, &dummy, 3, vol_shape, out_shape, 1, batch, (long long)nin, loc_batch_stride, loc_mode, has_fill);
    if (rc != NRT_OK) return rc;
    a.out = nullptr;
    vol_n = (long long)nin;
    return NRT_OK;
}

}  // namespace

extern "C" size_t nrt_warp_dice_labels_workspace_bytes(const int *out_shape, int nlabels, int batch) {
    if (!out_shape || nlabels < 1 || nlabels > WL_MAX_LABELS || batch < 1 || batch > 65535) return 0;
    unsigned long long nout = 1;
    for (int d = 0; d < 3; ++d) {
        if (out_shape[d] < 1) return 0;
        nout *= (unsigned long long)out_shape[d];
        if (nout >= (1ull << 31)) return 0;
    }
    return wl_ws_bytes(wl_num_blocks((unsigned)nout), nlabels, batch);
}

extern "C" int nrt_warp_dice_labels_f32(const int32_t *moving, const float *loc, const int32_t *fixed, float *warped,
                                        const int *vol_shape, const int *out_shape, int nlabels, int batch,
                                        long long loc_batch_stride, int loc_mode, int has_fill, float fill_value,
                                        float laplace_smoothing, float *sums, float *dice,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    if (!sums || !dice) return NRT_ERR_INVALID_ARG;
    if (has_fill && !(fill_value == 0.0f)) return NRT_ERR_INVALID_ARG;            // (NaN included)
    InterpArgs a;
    long long vol_n = 0;
    const int rc = wl_check(a, vol_n, moving, loc, fixed, vol_shape, out_shape, nlabels, batch, loc_batch_stride, loc_mode, has_fill);
    if (rc != NRT_OK) return rc;
    if (a.nout == 0) return NRT_ERR_INVALID_ARG;
    if (warped && (unsigned long long)a.nout * nlabels * 4ull >= (1ull << 32)) return NRT_ERR_UNSUPPORTED;
    const unsigned nblk = wl_num_blocks(a.nout);
    if (!workspace || workspace_bytes < wl_ws_bytes(nblk, nlabels, batch)) return NRT_ERR_WORKSPACE;
    a.out = warped;
    float *part = (float *)workspace;
    char *p = (char *)workspace + (size_t)batch * nblk * 3 * nlabels * sizeof(float);
    p = (char *)(((uintptr_t)p + 15) & ~(uintptr_t)15);
    double *gsum = (double *)p;
    const unsigned per = (unsigned)((((unsigned long long)a.nout + (unsigned long long)nblk * WL_BLOCK - 1) /
                                     ((unsigned long long)nblk * WL_BLOCK)) * WL_BLOCK);
    hipStream_t st = nrt_stream(stream);
    const dim3 grid(nrt_xcd_grid(nblk), batch);
    const size_t lds = (size_t)WL_WAVES * 3 * nlabels * sizeof(float);
#define NRT_WL_FWD(MODE, STORE) \
    hipLaunchKernelGGL((warp_labels_fwd<MODE, STORE>), grid, dim3(WL_BLOCK), lds, st, a, (const int *)fixed, part, nlabels, nblk, per, vol_n)
    if (loc_mode == NRT_LOC_SHIFT) {
        if (warped) { NRT_WL_FWD(NRT_LOC_SHIFT, true); } else { NRT_WL_FWD(NRT_LOC_SHIFT, false); }
    } else {
        if (warped) { NRT_WL_FWD(NRT_LOC_ABSOLUTE, true); } else { NRT_WL_FWD(NRT_LOC_ABSOLUTE, false); }
    }
#undef NRT_WL_FWD
    NRT_CHECK_LAUNCH();
    const int ngrp = (int)((nblk + RED_ROWS - 1) / RED_ROWS);
    hipLaunchKernelGGL((reduce_rows<float, double>), dim3(batch, ngrp), dim3(256), 0, st, (const float *)part, (int)nblk, 3 * nlabels, gsum,
                       (const float *)nullptr, (float *)nullptr, 0);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(dice_soft_finalize, dim3(batch), dim3(256), (size_t)3 * nlabels * sizeof(float), st, (const double *)gsum,
                       (const float *)nullptr, ngrp, nlabels, laplace_smoothing, sums, dice, (float *)nullptr);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_warp_dice_labels_bwd_f32(const int32_t *moving, const float *loc, const int32_t *fixed, const float *sums,
                                            const float *grad_dice, float *grad_loc, const int *vol_shape, const int *out_shape,
                                            int nlabels, int batch, long long loc_batch_stride, int loc_mode, int has_fill,
                                            float laplace_smoothing, void *stream) {
    if (!sums || !grad_dice || !grad_loc) return NRT_ERR_INVALID_ARG;
    InterpArgs a;
    long long vol_n = 0;
    const int rc = wl_check(a, vol_n, moving, loc, fixed, vol_shape, out_shape, nlabels, batch, loc_batch_stride, loc_mode, has_fill);
    if (rc != NRT_OK) return rc;
    if (a.nout == 0) return NRT_OK;
    unsigned blocks = (a.nout + WL_BLOCK - 1) / WL_BLOCK;
    if (blocks > 256u * 16u) blocks = 256u * 16u;
    const unsigned per = (unsigned)((((unsigned long long)a.nout + (unsigned long long)blocks * WL_BLOCK - 1) /
                                     ((unsigned long long)blocks * WL_BLOCK)) * WL_BLOCK);
    hipStream_t st = nrt_stream(stream);
    const dim3 grid(blocks, batch);
    const size_t lds = (size_t)2 * nlabels * sizeof(float);
    if (loc_mode == NRT_LOC_SHIFT)
        hipLaunchKernelGGL((warp_labels_bwd<NRT_LOC_SHIFT>), grid, dim3(WL_BLOCK), lds, st, a, (const int *)fixed, sums, grad_dice, grad_loc,
                           laplace_smoothing, nlabels, per, vol_n);
    else
        hipLaunchKernelGGL((warp_labels_bwd<NRT_LOC_ABSOLUTE>), grid, dim3(WL_BLOCK), lds, st, a, (const int *)fixed, sums, grad_dice, grad_loc,
                           laplace_smoothing, nlabels, per, vol_n);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
