// Warp integer LABEL MAPS by linear interpolation + arg-max, and fuse several warped label maps by a weighted vote, gfx950.
//
// With M = one_hot(moving, L) in float32 the result of warp_labels_argmax is argmax_l / max_l of the tri-linear warp of M (utils.py:159-191
// on 0/1 data), but M never exists: per label the blend is the sum of the weights fl(fl(wx wy) wz) of the corners that carry the label,
// added in corner order 000 ... 111 starting from 0, so a voxel has at most 8 non-zero values; they follow from 8 gathered int32 ids and
// 8 weights (wl_core.h, shared with warp_labels.hip).  Per output voxel that is 12 B of field, 4 B of id stored (8 with `prob`) and 8 id
// reads from a volume that fits the Infinity Cache, against 3 passes over L floats for one-hot -> warp -> arg-max.
//
// warp_labels_argmax  one lane per output voxel, a block walks a contiguous range of voxels in steps of 256 on one XCD.  A lane merges
//   equal ids in corner order into at most 8 (id, p) slots (slot o belongs to the first corner with its id); the winner is the slot with
//   the largest p > 0, an exact tie going to the smaller id; no slot with p > 0: id 0, p 0 (np.argmax of an all-zero row).  Restricted
//   mode (L >= 1): an id outside [0, L) owns no slot that can win and is never used as an index.  L = 0: every int32 value is a label.
//   has_fill: a voxel whose unclipped location lies outside the volume gets fill_label and p 0; else the edge is clamped.
//   Fast path: while all 8 corners of all 64 lanes of a wave carry ONE id (the interior of every structure) the merge is skipped, and
//   so are the 8 weights unless `prob` is wanted: some corner weight is >= 1/8 whatever the location holds, so the id wins either way.
//   Location front ends (template argument): a dense field (NRT_LOC_SHIFT / NRT_LOC_ABSOLUTE), resize's align-corners grid
//   (NRT_LOC_LINSPACE, no loc tensor), or an affine matrix with exactly nrt_affine_warp_f32's roundings (affine_core.h).
// fuse_labels  N atlases, each under its own field (or one shared field).  One wave per block, one lane per output voxel; the lane keeps
//   the candidate list of the voxel, (id, vote) entries in LDS laid out [entry][lane] (a lane only ever touches its own column: no two
//   lanes of a half-wave meet in a bank, and nothing is shared, so no barrier).  Atlas n adds fl(w_n p_{n,l}) to the entry of l --
//   appended as 0 + fl(w_n p) where l is new: the atlases before n added +0 -- so V_l is the float32 sum in atlas order.  The list
//   holds min(8 N, 32) entries: with all 8 N of them (64 KiB at 16 atlases) two waves fit a CU and the gathers' latency is exposed
//   (15.7 ms for 16 atlases at 160^3 against 8.3 ms for 16 one-hot warps added by torch).  A voxel with more candidates than that --
//   more than 32 distinct ids among its 8 N corners -- is done again without a list, from a second look at the other atlases per
//   candidate: slow, exact, and not met on anatomical maps.
//   The winner follows the rule above.  With a fill label an atlas whose location is out of bounds adds nothing; all of them: fill_label.
// No atomics, no host synchronisation; paths depend on the data and the shapes only: run-to-run bit-identical.  Gather indices come
// from corner_1d and stay inside the volume for any location, NaN and Inf included.
#include "affine_core.h"
#include "wl_core.h"

namespace {

constexpr int WA_AFFINE = 3;                 // location front end next to the three NRT_LOC_* modes: an affine matrix in registers
constexpr int WA_MAX_BLOCKS = 2048;          // per batch entry: 8 blocks per CU
constexpr int WA_MIN_STEPS = 4;              // a block walks at least this many steps (where the volume has them)
constexpr int FL_MAX_ATLASES = 16;
constexpr int FL_CAP = 32;                   // entries of a lane's candidate list in LDS: 16 KiB per wave
constexpr int FL_MAX_BLOCKS = 16384;         // blocks of ONE wave

// blocks of `block` lanes for nout voxels, and the voxels per block (a multiple of `block`)
inline unsigned wa_num_blocks(unsigned nout, unsigned block, unsigned max_blocks, unsigned &per) {
    unsigned long long nb = ((unsigned long long)nout + block * WA_MIN_STEPS - 1) / (block * WA_MIN_STEPS);
    if (nb > max_blocks) nb = max_blocks;
    if (nb < 1) nb = 1;
    per = (unsigned)((((unsigned long long)nout + nb * block - 1) / (nb * block)) * block);
    return (unsigned)nb;
}

// merge equal ids in corner order: P[o] = the warped value of id lab[o]; bit o of the result: corner o is the first with its id
__device__ __forceinline__ unsigned wa_merge(const int (&lab)[8], const float (&wt)[8], float (&P)[8]) {
    unsigned own = 0u;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float s = wt[o];
        bool first = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c < o) first = first && lab[c] != lab[o];
            if (c > o) s = (lab[c] == lab[o]) ? nrt_add(s, wt[c]) : s;
        }
        P[o] = s;
        own |= first ? (1u << o) : 0u;
    }
    return own;
}

// the winner so far is (bid, bp), (0, 0) before the first candidate: the largest p > 0, an exact tie to the smaller id
__device__ __forceinline__ void wa_better(int id, float p, int &bid, float &bp) {
    const bool better = p > bp || (p == bp && bp > 0.0f && id < bid);
    bid = better ? id : bid;
    bp = better ? p : bp;
}

// grid (nrt_xcd_grid(nblk), batch); a.out: ids [batch][nout] int32; prob [batch][nout] (PROB)
template <int FRONT, bool PROB>
__global__ __launch_bounds__(WL_BLOCK) void warp_labels_argmax(InterpArgs a, AffWarpArgs af, float *__restrict__ prob, int L, int fill_label,
                                                               unsigned nblk, unsigned per, long long vol_n) {
    const unsigned blk = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (blk >= nblk) return;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int *mov = (const int *)a.vol + (long long)b * vol_n;
    const float *locb = (FRONT == NRT_LOC_SHIFT || FRONT == NRT_LOC_ABSOLUTE) ? a.loc + (long long)b * a.loc_bs : nullptr;
    int *ids = (int *)a.out + (long long)b * a.nout;
    float *pr = PROB ? prob + (long long)b * a.nout : nullptr;
    float M[3][4];
    if constexpr (FRONT == WA_AFFINE) load_matrix<3>(af, b, M);
    const bool any_id = L == 0;

    const unsigned long long beg64 = (unsigned long long)blk * per;
    const unsigned beg = beg64 < a.nout ? (unsigned)beg64 : a.nout;
    const unsigned end = (unsigned long long)beg + per < a.nout ? beg + per : a.nout;
    for (unsigned q0 = beg; q0 < end; q0 += WL_BLOCK) {
        const unsigned qq = q0 + (unsigned)tid;
        const bool live = qq < end;
        const unsigned q = live ? qq : a.nout - 1;
        float p[NRT_MAXD];
        if constexpr (FRONT == WA_AFFINE) {
            float pc[3], loc[3];
            affine_loc<3>(af, M, q, pc, loc);
            p[0] = loc[0]; p[1] = loc[1]; p[2] = loc[2];
        } else {
            int qd[NRT_MAXD];
            decode<3>(a, q, qd);
            load_loc<3, FRONT>(a, locb, q, qd, p);
        }
        const bool oob = a.has_fill ? out_of_bounds<3>(a, p) : false;
        int lab[8];
        float w0[3], w1[3];
        wl_gather(a, mov, p, lab, w0, w1);

        bool eq8 = true;
#pragma unroll
        for (int c = 1; c < 8; ++c) eq8 = eq8 && lab[c] == lab[0];
        const int l0u = __builtin_amdgcn_readfirstlane(lab[0]);
        const bool fast = __all(eq8 && lab[0] == l0u);

        int bid = 0;
        float bp = 0.0f;
        if (fast) {
            const bool valid = any_id || (unsigned)l0u < (unsigned)L;
            bid = valid ? l0u : 0;
            if (PROB) {
                float wt[8];
                wl_weights(w0, w1, wt);
                float s = wt[0];
#pragma unroll
                for (int c = 1; c < 8; ++c) s = nrt_add(s, wt[c]);
                bp = valid ? s : 0.0f;
            }
        } else {
            float wt[8], P[8];
            wl_weights(w0, w1, wt);
            const unsigned own = wa_merge(lab, wt, P);
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const bool cand = ((own >> o) & 1u) && (any_id || (unsigned)lab[o] < (unsigned)L);
                wa_better(lab[o], cand ? P[o] : 0.0f, bid, bp);                  // (p = 0 never wins)
            }
        }
        if (oob) {
            bid = fill_label;
            bp = 0.0f;
        }
        if (live) {
            ids[q] = bid;
            if (PROB) pr[q] = bp;
        }
    }
}

// what atlas n contributes at output voxel q: the 8 corner ids, the 8 corner weights, its vote weight and whether it is out of bounds
__device__ __forceinline__ void fl_sample(const InterpArgs &a, const float *__restrict__ weights, long long loc_as, long long vol_n, int n,
                                          unsigned q, const int (&qd)[NRT_MAXD], int (&lab)[8], float (&wt)[8], float &wn, bool &oob) {
    float p[NRT_MAXD], w0[3], w1[3];
    load_loc<3, NRT_LOC_SHIFT>(a, a.loc + (long long)n * loc_as, q, qd, p);
    oob = a.has_fill ? out_of_bounds<3>(a, p) : false;
    wl_gather(a, (const int *)a.vol + (long long)n * vol_n, p, lab, w0, w1);
    wl_weights(w0, w1, wt);
    wn = weights ? weights[n] : 1.0f;
}

// grid nrt_xcd_grid(nblk), one wave per block; dynamic LDS cap entries x 64 lanes x (int + float), cap = min(8 N, FL_CAP)
// a.vol: atlases [N][vol_n] int32, a.loc: fields [N][nout][3] (loc_as = 0: one field), a.out: ids [nout] int32
__global__ __launch_bounds__(NRT_WAVE) void fuse_labels(InterpArgs a, const float *__restrict__ weights, float *__restrict__ votes, int L,
                                                        int N, int cap, long long loc_as, int fill_label, unsigned nblk, unsigned per,
                                                        long long vol_n) {
    extern __shared__ int fl_lds[];                              // ids [cap][64], then votes [cap][64]
    const unsigned blk = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (blk >= nblk) return;
    const int lane = threadIdx.x;
    int *cid = fl_lds + lane;                                    // entry j of this lane: cid[j * 64], cv[j * 64]
    float *cv = (float *)(fl_lds + cap * NRT_WAVE) + lane;
    int *ids = (int *)a.out;
    const bool any_id = L == 0;

    const unsigned long long beg64 = (unsigned long long)blk * per;
    const unsigned beg = beg64 < a.nout ? (unsigned)beg64 : a.nout;
    const unsigned end = (unsigned long long)beg + per < a.nout ? beg + per : a.nout;
    for (unsigned q0 = beg; q0 < end; q0 += NRT_WAVE) {
        const unsigned qq = q0 + (unsigned)lane;
        const bool live = qq < end;
        const unsigned q = live ? qq : a.nout - 1;
        int qd[NRT_MAXD];
        decode<3>(a, q, qd);
        int cnt = 0;                                             // entries of this lane's list
        bool over = false;                                       // the voxel has more than `cap` candidates: see below
        bool inside = false;                                     // some atlas is sampled inside its volume (or there is no fill)
        for (int n = 0; n < N; ++n) {
            int lab[8];
            float wt[8], P[8], wn;
            bool oob;
            fl_sample(a, weights, loc_as, vol_n, n, q, qd, lab, wt, wn, oob);
            const unsigned own = wa_merge(lab, wt, P);
            inside = inside || !oob;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                if (!over && !oob && ((own >> o) & 1u) && (any_id || (unsigned)lab[o] < (unsigned)L)) {
                    const float v = nrt_mul(wn, P[o]);
                    int j = 0;
                    while (j < cnt && cid[j * NRT_WAVE] != lab[o]) ++j;
                    if (j < cnt) {
                        cv[j * NRT_WAVE] = nrt_add(cv[j * NRT_WAVE], v);
                    } else if (cnt < cap) {
                        cid[cnt * NRT_WAVE] = lab[o];
                        cv[cnt * NRT_WAVE] = nrt_add(0.0f, v);
                        ++cnt;
                    } else {
                        over = true;
                    }
                }
            }
        }
        int bid = 0;
        float bp = 0.0f;
        if (!over)
            for (int j = 0; j < cnt; ++j) wa_better(cid[j * NRT_WAVE], cv[j * NRT_WAVE], bid, bp);
        // More candidates than the list holds (only possible where 8 N > cap): the voxel is done again without a list, exactly.  Every
        // candidate (atlas n, slot o) whose id l is not carried by an atlas before n gets V_l = 0 + fl(w_n p_{n,l}) + the terms of
        // the atlases after n that carry l, in order -- the sum the list would hold -- from a second look at every other atlas.
        if (__any(over)) {
            for (int n = 0; n < N; ++n) {
                int lab[8];
                float wt[8], P[8], wn;
                bool oob;
                fl_sample(a, weights, loc_as, vol_n, n, q, qd, lab, wt, wn, oob);
                const unsigned own = wa_merge(lab, wt, P);
#pragma unroll 1
                for (int o = 0; o < 8; ++o) {
                    int l = lab[0];
                    float pl = P[0];
#pragma unroll
                    for (int k = 1; k < 8; ++k) {
                        l = o == k ? lab[k] : l;
                        pl = o == k ? P[k] : pl;
                    }
                    const bool cand = over && !oob && ((own >> o) & 1u) && (any_id || (unsigned)l < (unsigned)L);
                    if (!__any(cand)) continue;
                    float V = nrt_add(0.0f, nrt_mul(wn, pl));
                    bool seen = false;
                    for (int n2 = 0; n2 < N; ++n2) {
                        if (n2 == n) continue;
                        int lab2[8];
                        float wt2[8], w2;
                        bool oob2;
                        fl_sample(a, weights, loc_as, vol_n, n2, q, qd, lab2, wt2, w2, oob2);
                        float s = 0.0f;
                        bool has = false;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const bool m = lab2[c] == l;
                            s = m ? nrt_add(s, wt2[c]) : s;
                            has = has || m;
                        }
                        has = has && !oob2;
                        if (n2 < n) seen = seen || has;
                        else V = has ? nrt_add(V, nrt_mul(w2, s)) : V;
                    }
                    if (cand && !seen) wa_better(l, V, bid, bp);
                }
            }
        }
        if (!inside) bid = fill_label;                           // (no candidate: bp = 0)
        if (live) {
            ids[q] = bid;
            if (votes) votes[q] = bp;
        }
    }
}

// the checks the three entry points share; NRT_OK with `a` and vol_n filled, or the refusal.  `loc` may be NULL for NRT_LOC_LINSPACE.
inline int wa_check(InterpArgs &a, long long &vol_n, const void *moving, const float *loc, void *out_ids, const int *vol_shape,
                    const int *out_shape, int nlabels, int batch, long long loc_stride, int loc_mode, int has_fill) {
    if (!moving || !out_ids || !vol_shape || !out_shape) return NRT_ERR_INVALID_ARG;
    if (nlabels < 0 || batch < 1 || loc_stride < 0) return NRT_ERR_INVALID_ARG;
    if (loc_mode != NRT_LOC_ABSOLUTE && loc_mode != NRT_LOC_SHIFT && loc_mode != NRT_LOC_LINSPACE) return NRT_ERR_INVALID_ARG;
    if ((loc_mode == NRT_LOC_LINSPACE) != (loc == nullptr)) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < 3; ++d)
        if (vol_shape[d] < 1 || out_shape[d] < 1) return NRT_ERR_INVALID_ARG;
    unsigned long long nin = 1, nout = 1;
    for (int d = 0; d < 3; ++d) {
        nin *= (unsigned long long)vol_shape[d];
        nout *= (unsigned long long)out_shape[d];
        if (nin >= (1ull << 31) || nout >= (1ull << 31)) return NRT_ERR_UNSUPPORTED;    // (each factor < 2^31: no overflow before the test)
    }
    const int rc = fill_args(a, moving, loc, out_ids, 3, vol_shape, out_shape, 1, batch, (long long)nin, loc_stride, loc_mode, has_fill);
    if (rc != NRT_OK) return rc;
    vol_n = (long long)nin;
    return NRT_OK;
}

template <int FRONT>
void wa_launch(const InterpArgs &a, const AffWarpArgs &af, float *prob, int nlabels, int fill_label, long long vol_n, int batch,
               hipStream_t st) {
    unsigned per = 0;
    const unsigned nblk = wa_num_blocks(a.nout, WL_BLOCK, WA_MAX_BLOCKS, per);
    const dim3 grid(nrt_xcd_grid(nblk), (unsigned)batch);
    if (prob)
        hipLaunchKernelGGL((warp_labels_argmax<FRONT, true>), grid, dim3(WL_BLOCK), 0, st, a, af, prob, nlabels, fill_label, nblk, per, vol_n);
    else
        hipLaunchKernelGGL((warp_labels_argmax<FRONT, false>), grid, dim3(WL_BLOCK), 0, st, a, af, prob, nlabels, fill_label, nblk, per, vol_n);
}

}  // namespace

extern "C" int nrt_warp_labels_argmax_i32(const int32_t *moving, const float *loc, int32_t *out_ids, float *out_prob, const int *vol_shape,
                                          const int *out_shape, int nlabels, int batch, long long loc_batch_stride, int loc_mode,
                                          int has_fill, int fill_label, void *stream) {
    InterpArgs a;
    long long vol_n = 0;
    const int rc = wa_check(a, vol_n, moving, loc, out_ids, vol_shape, out_shape, nlabels, batch, loc_batch_stride, loc_mode, has_fill);
    if (rc != NRT_OK) return rc;
    AffWarpArgs af = {};
    hipStream_t st = nrt_stream(stream);
    if (loc_mode == NRT_LOC_SHIFT) wa_launch<NRT_LOC_SHIFT>(a, af, out_prob, nlabels, fill_label, vol_n, batch, st);
    else if (loc_mode == NRT_LOC_ABSOLUTE) wa_launch<NRT_LOC_ABSOLUTE>(a, af, out_prob, nlabels, fill_label, vol_n, batch, st);
    else wa_launch<NRT_LOC_LINSPACE>(a, af, out_prob, nlabels, fill_label, vol_n, batch, st);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_affine_warp_labels_argmax_i32(const int32_t *moving, const float *matrix, int32_t *out_ids, float *out_prob,
                                                 const int *vol_shape, const int *out_shape, int nlabels, int batch, int matrix_batch,
                                                 int shift_center, int has_fill, int fill_label, void *stream) {
    if (!matrix || batch < 1 || (matrix_batch != 1 && matrix_batch != batch)) return NRT_ERR_INVALID_ARG;
    InterpArgs a;
    long long vol_n = 0;
    const int rc = wa_check(a, vol_n, moving, nullptr, out_ids, vol_shape, out_shape, nlabels, batch, 0, NRT_LOC_LINSPACE, has_fill);
    if (rc != NRT_OK) return rc;
    AffWarpArgs af = {};
    af.matrix = matrix;
    af.m_bs = matrix_batch == 1 ? 0 : 12;
    for (int d = 0; d < 3; ++d) {
        af.S[d] = a.S[d];
        af.O[d] = a.O[d];
        af.c[d] = shift_center ? (float)(a.O[d] - 1) / 2.0f : 0.0f;          // as nrt_affine_warp_f32
    }
    wa_launch<WA_AFFINE>(a, af, out_prob, nlabels, fill_label, vol_n, batch, nrt_stream(stream));
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_fuse_labels_i32(const int32_t *atlases, const float *loc, const float *weights, int32_t *out_ids, float *out_votes,
                                   const int *vol_shape, const int *out_shape, int nlabels, int n_atlases, long long loc_atlas_stride,
                                   int has_fill, int fill_label, void *stream) {
    if (!loc || n_atlases < 1) return NRT_ERR_INVALID_ARG;
    InterpArgs a;
    long long vol_n = 0;
    // (the atlases take the place of the batch in the shared checks; their limit is below)
    const int rc = wa_check(a, vol_n, atlases, loc, out_ids, vol_shape, out_shape, nlabels, 1, loc_atlas_stride, NRT_LOC_SHIFT, has_fill);
    if (rc != NRT_OK) return rc;
    if (n_atlases > FL_MAX_ATLASES) return NRT_ERR_UNSUPPORTED;
    unsigned per = 0;
    const unsigned nblk = wa_num_blocks(a.nout, NRT_WAVE, FL_MAX_BLOCKS, per);
    const int cap = 8 * n_atlases < FL_CAP ? 8 * n_atlases : FL_CAP;
    const size_t lds = (size_t)cap * NRT_WAVE * (sizeof(int) + sizeof(float));                        // at most 16 KiB
    hipLaunchKernelGGL(fuse_labels, dim3(nrt_xcd_grid(nblk)), dim3(NRT_WAVE), lds, nrt_stream(stream), a, weights, out_votes, nlabels,
                       n_atlases, cap, loc_atlas_stride, fill_label, nblk, per, vol_n);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
