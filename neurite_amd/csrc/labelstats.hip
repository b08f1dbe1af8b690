// Per-label region statistics of an integer id map and the confusion matrix of two id maps.  What they replace: a one-hot
// tensor [B, *S, L] and its reductions, torch.bincount / scatter_add (float atomics), or a round trip through the host and scipy.ndimage.
//
// nrt_label_stats, three launches:
//   init      zeroes counts and coord_sums, sets the boxes to (shape[a], -1) and the min / max keys to (+inf, -inf), and one block sorts
//             the label list into the workspace (keys ascending, the slot of each key)
//   main      grid (blocks of an entry, B), 4 waves; a block owns one contiguous share of an entry, a wave every fourth 64-voxel step of
//             it, one lane per voxel.  Per step the wave peels off its distinct slots (the slot of the lowest pending lane, a ballot of
//             the lanes that hold it).  The count, the coordinate sums and the box of a segment follow from the ballot mask and the
//             step's first voxel alone (ls_seg_of_lanes: no lane exchanges anything); x, x * x, min and max per channel are reduced
//             over the mask in float32 by a fixed tree of DPP steps.  Lane 0 adds the float sums to the wave's PRIVATE LDS row (one
//             writer: a fixed order) and the integers, with the min / max as ordered keys, to the block's LDS tables by integer
//             atomics.  A wave whose 64 voxels carry one id runs the loop once.  At the end the block writes the float64 sum of its
//             four wave rows, in wave order, to its workspace row (every element: the rows need no zeroing) and adds its integers to
//             the outputs by integer atomics.
//   finish    per (entry, slot, channel, which) the float64 sum of the block rows: 32 runs of consecutive blocks, each in block order,
//             then the runs in order; the keys become floats.
// nrt_label_confusion_i32, two launches: init (zero, sort) and one pass over both maps.  Up to kConfLdsLabels labels a block counts in
// a private LDS table of (L + 1)^2 words and adds its non-zero counters to the global table; above that every wave adds once per distinct
// (i, j) pair it holds straight to the global table.  Integers only: exact and order-free.
// No float atomics, no workgroup waits for another, nothing goes to the host, nothing is allocated: the calls capture into a graph.
#include "nrt_common.h"

#include "labelstats_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kMaxBatch = 65535;                     // gridDim.y
constexpr int kBlockVoxels = 4096;                   // the least share of a block
constexpr int kTargetBlocks = 2048;                  // about that many blocks in a launch
constexpr int kTableWords = 2 * kLsMaxLabels;        // the sorted label list in the workspace: keys, then slots
constexpr int kConfLdsLabels = 111;                  // (111 + 1)^2 counters = 49 KB: three blocks on a CU's 160 KB of LDS
constexpr unsigned kNoCode = 0xFFFFFFFFu;

static_assert(kLsWave == NRT_WAVE, "labelstats_core.h is written for wave64");

struct LsOut {
    unsigned long long *counts, *coord_sums;         // int64 outputs, added to as unsigned words
    int *bbox;
    double *sums;
    unsigned *minmax;                                // the float output, holding ordered keys until the finish
};

struct LsGeom {
    LsShape g;
    unsigned V, per, blocks;
    int nd, nl;
};

// ---- init ----------------------------------------------------------------------------------------------------------------------------
// every output to its empty value; block 0 sorts the label list.  n_* are element counts (0 for an output that is not wanted).
__global__ void __launch_bounds__(kThreads)
ls_init(const int *__restrict__ labels, int nl, int *__restrict__ table, LsOut o, size_t n_counts, size_t n_cs, size_t n_bbox, size_t n_mm,
        LsShape g, int nd) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    for (size_t i = first; i < n_counts; i += stride) o.counts[i] = 0ull;
    for (size_t i = first; i < n_cs; i += stride) o.coord_sums[i] = 0ull;
    for (size_t i = first; i < n_bbox; i += stride) {
        const int a = (int)(i % (size_t)nd), which = (int)((i / (size_t)nd) & 1);
        o.bbox[i] = which == 0 ? (int)g.s[a + 3 - nd] : -1;
    }
    for (size_t i = first; i < n_mm; i += stride) o.minmax[i] = (i & 1) ? kLsKeyNegInf : kLsKeyPosInf;
    if (blockIdx.x == 0 && labels && (int)threadIdx.x < nl) {
        const int r = ls_rank(labels, nl, (int)threadIdx.x);
        table[r] = labels[threadIdx.x];
        table[kLsMaxLabels + r] = (int)threadIdx.x;
    }
}

// ---- loads and wave reductions -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ls_load(const void *image, int dt, size_t at) {
    if (dt == NRT_DT_F32) return ((const float *)image)[at];
    const unsigned short h = ((const unsigned short *)image)[at];
    if (dt == NRT_DT_BF16) return __uint_as_float((unsigned)h << 16);
    return (float)__builtin_bit_cast(_Float16, h);
}

// A wave reduction on the DPP path (no LDS crossbar): pairs and quads by quad_perm, the four quads of a row of 16 by row_ror 4 and 8,
// rows 0 + 1 and 2 + 3 by row_bcast15, the halves by row_bcast31; lane 63 holds the result, which comes back uniform.  The tree is the
// same whatever the lanes hold: a fixed order.  Lanes that a step's row mask leaves out combine with the identity.  Every lane of the
// wave calls it (EXEC all ones).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float ls_dpp(float v, float identity) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}

template <typename OP>
__device__ __forceinline__ float ls_wave_reduce(float v, float identity, OP op) {
    v = op(v, ls_dpp<0xB1, 0xF>(v, identity));                                       // quad_perm [1, 0, 3, 2]
    v = op(v, ls_dpp<0x4E, 0xF>(v, identity));                                       // quad_perm [2, 3, 0, 1]
    v = op(v, ls_dpp<0x124, 0xF>(v, identity));                                      // row_ror 4
    v = op(v, ls_dpp<0x128, 0xF>(v, identity));                                      // row_ror 8
    v = op(v, ls_dpp<0x142, 0xA>(v, identity));                                      // row_bcast15 into rows 1 and 3
    v = op(v, ls_dpp<0x143, 0xC>(v, identity));                                      // row_bcast31 into rows 2 and 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), NRT_WAVE - 1));
}

__device__ __forceinline__ float ls_wave_sum(float v) {
    return ls_wave_reduce(v, 0.0f, [](float a, float b) { return nrt_add(a, b); });
}
__device__ __forceinline__ float ls_wave_min(float v) {                              // (fminf / fmaxf skip a NaN)
    return ls_wave_reduce(v, __uint_as_float(0x7F800000u), [](float a, float b) { return fminf(a, b); });
}
__device__ __forceinline__ float ls_wave_max(float v) {
    return ls_wave_reduce(v, __uint_as_float(0xFF800000u), [](float a, float b) { return fmaxf(a, b); });
}

__device__ __forceinline__ int ls_slot(const int *keys, const int *slots, bool listed, int nl, int id) {
    return listed ? ls_find(keys, slots, nl, id) : ls_direct(id, nl);
}

// the label list of a call from the workspace into LDS
__device__ __forceinline__ void ls_stage_table(const int *table, int nl, int *keys, int *slots) {
    if (table)
        for (int i = threadIdx.x; i < nl; i += kThreads) {
            keys[i] = table[i];
            slots[i] = table[kLsMaxLabels + i];
        }
}

// ---- main ----------------------------------------------------------------------------------------------------------------------------
// dynamic LDS, nl * (60 + 40 C) bytes: cs [nl, 3] u64 | lo, hi [nl, 3] | cnt [nl] | keys, slots [nl] | mm [nl, C, 2] | wrow [4][nl, C, 2]
template <int C>
__global__ void __launch_bounds__(kThreads)
ls_main(const int *__restrict__ ids, const void *__restrict__ image, int dt, const int *__restrict__ table, LsGeom p, LsOut o,
        double *__restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ls_lds[];
    const int nl = p.nl, ax0 = 3 - p.nd;
    const int rowlen = nl * C * 2;
    unsigned long long *cs = ls_lds;
    int *lo = (int *)(cs + nl * 3), *hi = lo + nl * 3;
    unsigned *cnt = (unsigned *)(hi + nl * 3);
    int *keys = (int *)(cnt + nl), *slots = keys + nl;
    unsigned *mm = (unsigned *)(slots + nl);
    float *wrow = (float *)(mm + rowlen);
    const bool listed = table != nullptr;

    for (int i = threadIdx.x; i < nl * 3; i += kThreads) cs[i] = 0ull, lo[i] = 0x7FFFFFFF, hi[i] = -1;
    for (int i = threadIdx.x; i < nl; i += kThreads) cnt[i] = 0u;
    for (int i = threadIdx.x; i < rowlen; i += kThreads) mm[i] = (i & 1) ? kLsKeyNegInf : kLsKeyPosInf;
    for (int i = threadIdx.x; i < kWaves * rowlen; i += kThreads) wrow[i] = 0.0f;
    ls_stage_table(table, nl, keys, slots);
    __syncthreads();

    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    float *mine = wrow + wave * rowlen;
    const unsigned beg = min(blockIdx.x * p.per, p.V), end = min(beg + p.per, p.V);              // (blockIdx.x * per < V + per < 2^32)
    const size_t base = (size_t)blockIdx.y * p.V;

    // (the loops are uniform per wave: every lane takes part in the ballots and the butterflies)
    unsigned v = beg + (unsigned)(wave * NRT_WAVE + lane);
    int id = 0;
    float x[C > 0 ? C : 1] = {};
    if (v < end) {
        id = ids[base + v];
        for (int c = 0; c < C; ++c) x[c] = ls_load(image, dt, (base + v) * C + c);
    }
    for (unsigned step = beg + (unsigned)(wave * NRT_WAVE); step < end; step += kThreads) {
        const unsigned cur = v;
        const int slot = cur < end ? ls_slot(keys, slots, listed, nl, id) : kLsNone;
        float xc[C > 0 ? C : 1];
        for (int c = 0; c < C; ++c) xc[c] = x[c];
        // the next step's loads are in flight while this one is reduced
        v += kThreads;
        if (v < end) {
            id = ids[base + v];
            for (int c = 0; c < C; ++c) x[c] = ls_load(image, dt, (base + v) * C + c);
        }
        const unsigned v0 = (unsigned)__builtin_amdgcn_readfirstlane((int)step);     // (the wave's first voxel, as a scalar)
        unsigned long long pending = __ballot(slot != kLsNone);
        while (pending != 0ull) {                                                    // (uniform)
            const int s = __builtin_amdgcn_readlane(slot, ls_lowest(pending));
            const bool in = slot == s;
            const unsigned long long lanes = __ballot(in);
            const LsSeg seg = ls_seg_of_lanes(lanes, v0, p.g);
            if (lane == 0) {
                atomicAdd(cnt + s, (unsigned)__popcll(lanes));
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (a < ax0) continue;
                    atomicAdd(cs + s * 3 + a, seg.cs[a]);
                    atomicMin(lo + s * 3 + a, seg.lo[a]);
                    atomicMax(hi + s * 3 + a, seg.hi[a]);
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float inf = __uint_as_float(0x7F800000u);
                const float sum = ls_wave_sum(in ? xc[c] : 0.0f);
                const float sq = ls_wave_sum(in ? nrt_mul(xc[c], xc[c]) : 0.0f);
                const float mn = ls_wave_min(in ? xc[c] : inf);                      // (fminf / fmaxf skip a NaN: never a NaN)
                const float mx = ls_wave_max(in ? xc[c] : -inf);
                if (lane == 0) {
                    const int at = (s * C + c) * 2;
                    mine[at] = nrt_add(mine[at], sum);
                    mine[at + 1] = nrt_add(mine[at + 1], sq);
                    atomicMin(mm + at, ls_fkey(__float_as_uint(mn)));
                    atomicMax(mm + at + 1, ls_fkey(__float_as_uint(mx)));
                }
            }
            pending &= ~lanes;
        }
    }
    __syncthreads();

    const size_t entry = (size_t)blockIdx.y * nl;
    for (int s = threadIdx.x; s < nl; s += kThreads) {
        if (cnt[s] == 0u) continue;
        atomicAdd(o.counts + entry + s, (unsigned long long)cnt[s]);
        for (int a = ax0; a < 3; ++a) {
            if (o.coord_sums) atomicAdd(o.coord_sums + (entry + s) * p.nd + (a - ax0), cs[s * 3 + a]);
            if (o.bbox) {
                atomicMin(o.bbox + ((entry + s) * 2 + 0) * p.nd + (a - ax0), lo[s * 3 + a]);
                atomicMax(o.bbox + ((entry + s) * 2 + 1) * p.nd + (a - ax0), hi[s * 3 + a]);
            }
        }
    }
    if (C > 0) {
        double *row = rows + ((size_t)blockIdx.y * p.blocks + blockIdx.x) * rowlen;
        for (int i = threadIdx.x; i < rowlen; i += kThreads) {
            if (o.sums) {
                double d = (double)wrow[i];
                for (int w = 1; w < kWaves; ++w) d += (double)wrow[w * rowlen + i];
                row[i] = d;
            }
            if (o.minmax) {
                const unsigned key = mm[i];
                if ((i & 1) == 0 && key != kLsKeyPosInf) atomicMin(o.minmax + (size_t)blockIdx.y * rowlen + i, key);
                if ((i & 1) == 1 && key != kLsKeyNegInf) atomicMax(o.minmax + (size_t)blockIdx.y * rowlen + i, key);
            }
        }
    }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------------
// 8 outputs per block, 32 threads each: thread `part` adds the rows of the part-th run of consecutive blocks in block order, thread 0 of
// an output the 32 runs in run order, all in float64: a fixed order, and no thread walks more than blocks / 32 rows.
constexpr int kFinishCols = 8, kFinishParts = kThreads / kFinishCols;

__global__ void __launch_bounds__(kThreads)
ls_finish(const double *__restrict__ rows, unsigned blocks, size_t rowlen, size_t total, LsOut o) {
    __shared__ double run_sum[kFinishParts][kFinishCols];
    const unsigned col = threadIdx.x % kFinishCols, part = threadIdx.x / kFinishCols;
    const size_t i = (size_t)blockIdx.x * kFinishCols + col;
    if (o.sums) {                                                                    // (uniform)
        double d = 0.0;
        if (i < total) {
            const size_t e = i / rowlen, r = i - e * rowlen;
            const double *column = rows + e * blocks * rowlen + r;
            const unsigned run = (blocks + kFinishParts - 1) / kFinishParts;
            const unsigned b0 = min(part * run, blocks), b1 = min(b0 + run, blocks);
#pragma unroll 4
            for (unsigned b = b0; b < b1; ++b) d += column[(size_t)b * rowlen];
        }
        run_sum[part][col] = d;
        __syncthreads();
        if (part == 0 && i < total) {
            double t = run_sum[0][col];
            for (int k = 1; k < kFinishParts; ++k) t += run_sum[k][col];
            o.sums[i] = t;
        }
    }
    if (o.minmax && part == 0 && i < total) o.minmax[i] = ls_funkey(o.minmax[i]);
}

// ---- confusion -----------------------------------------------------------------------------------------------------------------------
// counter[code] += 1 for every lane with a code, added per wave: the lanes that hold the code of the lowest pending lane are counted by a
// ballot and added once; after `rounds` such rounds what is left goes lane by lane (rounds < 0: until nothing is left)
template <typename T>
__device__ __forceinline__ void ls_conf_add(T *counter, unsigned code, int lane, int rounds) {
    unsigned long long pending = __ballot(code != kNoCode);
    for (int r = 0; pending != 0ull && (rounds < 0 || r < rounds); ++r) {              // (uniform)
        const int leader = __ffsll(pending) - 1;
        const unsigned lead = (unsigned)__shfl((int)code, leader, NRT_WAVE);
        const unsigned long long same = __ballot(code == lead);
        if (lane == leader) atomicAdd(counter + lead, (T)__popcll(same));
        if (code == lead) code = kNoCode;
        pending &= ~same;
    }
    if (code != kNoCode) atomicAdd(counter + code, (T)1);
}

// grid (blocks of an entry, B); dynamic LDS: keys, slots [nl] and, with LDS_TABLE, (nl + 1)^2 counters
template <bool LDS_TABLE>
__global__ void __launch_bounds__(kThreads)
ls_confusion(const int *__restrict__ a, const int *__restrict__ b, const int *__restrict__ table, int nl, unsigned V, unsigned per,
             unsigned long long *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ls_lds[];
    int *keys = (int *)ls_lds, *slots = keys + nl;
    unsigned *counter = (unsigned *)(slots + nl);
    const int ncounters = (nl + 1) * (nl + 1);
    const bool listed = table != nullptr;
    if (LDS_TABLE)
        for (int i = threadIdx.x; i < ncounters; i += kThreads) counter[i] = 0u;
    ls_stage_table(table, nl, keys, slots);
    __syncthreads();
    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    const unsigned beg = min(blockIdx.x * per, V), end = min(beg + per, V);
    const size_t base = (size_t)blockIdx.y * V;
    unsigned long long *out = counts + (size_t)blockIdx.y * ncounters;
    // (uniform per wave) four steps' loads at a time
    for (unsigned step = beg + (unsigned)(wave * NRT_WAVE); step < end; step += 4 * kThreads) {
        int ia[4], ib[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned v = step + (unsigned)(k * kThreads + lane);
            ok[k] = v < end;
            ia[k] = ok[k] ? a[base + v] : 0;
            ib[k] = ok[k] ? b[base + v] : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned code = ok[k] ? ls_pair(ls_slot(keys, slots, listed, nl, ia[k]), ls_slot(keys, slots, listed, nl, ib[k]), nl) : kNoCode;
            if (LDS_TABLE) ls_conf_add(counter, code, lane, 2);
            else ls_conf_add(out, code, lane, -1);
        }
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int i = threadIdx.x; i < ncounters; i += kThreads) {
            const unsigned c = counter[i];
            if (c != 0u) atomicAdd(out + i, (unsigned long long)c);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct LsPlan {
    LsGeom p;
    size_t rowlen, bytes;
};

inline bool ls_dtype_ok(int dtype) { return dtype == NRT_DT_F32 || dtype == NRT_DT_BF16 || dtype == NRT_DT_F16; }

// the argument checks the entry points share; `channels` 0: no image
inline int ls_check(int batch, const int *shape, int nd, int nlabels, int channels, bool image, long long &voxels) {
    if (batch < 1 || (nd != 2 && nd != 3)) return NRT_ERR_INVALID_ARG;
    bool wide = false;
    voxels = 1;
    for (int a = 0; a < nd; ++a) {
        if (shape[a] < 1) return NRT_ERR_INVALID_ARG;
        if (voxels >= (1LL << 31)) wide = true;                                      // (the product stays below 2^62)
        else voxels *= shape[a];
    }
    if (image && (channels < 1 || channels > kLsMaxChannels)) return NRT_ERR_INVALID_ARG;
    if (nlabels < 1 || nlabels > kLsMaxLabels) return NRT_ERR_INVALID_ARG;
    if (wide || batch > kMaxBatch || voxels >= (1LL << 31) || voxels * batch >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    return NRT_OK;
}

// a block's share: contiguous, a multiple of the block's 256 voxels per step, from the geometry alone
inline void ls_shares(int batch, long long voxels, unsigned &per, unsigned &blocks) {
    long long n = (voxels + kBlockVoxels - 1) / kBlockVoxels;
    const long long most = kTargetBlocks / batch > 1 ? kTargetBlocks / batch : 1;
    if (n > most) n = most;
    long long share = (voxels + n - 1) / n;
    share = (share + kThreads - 1) / kThreads * kThreads;
    per = (unsigned)share;
    blocks = (unsigned)((voxels + share - 1) / share);
}

inline void ls_plan(int batch, long long voxels, const int *shape, int nd, int nlabels, int channels, LsPlan &pl) {
    pl.p.g = ls_shape(shape, nd);
    pl.p.V = (unsigned)voxels;
    pl.p.nd = nd;
    pl.p.nl = nlabels;
    ls_shares(batch, voxels, pl.p.per, pl.p.blocks);
    pl.rowlen = (size_t)nlabels * channels * 2;
    pl.bytes = (size_t)kTableWords * sizeof(int) + (size_t)batch * pl.p.blocks * pl.rowlen * sizeof(double);
}

template <int C>
inline void ls_launch_main(const int *ids, const void *image, int dt, const int *table, const LsPlan &pl, int batch, const LsOut &o,
                           double *rows, hipStream_t st) {
    const size_t lds = (size_t)pl.p.nl * (60 + 40 * C);
    hipLaunchKernelGGL(ls_main<C>, dim3(pl.p.blocks, (unsigned)batch), dim3(kThreads), lds, st, ids, image, dt, table, pl.p, o, rows);
}

}  // namespace

// What nrt_label_stats of this geometry needs (channels 0: no image); 0 for a geometry the call refuses.
extern "C" size_t nrt_label_stats_workspace_bytes(int batch, const int shape[], int nd, int nlabels, int channels) {
    long long voxels;
    if (!shape || channels < 0 || channels > kLsMaxChannels) return 0;
    if (ls_check(batch, shape, nd, nlabels, channels, false, voxels) != NRT_OK) return 0;
    LsPlan pl;
    ls_plan(batch, voxels, shape, nd, nlabels, channels, pl);
    return pl.bytes;
}

extern "C" int nrt_label_stats(const int *ids, const int *labels, int nlabels, const void *image, int dtype, int channels, int batch,
                               const int shape[], int nd, long long *counts, long long *coord_sums, int *bbox, double *sums,
                               float *minmax, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ids || !counts || !shape) return NRT_ERR_INVALID_ARG;
    if (!image && (sums || minmax)) return NRT_ERR_INVALID_ARG;
    if (image && !ls_dtype_ok(dtype)) return NRT_ERR_INVALID_ARG;
    long long voxels;
    const int rc = ls_check(batch, shape, nd, nlabels, channels, image != nullptr, voxels);
    if (rc != NRT_OK) return rc;
    const int C = (image && (sums || minmax)) ? channels : 0;                        // (an image nothing is asked of is not read)
    LsPlan pl;
    ls_plan(batch, voxels, shape, nd, nlabels, C, pl);
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < pl.bytes) return NRT_ERR_WORKSPACE;

    hipStream_t st = nrt_stream(stream);
    int *table = (int *)workspace;
    double *rows = (double *)(table + kTableWords);
    const LsOut o = {(unsigned long long *)counts, (unsigned long long *)coord_sums, bbox, sums, (unsigned *)minmax};
    const size_t slots = (size_t)batch * nlabels, n_mm = minmax ? (size_t)batch * pl.rowlen : 0;
    const size_t n_cs = coord_sums ? slots * nd : 0, n_bbox = bbox ? slots * 2 * nd : 0;
    size_t most = slots * 2 * nd > n_mm ? slots * 2 * nd : n_mm;
    unsigned init_blocks = (unsigned)((most + kThreads - 1) / kThreads);
    if (init_blocks > 1024u) init_blocks = 1024u;
    hipLaunchKernelGGL(ls_init, dim3(init_blocks), dim3(kThreads), 0, st, labels, nlabels, table, o, slots, n_cs, n_bbox, n_mm, pl.p.g, nd);
    NRT_CHECK_LAUNCH();
    const int *tab = labels ? table : nullptr;
    if (C == 0) ls_launch_main<0>(ids, image, dtype, tab, pl, batch, o, rows, st);
    else if (C == 1) ls_launch_main<1>(ids, image, dtype, tab, pl, batch, o, rows, st);
    else if (C == 2) ls_launch_main<2>(ids, image, dtype, tab, pl, batch, o, rows, st);
    else if (C == 3) ls_launch_main<3>(ids, image, dtype, tab, pl, batch, o, rows, st);
    else ls_launch_main<4>(ids, image, dtype, tab, pl, batch, o, rows, st);
    NRT_CHECK_LAUNCH();
    if (C > 0) {
        const size_t total = (size_t)batch * pl.rowlen;
        hipLaunchKernelGGL(ls_finish, dim3((unsigned)((total + kFinishCols - 1) / kFinishCols)), dim3(kThreads), 0, st, (const double *)rows,
                           pl.p.blocks, pl.rowlen, total, o);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}

// What nrt_label_confusion_i32 of this geometry needs: the sorted label list; 0 for a geometry the call refuses.
extern "C" size_t nrt_label_confusion_workspace_bytes(int batch, long long voxels, int nlabels) {
    if (batch < 1 || voxels < 1 || nlabels < 1 || nlabels > kLsMaxLabels) return 0;
    if (batch > kMaxBatch || voxels >= (1LL << 31) || voxels * batch >= (1LL << 31)) return 0;
    return (size_t)kTableWords * sizeof(int);
}

extern "C" int nrt_label_confusion_i32(const int *a, const int *b, const int *labels, int nlabels, int batch, long long voxels,
                                       long long *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (!a || !b || !counts) return NRT_ERR_INVALID_ARG;
    if (batch < 1 || voxels < 1 || nlabels < 1 || nlabels > kLsMaxLabels) return NRT_ERR_INVALID_ARG;
    if (batch > kMaxBatch || voxels >= (1LL << 31) || voxels * batch >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < (size_t)kTableWords * sizeof(int)) return NRT_ERR_WORKSPACE;

    hipStream_t st = nrt_stream(stream);
    int *table = (int *)workspace;
    const size_t ncounters = (size_t)(nlabels + 1) * (nlabels + 1), n_counts = (size_t)batch * ncounters;
    const LsOut o = {(unsigned long long *)counts, nullptr, nullptr, nullptr, nullptr};
    unsigned init_blocks = (unsigned)((n_counts + kThreads - 1) / kThreads);
    if (init_blocks > 1024u) init_blocks = 1024u;
    const LsShape none = {{1u, 1u, 1u}};
    hipLaunchKernelGGL(ls_init, dim3(init_blocks), dim3(kThreads), 0, st, labels, nlabels, table, o, n_counts, (size_t)0, (size_t)0,
                       (size_t)0, none, 3);
    NRT_CHECK_LAUNCH();
    unsigned per, blocks;
    ls_shares(batch, voxels, per, blocks);
    const dim3 grid(blocks, (unsigned)batch), block(kThreads);
    const int *tab = labels ? table : nullptr;
    const size_t lds_table = 2 * (size_t)nlabels * sizeof(int);
    if (nlabels <= kConfLdsLabels)
        hipLaunchKernelGGL(ls_confusion<true>, grid, block, lds_table + ncounters * sizeof(unsigned), st, a, b, tab, nlabels,
                           (unsigned)voxels, per, (unsigned long long *)counts);
    else
        hipLaunchKernelGGL(ls_confusion<false>, grid, block, lds_table, st, a, b, tab, nlabels, (unsigned)voxels, per,
                           (unsigned long long *)counts);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
