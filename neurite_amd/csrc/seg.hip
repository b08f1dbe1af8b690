// Patch-wise volume prediction (neurite/tf/utils/seg.py): what turns the probability maps of overlapping patches into one label volume.
//
//   seg_argmax_group / seg_argmax_row   pred [n_vox, C] float32 / bfloat16 -> np.argmax over C (seg.py:301) and, in the same pass, the
//                                       probability of a label, pred[v, l] / sum_c pred[v, c] (prob_of_label, :230-260).
//     group arm (C % 4 == 0)            G lanes (a power of two up to 16) share a voxel: lane j loads the 8- / 16-byte pieces j, j + G, ...
//                                       of the row, keeps its best (value, index) pair and its sum, the pairs are merged by xor
//                                       shuffles (the lower index wins a tie) and the sums are added the same way.  The value of the
//                                       wanted label comes from the lane that loaded it, by one shuffle.
//     row arm (any C)                   a thread per voxel scans its row.
//   seg_recode                          out[v] = lookup[seg[v]], 0 outside the table (seg.py:355, tf.gather on the GPU).
//   seg_extract                         patches n0 .. n0 + count - 1 of a grid out of a channels-last volume: a copy in the widest
//                                       pieces (2 .. 16 bytes) that divide a voxel's channels.
//   seg_quilt_mean / seg_quilt_median   the inverse (pystrum's patchlib.quilt as seg.py:370 calls it): a thread per output element
//                                       finds the patches that cover its voxel from the coordinates and reads their values in ascending
//                                       patch index, NaN values skipped.  Mean: a float32 sum in that order.  Median: the values go to
//                                       the thread's column of LDS (at most 64), the two middle ranks are found by counting.
//
// No atomics, no workspace and no host reads; an output element is written by one thread from a fixed order of reads: results are
// run-to-run bit-identical.  Every index is checked against its tensor before it is used, a label outside the row reads nothing.
#include "nrt_common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 8192;         // the streaming kernels give a block one contiguous range (nrt_block_range)
constexpr int kMaxChannels = 256;
constexpr int kMaxGroup = 16;            // lanes per voxel in the group arm
constexpr int kMedianThreads = 128;      // 64 covers x 128 threads x 4 bytes = 32 KB of LDS at most
constexpr int kMedianMax = 64;
constexpr int kNone = INT_MAX;           // the index of "no value yet"
constexpr long long kMaxElems = 1LL << 31;

typedef unsigned seg_u4 __attribute__((ext_vector_type(4)));
typedef unsigned seg_u2 __attribute__((ext_vector_type(2)));
struct Bf16 {};

// W elements at element index e of `base`, widened to float32
template <typename ST, int W> struct SegIn;
template <> struct SegIn<float, 1> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[1]) { v[0] = ((const float *)b)[e]; }
};
template <> struct SegIn<float, 4> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[4]) {
        const nrt_f4 t = __builtin_nontemporal_load((const nrt_f4 *)((const float *)b + e));
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};
template <> struct SegIn<Bf16, 1> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[1]) {
        v[0] = __uint_as_float((unsigned)((const unsigned short *)b)[e] << 16);
    }
};
template <> struct SegIn<Bf16, 4> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[4]) {
        const seg_u2 t = __builtin_nontemporal_load((const seg_u2 *)((const unsigned short *)b + e));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            v[2 * j] = __uint_as_float(t[j] << 16);
            v[2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u);
        }
    }
};
template <> struct SegIn<Bf16, 8> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[8]) {
        const seg_u4 t = __builtin_nontemporal_load((const seg_u4 *)((const unsigned short *)b + e));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(t[j] << 16);
            v[2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u);
        }
    }
};

// does np.argmax prefer (ov, oi) to (bv, bi)?  A NaN is the maximum, the lower index wins among equals.  Branch-free; a lane
// without a value holds (-inf, kNone), which loses to every real pair and never wins.
__device__ __forceinline__ bool seg_beats(float ov, int oi, float bv, int bi) {
    const bool on = ov != ov, bn = bv != bv;
    const bool gt = ov > bv, eq = ov == bv;                             // both false where either is a NaN
    return (on & !bn) | gt | ((eq | (on & bn)) & (oi < bi));
}

// the label whose probability voxel v wants: of[v] if it lies in [0, C), else -1
__device__ __forceinline__ int seg_wanted(const void *of, int of64, long long v, int C) {
    const long long l = of64 ? ((const long long *)of)[v] : (long long)((const int *)of)[v];
    return (l >= 0 && l < C) ? (int)l : -1;
}

struct SegOut {
    void *labels;            // or NULL
    const void *of;          // or NULL: the probability of the arg-max
    float *prob;             // or NULL
    int labels64, of64;
};

__device__ __forceinline__ void seg_store(const SegOut &o, long long v, int best, float pv, float sum) {
    if (o.labels) {
        if (o.labels64) ((long long *)o.labels)[v] = best;
        else ((int *)o.labels)[v] = best;
    }
    if (o.prob) o.prob[v] = pv / sum;
}

// ------------------------------------------------------------------------------------------------------------------------------
// arg-max, group arm: C % W == 0.  G lanes share a voxel, lane j owns the pieces j, j + G, ..., P of them at most, so P G >= C / W.
// A pass takes U = 4 / P voxels per group: their U P loads are issued before the first value is looked at.
// ------------------------------------------------------------------------------------------------------------------------------
template <typename ST, int W, int P, bool PROB>
__global__ void __launch_bounds__(kThreads)
seg_argmax_group(const void *__restrict__ pred, long long nvox, int C, int G, SegOut o) {
    constexpr int U = 4 / P;
    const int NG = kThreads / G;
    const int lg = threadIdx.x & (G - 1), g = threadIdx.x / G;
    const int lane0 = (threadIdx.x & (NRT_WAVE - 1)) - lg;               // the group's first lane in its wave
    const int Q = C / W;
    const float ninf = -__builtin_inff();
    long long vbeg, vend;
    nrt_block_range(nvox, (long long)U * NG, vbeg, vend);
    for (long long v0 = vbeg + g; v0 < vend; v0 += (long long)U * NG) {  // (the lanes of a group agree on v0)
        float x[U][P][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long v = v0 + (long long)u * NG;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int q = lg + p * G;
                if (v < vend && q < Q) SegIn<ST, W>::load(pred, v * C + (long long)q * W, x[u][p]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long v = v0 + (long long)u * NG;
            const bool live = v < vend;
            int want = -1;
            if (PROB && o.of && live) want = seg_wanted(o.of, o.of64, v, C);
            float bv = ninf, sum = 0.0f, pv = __builtin_nanf("");
            int bi = lg < Q ? lg * W : kNone;                           // -inf at the lane's first index: what an all -inf lane answers
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int q = lg + p * G;
                if (live && q < Q) {
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const int c = q * W + j;
                        const float xj = x[u][p][j];
                        const bool take = !(xj <= bv) & (bv == bv);     // in ascending index: larger, or the first NaN
                        bv = take ? xj : bv;
                        bi = take ? c : bi;
                        if (PROB) {
                            sum += xj;
                            pv = c == want ? xj : pv;
                        }
                    }
                }
            }
            for (int off = 1; off < G; off <<= 1) {
                const float ov = __shfl_xor(bv, off, NRT_WAVE);
                const int oi = __shfl_xor(bi, off, NRT_WAVE);
                const bool take = seg_beats(ov, oi, bv, bi);
                bv = take ? ov : bv;
                bi = take ? oi : bi;
                // (nrt_wave_sum over the group, by hand: G is a run-time value and the loop is the arg-max's)
                if (PROB) sum += __shfl_xor(sum, off, NRT_WAVE);
            }
            if (PROB) {
                if (o.of) pv = __shfl(pv, lane0 + (want < 0 ? 0 : (want / W) & (G - 1)), NRT_WAVE);  // from the lane that loaded it
                else pv = bv;
            }
            if (live && lg == 0) seg_store(o, v, bi, pv, sum);
        }
    }
}

// arg-max, row arm: a thread per voxel
template <typename ST>
__global__ void __launch_bounds__(kThreads)
seg_argmax_row(const void *__restrict__ pred, long long nvox, int C, SegOut o) {
    long long vbeg, vend;
    nrt_block_range(nvox, kThreads, vbeg, vend);
    for (long long v = vbeg + threadIdx.x; v < vend; v += kThreads) {
        const int want = (o.prob && o.of) ? seg_wanted(o.of, o.of64, v, C) : -1;
        float bv = -__builtin_inff(), sum = 0.0f, pv = __builtin_nanf("");
        int bi = kNone;
        for (int c = 0; c < C; ++c) {
            float x[1];
            SegIn<ST, 1>::load(pred, v * C + c, x);
            if (seg_beats(x[0], c, bv, bi)) { bv = x[0]; bi = c; }
            sum += x[0];
            if (c == want) pv = x[0];
        }
        if (o.prob && !o.of) pv = bv;
        seg_store(o, v, bi, pv, sum);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// recode
// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
seg_recode(const void *__restrict__ seg, int seg64, long long n, const float *__restrict__ lookup, long long nlookup,
           float *__restrict__ out) {
    long long beg, end;
    nrt_block_range(n, kThreads, beg, end);
    for (long long v = beg + threadIdx.x; v < end; v += kThreads) {
        const long long l = seg64 ? ((const long long *)seg)[v] : (long long)((const int *)seg)[v];
        out[v] = (l >= 0 && l < nlookup) ? lookup[l] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// patches.  Axes are padded in front to rank 3 with size 1, stride 1, grid 1.
// ------------------------------------------------------------------------------------------------------------------------------
struct PatchGeom {
    int vol[3], patch[3], stride[3], grid[3];
};

template <typename U>                    // a piece of 2 .. 16 bytes; cu pieces per voxel
__global__ void __launch_bounds__(kThreads)
seg_extract(const U *__restrict__ vol, U *__restrict__ out, PatchGeom P, int cu, long long n0, long long npieces) {
    long long beg, end;
    nrt_block_range(npieces, kThreads, beg, end);
    for (long long u = beg + threadIdx.x; u < end; u += kThreads) {
        const int c = (int)(u % cu);
        long long t = u / cu;
        const int p2 = (int)(t % P.patch[2]); t /= P.patch[2];
        const int p1 = (int)(t % P.patch[1]); t /= P.patch[1];
        const int p0 = (int)(t % P.patch[0]); t /= P.patch[0];
        long long n = n0 + t;
        const int g2 = (int)(n % P.grid[2]); n /= P.grid[2];
        const int g1 = (int)(n % P.grid[1]); n /= P.grid[1];
        const int g0 = (int)n;                                          // < grid[0]: n0 + count <= prod(grid)
        const long long src = ((long long)(g0 * P.stride[0] + p0) * P.vol[1] + (g1 * P.stride[1] + p1)) * P.vol[2] + (g2 * P.stride[2] + p2);
        out[u] = vol[src * cu + c];
    }
}

// which grid indices along an axis cover coordinate x: [lo, hi], empty where a stride larger than the patch leaves a gap
__device__ __forceinline__ void seg_cover(int x, int patch, int stride, int grid, int &lo, int &hi) {
    lo = x >= patch ? (x - patch) / stride + 1 : 0;
    hi = min(grid - 1, x / stride);
}

__device__ __forceinline__ float seg_value(const float *p, long long i) { return p[i]; }
__device__ __forceinline__ float seg_value(const int *p, long long i) { return (float)p[i]; }

// the values that cover output element e, in ascending patch index, NaN values left out: f(value) for each
template <typename T, typename F>
__device__ __forceinline__ void seg_for_covers(const T *__restrict__ patches, const PatchGeom &P, int C, long long e, F f) {
    const int c = (int)(e % C);
    long long t = e / C;
    const int x2 = (int)(t % P.vol[2]); t /= P.vol[2];
    const int x1 = (int)(t % P.vol[1]); t /= P.vol[1];
    const int x0 = (int)t;
    int lo0, hi0, lo1, hi1, lo2, hi2;
    seg_cover(x0, P.patch[0], P.stride[0], P.grid[0], lo0, hi0);
    seg_cover(x1, P.patch[1], P.stride[1], P.grid[1], lo1, hi1);
    seg_cover(x2, P.patch[2], P.stride[2], P.grid[2], lo2, hi2);
    for (int g0 = lo0; g0 <= hi0; ++g0)
        for (int g1 = lo1; g1 <= hi1; ++g1)
            for (int g2 = lo2; g2 <= hi2; ++g2) {
                const long long n = ((long long)g0 * P.grid[1] + g1) * P.grid[2] + g2;
                const int p0 = x0 - g0 * P.stride[0], p1 = x1 - g1 * P.stride[1], p2 = x2 - g2 * P.stride[2];      // each in [0, patch)
                const long long i = ((((n * P.patch[0] + p0) * P.patch[1] + p1) * P.patch[2] + p2) * C) + c;
                const float v = seg_value(patches, i);
                if (v == v) f(v);
            }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
seg_quilt_mean(const T *__restrict__ patches, float *__restrict__ vol, PatchGeom P, int C, long long nout) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= nout) return;
    float sum = 0.0f;
    int k = 0;
    seg_for_covers(patches, P, C, e, [&](float v) { sum += v; ++k; });
    vol[e] = k ? sum / (float)k : __builtin_nanf("");
}

template <typename T>
__global__ void __launch_bounds__(kMedianThreads)
seg_quilt_median(const T *__restrict__ patches, float *__restrict__ vol, PatchGeom P, int C, long long nout, int cap) {
    extern __shared__ float seg_cols[];                                 // [cap][kMedianThreads]: a column per thread
    const long long e = (long long)blockIdx.x * kMedianThreads + threadIdx.x;
    if (e >= nout) return;
    float *col = seg_cols + threadIdx.x;
    int m = 0;
    seg_for_covers(patches, P, C, e, [&](float v) {
        if (m < cap) col[m * kMedianThreads] = v;                       // (the host's cap is the largest count there can be)
        ++m;
    });
    if (m > cap) m = cap;
    if (m == 0) {
        vol[e] = __builtin_nanf("");
        return;
    }
    // ranks are distinct: equal values are ordered by their place
    const int r_lo = (m - 1) >> 1, r_hi = m >> 1;
    float a = 0.0f, b = 0.0f;
    for (int i = 0; i < m; ++i) {
        const float vi = col[i * kMedianThreads];
        int r = 0;
        for (int j = 0; j < m; ++j) {
            const float vj = col[j * kMedianThreads];
            r += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
        }
        if (r == r_lo) a = vi;
        if (r == r_hi) b = vi;
    }
    vol[e] = r_lo == r_hi ? a : (a + b) / 2.0f;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline bool aligned_to(const void *p, size_t n) { return (((uintptr_t)p) & (n - 1)) == 0; }

inline unsigned stream_blocks(long long n, long long per_pass) {
    long long nb = (n + per_pass - 1) / per_pass;
    if (nb > kMaxBlocks) nb = kMaxBlocks;
    return (unsigned)(nb < 1 ? 1 : nb);
}

template <typename ST, int W, int P>
int launch_group_p(const void *pred, long long nvox, int C, const SegOut &o, hipStream_t st) {
    const int Q = C / W;
    int G = 1;
    while (G * P < Q) G <<= 1;
    const unsigned blocks = stream_blocks(nvox, 4LL * (4 / P) * (kThreads / G));
    if (o.prob) hipLaunchKernelGGL((seg_argmax_group<ST, W, P, true>), dim3(blocks), dim3(kThreads), 0, st, pred, nvox, C, G, o);
    else hipLaunchKernelGGL((seg_argmax_group<ST, W, P, false>), dim3(blocks), dim3(kThreads), 0, st, pred, nvox, C, G, o);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

// As many lanes per voxel as there are pieces, up to kMaxGroup: a load instruction then covers a voxel's whole row, or 16 pieces in a
// run.  Measured at 4 x 160^3 x 32 float32 (8 pieces; profiles/seg/lanes_per_voxel_sweep.jsonl): 8 lanes with one piece each 0.43 ms,
// 4 lanes with two 0.59 ms, 2 lanes with four 1.33 ms.  More than kMaxGroup pieces take two per lane, more than 2 kMaxGroup four:
// C <= 256 reaches that only with 4-element pieces (W = 8 has at most 32 pieces), so no four-piece kernel is built for W = 8.
template <typename ST, int W>
int launch_group(const void *pred, long long nvox, int C, const SegOut &o, hipStream_t st) {
    const int Q = C / W;
    if (Q <= kMaxGroup) return launch_group_p<ST, W, 1>(pred, nvox, C, o, st);
    if constexpr (W * 2 * kMaxGroup >= kMaxChannels) {
        return launch_group_p<ST, W, 2>(pred, nvox, C, o, st);
    } else {
        if (Q <= 2 * kMaxGroup) return launch_group_p<ST, W, 2>(pred, nvox, C, o, st);
        return launch_group_p<ST, W, 4>(pred, nvox, C, o, st);
    }
}

template <typename ST>
int launch_row(const void *pred, long long nvox, int C, const SegOut &o, hipStream_t st) {
    hipLaunchKernelGGL((seg_argmax_row<ST>), dim3(stream_blocks(nvox, kThreads)), dim3(kThreads), 0, st, pred, nvox, C, o);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

// checks the arrays of a patch grid and pads them to rank 3; *patch_vox, *npatches, *out_vox (the quilted volume) as products
inline int make_geom(int ndim, const int *patch, const int *stride, const int *grid, PatchGeom &P, long long &patch_vox,
                     long long &npatches, long long &quilt_vox) {
    if (ndim < 1 || ndim > 3 || !patch || !stride || !grid) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < ndim; ++d)
        if (patch[d] < 1 || stride[d] < 1 || grid[d] < 1) return NRT_ERR_INVALID_ARG;
    patch_vox = npatches = quilt_vox = 1;
    for (int d = 0; d < 3; ++d) {
        const int s = d - (3 - ndim);
        P.patch[d] = s < 0 ? 1 : patch[s];
        P.stride[d] = s < 0 ? 1 : stride[s];
        P.grid[d] = s < 0 ? 1 : grid[s];
        const long long ext = (long long)(P.grid[d] - 1) * P.stride[d] + P.patch[d];
        if (ext >= kMaxElems) return NRT_ERR_UNSUPPORTED;
        P.vol[d] = (int)ext;
        patch_vox *= P.patch[d];
        npatches *= P.grid[d];
        quilt_vox *= ext;
        if (patch_vox >= kMaxElems || npatches >= kMaxElems || quilt_vox >= kMaxElems) return NRT_ERR_UNSUPPORTED;
    }
    return NRT_OK;
}

template <typename U>
int launch_extract(const void *vol, void *out, const PatchGeom &P, int cu, long long n0, long long npieces, hipStream_t st) {
    hipLaunchKernelGGL((seg_extract<U>), dim3(stream_blocks(npieces, 4LL * kThreads)), dim3(kThreads), 0, st, (const U *)vol, (U *)out, P, cu,
                       n0, npieces);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

template <typename T>
int launch_quilt(const void *patches, float *vol, const PatchGeom &P, int C, long long nout, int reduce, int cap, hipStream_t st) {
    if (reduce == NRT_QUILT_MEAN) {
        hipLaunchKernelGGL((seg_quilt_mean<T>), dim3((unsigned)((nout + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const T *)patches,
                           vol, P, C, nout);
    } else {
        hipLaunchKernelGGL((seg_quilt_median<T>), dim3((unsigned)((nout + kMedianThreads - 1) / kMedianThreads)), dim3(kMedianThreads),
                           (size_t)cap * kMedianThreads * sizeof(float), st, (const T *)patches, vol, P, C, nout, cap);
    }
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

}  // namespace

extern "C" int nrt_seg_argmax(const void *pred, int dtype, long long n_vox, int channels, void *labels, int labels_i64,
                              const void *of_labels, int of_labels_i64, float *prob, void *stream) {
    if (!pred || (!labels && !prob) || (of_labels && !prob) || n_vox < 1 || channels < 1) return NRT_ERR_INVALID_ARG;
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_BF16) return NRT_ERR_UNSUPPORTED;
    if (channels > kMaxChannels || n_vox >= kMaxElems || n_vox * channels >= kMaxElems) return NRT_ERR_UNSUPPORTED;
    const SegOut o = {labels, of_labels, prob, labels_i64 ? 1 : 0, of_labels_i64 ? 1 : 0};
    hipStream_t st = nrt_stream(stream);
    const int C = channels;
    if (dtype == NRT_DT_F32) {
        if (C % 4 == 0 && aligned_to(pred, 16)) return launch_group<float, 4>(pred, n_vox, C, o, st);
        return launch_row<float>(pred, n_vox, C, o, st);
    }
    if (C % 8 == 0 && aligned_to(pred, 16)) return launch_group<Bf16, 8>(pred, n_vox, C, o, st);
    if (C % 4 == 0 && aligned_to(pred, 8)) return launch_group<Bf16, 4>(pred, n_vox, C, o, st);
    return launch_row<Bf16>(pred, n_vox, C, o, st);
}

extern "C" int nrt_seg_recode(const void *seg, int seg_i64, long long n, const float *lookup, long long n_lookup, float *out,
                              void *stream) {
    if (!seg || !lookup || !out || n < 1 || n_lookup < 1) return NRT_ERR_INVALID_ARG;
    if (n >= kMaxElems || n_lookup >= kMaxElems) return NRT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(seg_recode, dim3(stream_blocks(n, 4LL * kThreads)), dim3(kThreads), 0, nrt_stream(stream), seg, seg_i64 ? 1 : 0, n,
                       lookup, n_lookup, out);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_patch_extract(const void *vol, int dtype, int ndim, const int *vol_shape, int channels, const int *patch_size,
                                 const int *patch_stride, const int *grid_size, long long n0, long long count, void *patches,
                                 void *stream) {
    if (!vol || !patches || !vol_shape || channels < 1 || count < 1 || n0 < 0) return NRT_ERR_INVALID_ARG;
    PatchGeom P;
    long long patch_vox, npatches, quilt_vox;
    const int rc = make_geom(ndim, patch_size, patch_stride, grid_size, P, patch_vox, npatches, quilt_vox);
    if (rc == NRT_ERR_INVALID_ARG) return rc;
    long long vol_vox = 1;
    bool big = rc != NRT_OK;
    for (int d = 0; d < ndim; ++d) {
        if (vol_shape[d] < 1) return NRT_ERR_INVALID_ARG;
        if (!big && vol_vox * vol_shape[d] >= kMaxElems) big = true;
        if (!big) vol_vox *= vol_shape[d];
    }
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_BF16) return NRT_ERR_UNSUPPORTED;
    if (big || vol_vox * channels >= kMaxElems) return NRT_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d) {                                       // the grid fits inside the volume
        const int s = d - (3 - ndim);
        const int have = s < 0 ? 1 : vol_shape[s];
        if (P.vol[d] > have) return NRT_ERR_INVALID_ARG;
        P.vol[d] = have;
    }
    if (n0 + count > npatches) return NRT_ERR_INVALID_ARG;
    if (count * patch_vox >= kMaxElems || count * patch_vox * channels >= kMaxElems) return NRT_ERR_UNSUPPORTED;
    const int eb = dtype == NRT_DT_F32 ? 4 : 2;
    const long long row = (long long)channels * eb;
    int piece = 16;
    while (piece > eb && (row % piece != 0 || !aligned_to(vol, piece) || !aligned_to(patches, piece))) piece >>= 1;
    const int cu = (int)(row / piece);
    const long long npieces = count * patch_vox * cu;
    hipStream_t st = nrt_stream(stream);
    switch (piece) {
        case 16: return launch_extract<seg_u4>(vol, patches, P, cu, n0, npieces, st);
        case 8: return launch_extract<seg_u2>(vol, patches, P, cu, n0, npieces, st);
        case 4: return launch_extract<unsigned>(vol, patches, P, cu, n0, npieces, st);
        default: return launch_extract<unsigned short>(vol, patches, P, cu, n0, npieces, st);
    }
}

extern "C" int nrt_patch_quilt(const void *patches, int dtype, int ndim, const int *patch_size, const int *patch_stride,
                               const int *grid_size, int channels, int reduce, float *vol, void *stream) {
    if (!patches || !vol || channels < 1 || (reduce != NRT_QUILT_MEAN && reduce != NRT_QUILT_MEDIAN)) return NRT_ERR_INVALID_ARG;
    PatchGeom P;
    long long patch_vox, npatches, quilt_vox;
    const int rc = make_geom(ndim, patch_size, patch_stride, grid_size, P, patch_vox, npatches, quilt_vox);
    if (rc == NRT_ERR_INVALID_ARG) return rc;
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_I32) return NRT_ERR_UNSUPPORTED;
    if (rc != NRT_OK) return rc;
    if (npatches * patch_vox >= kMaxElems || npatches * patch_vox * channels >= kMaxElems || quilt_vox * channels >= kMaxElems)
        return NRT_ERR_UNSUPPORTED;
    long long cover = 1;                                                // the most patches that can cover a voxel
    for (int d = 0; d < 3; ++d) {
        cover *= (P.patch[d] + P.stride[d] - 1) / P.stride[d];
        if (cover > kMedianMax) break;
    }
    if (reduce == NRT_QUILT_MEDIAN && cover > kMedianMax) return NRT_ERR_UNSUPPORTED;
    const long long nout = quilt_vox * channels;
    hipStream_t st = nrt_stream(stream);
    if (dtype == NRT_DT_F32) return launch_quilt<float>(patches, vol, P, channels, nout, reduce, (int)cover, st);
    return launch_quilt<int>(patches, vol, P, channels, nout, reduce, (int)cover, st);
}
