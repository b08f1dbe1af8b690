// Binary morphology, flat grey morphology (box minimum / maximum) and box rank filters of 2-D and 3-D volumes: what
// scipy.ndimage.binary_erosion / binary_dilation, minimum_filter / maximum_filter and rank_filter / median_filter / percentile_filter
// give on the host.  Every result is an exact integer or order statistic.
//
// nrt_binary_morph: one voxel is one bit (morph_core.h).  A block of 4 waves owns a tile of rows along the last axis.  It packs the
//   rows of its footprint (the tile and a halo of k rows on every side, kMbFootprint rows across in each row axis) into LDS: a wave's
//   ballot over 64 consecutive voxels of a row IS the packed word, and rows outside the volume and the bits past the end of a row
//   take the border value.  Then k steps on two LDS buffers: a step forms every word of the still valid region (one row less on every
//   side per step) from its neighbour rows by mc_step_word, rows outside the volume being set to the border value again.  Last the
//   tile is written out as bytes.  Nothing packed ever reaches global memory.  More than kMbSteps iterations are further launches
//   through the workspace (one byte per voxel); the composition is exact because the outside is re-imposed at every step.
// nrt_minmax_filter: one running minimum / maximum pass per axis whose size is above 1, each out of place (x -> workspace -> out, so
//   that the last pass writes out).  A block stages a tile of lines with its halo in LDS (the boundary mode is folded into the staging
//   index, mc_fold) and every thread scans its window there.
// nrt_rank_filter: a block stages its tile and halo in LDS; a thread reads its N <= 27 samples into registers (the LDS offsets of the
//   window come as kernel arguments), pads them to 16 or 32 with the largest value, sorts them by a fixed bitonic network of
//   compare-exchanges and picks the rank by a chain of selects: no data-dependent branch, no run-time index into the registers.
// No atomics, no workgroup waits for another, nothing goes to the host, nothing is allocated: the calls capture into a graph and are
// bit-identical from run to run.
#include "nrt_common.h"

#include <limits.h>

#include "morph_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kMaxBatch = 65535;

// ---- binary --------------------------------------------------------------------------------------------------------------------------
constexpr int kMbFootprint = 16;                     // rows of the footprint in each row axis (3-D); 16 * 16 rows * 16 words * 2 buffers = 64 KB
constexpr int kMbSteps = 4;                          // iterations of one launch: the tile is then 8 x 8 rows
constexpr int kMbRows2d = 32;                        // 2-D: rows of the footprint along the one row axis (256 left a 256^2 image 2 blocks)

struct MbGeom {
    int Z, Y, X, W;                                  // extents (Z = 1 for 2-D) and the words of a row
    int FZ, FY, hz, k;                               // footprint rows, the halo along z (0 for 2-D) and along y = the steps of the launch
    unsigned structure;                              // already reflected for a dilation
    int any, border, dtype;
};

__device__ __forceinline__ bool mb_is_set(const void *x, int dt, size_t at) {
    if (dt == NRT_DT_U8) return ((const unsigned char *)x)[at] != 0;
    if (dt == NRT_DT_I32) return ((const int *)x)[at] != 0;
    return ((const float *)x)[at] != 0.0f;                                  // (-0.0 is not set, a NaN is)
}

__global__ void __launch_bounds__(kThreads)
mb_morph(const void *__restrict__ x, unsigned char *__restrict__ out, MbGeom g) {
    extern __shared__ uint64_t mb_lds[];
    const int rows = g.FZ * g.FY, W = g.W;
    uint64_t *src = mb_lds, *dst = mb_lds + (size_t)rows * W;
    const int TZ = g.FZ - 2 * g.hz, TY = g.FY - 2 * g.k;
    const int z0 = (int)blockIdx.y * TZ - g.hz, y0 = (int)blockIdx.x * TY - g.k;
    const size_t base = (size_t)blockIdx.z * g.Z * g.Y * g.X;
    const int wave = threadIdx.x / NRT_WAVE, lane = threadIdx.x % NRT_WAVE;
    const uint64_t fill = mc_fill(g.border);

    for (int row = wave; row < rows; row += kWaves) {                       // pack: a ballot is a word
        const int z = z0 + row / g.FY, y = y0 + row % g.FY;
        const bool inside = z >= 0 && z < g.Z && y >= 0 && y < g.Y;         // (wave-uniform)
        for (int w = 0; w < W; ++w) {
            uint64_t word = fill;
            if (inside) {
                const int xx = w * kMcWordBits + lane;
                const bool set = xx < g.X && mb_is_set(x, g.dtype, base + ((size_t)z * g.Y + y) * g.X + xx);
                word = mc_border_fill(__ballot(set), mc_tail_mask(g.X, w), g.border);
            }
            if (lane == 0) src[row * W + w] = word;
        }
    }
    __syncthreads();

    for (int s = 1; s <= g.k; ++s) {                                        // the region that is still valid loses a row per side
        const int zlo = g.hz ? s : 0, nz = g.FZ - 2 * zlo, ny = g.FY - 2 * s;
        const int items = nz * ny * W;
        for (int it = threadIdx.x; it < items; it += kThreads) {
            const int w = it % W, rr = it / W;
            const int fz = zlo + rr / ny, fy = s + rr % ny;
            const int z = z0 + fz, y = y0 + fy;
            uint64_t word = fill;
            if (z >= 0 && z < g.Z && y >= 0 && y < g.Y) {
                uint64_t nb[9][3];
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    if (!mc_row_bits(g.structure, r)) continue;             // (a 2-D launch names no row with dz != 0: checked by the host)
                    const uint64_t *p = src + ((fz + r / 3 - 1) * g.FY + (fy + r % 3 - 1)) * W;
                    nb[r][0] = w > 0 ? p[w - 1] : fill;
                    nb[r][1] = p[w];
                    nb[r][2] = w < W - 1 ? p[w + 1] : fill;
                }
                word = mc_border_fill(mc_step_word(nb, g.structure, g.any), mc_tail_mask(g.X, w), g.border);
            }
            dst[(fz * g.FY + fy) * W + w] = word;
        }
        __syncthreads();
        uint64_t *t = src;
        src = dst;
        dst = t;
    }

    for (int trow = wave; trow < TZ * TY; trow += kWaves) {
        const int tz = trow / TY, ty = trow % TY;
        const int z = z0 + g.hz + tz, y = y0 + g.k + ty;
        if (z >= g.Z || y >= g.Y) continue;
        const uint64_t *p = src + ((tz + g.hz) * g.FY + (ty + g.k)) * W;
        for (int w = 0; w < W; ++w) {
            const int xx = w * kMcWordBits + lane;
            if (xx < g.X) out[base + ((size_t)z * g.Y + y) * g.X + xx] = (unsigned char)((p[w] >> lane) & 1ull);
        }
    }
}

// ---- minimum / maximum along one axis ------------------------------------------------------------------------------------------------
constexpr int kMmMaxSize = 31;
constexpr int kMmLines = 4, kMmChunk = 256;          // last axis: 4 lines x 256 outputs per block, one output per thread and line
constexpr int kMmAxisTile = 32, kMmInnerTile = 64;   // a strided axis: 32 outputs along the axis x 64 along the memory order

template <bool MAX, typename T>
__device__ __forceinline__ T mm_op(T a, T b) {
    return MAX ? (b > a ? b : a) : (b < a ? b : a);
}

// x [lines, n] -> out: lanes run along the axis
template <typename T, bool MAX>
__global__ void __launch_bounds__(kThreads)
mm_last_axis(const T *__restrict__ x, T *__restrict__ out, unsigned lines, int n, int size, int mode, T cval, unsigned chunks) {
    __shared__ T tile[kMmLines][kMmChunk + kMmMaxSize - 1];
    const int r = size / 2, span = kMmChunk + 2 * r;
    const int c0 = (int)(blockIdx.x % chunks) * kMmChunk;
    const unsigned l0 = (blockIdx.x / chunks) * kMmLines;
    for (int idx = threadIdx.x; idx < kMmLines * span; idx += kThreads) {
        const int l = idx / span, j = idx % span;
        if (l0 + l >= lines) break;
        const int q = mc_fold(c0 - r + j, n, mode);
        tile[l][j] = q >= 0 ? x[(size_t)(l0 + l) * n + q] : cval;
    }
    __syncthreads();
    const int a = c0 + (int)threadIdx.x;
    if (a >= n) return;
    for (int l = 0; l < kMmLines && l0 + l < lines; ++l) {
        T m = tile[l][threadIdx.x];
        for (int j = 1; j < size; ++j) m = mm_op<MAX>(m, tile[l][threadIdx.x + j]);
        out[(size_t)(l0 + l) * n + a] = m;
    }
}

// x [outer, n, inner] -> out, inner > 1: lanes run along inner
template <typename T, bool MAX>
__global__ void __launch_bounds__(kThreads)
mm_strided_axis(const T *__restrict__ x, T *__restrict__ out, int n, int inner, int size, int mode, T cval, unsigned tiles_i,
                unsigned tiles_a) {
    __shared__ T tile[kMmAxisTile + kMmMaxSize - 1][kMmInnerTile];
    const int r = size / 2;
    const int i = (int)(blockIdx.x % tiles_i) * kMmInnerTile + (int)(threadIdx.x % NRT_WAVE);
    const int a0 = (int)((blockIdx.x / tiles_i) % tiles_a) * kMmAxisTile;
    const size_t o = blockIdx.x / tiles_i / tiles_a;
    const int wave = threadIdx.x / NRT_WAVE, lane = threadIdx.x % NRT_WAVE;
    for (int j = wave; j < kMmAxisTile + 2 * r; j += kWaves) {
        const int q = mc_fold(a0 - r + j, n, mode);
        T v = cval;
        if (q >= 0 && i < inner) v = x[(o * n + q) * inner + i];
        tile[j][lane] = v;
    }
    __syncthreads();
    if (i >= inner) return;
    for (int a = wave; a < kMmAxisTile && a0 + a < n; a += kWaves) {
        T m = tile[a][lane];
        for (int j = 1; j < size; ++j) m = mm_op<MAX>(m, tile[a + j][lane]);
        out[(o * n + a0 + a) * inner + i] = m;
    }
}

// ---- rank ----------------------------------------------------------------------------------------------------------------------------
constexpr int kRkMaxSamples = 27;
constexpr int kRkTileX = 64;
constexpr size_t kRkMaxLds = 64 * 1024;

struct RkGeom {
    int Z, Y, X;
    int rz, ry, rx;                                  // the radii of the box
    int TZ, TY, FZ, FY, FX;                          // the tile (TZ x TY x 64) and its footprint
    unsigned tiles_x, tiles_y, tiles_z;
    int n, rank, mode;
    int off[kRkMaxSamples];                          // the LDS offset of every sample of the window from its first one
};

template <typename T> __device__ __forceinline__ T rk_pad();
template <> __device__ __forceinline__ float rk_pad<float>() { return __uint_as_float(0x7F800000u); }
template <> __device__ __forceinline__ int rk_pad<int>() { return INT_MAX; }

__device__ __forceinline__ void rk_exchange(float &a, float &b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}
__device__ __forceinline__ void rk_exchange(int &a, int &b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

template <typename T, int P>
__global__ void __launch_bounds__(kThreads)
rk_filter(const T *__restrict__ x, T *__restrict__ out, RkGeom g, T cval) {
    extern __shared__ unsigned char rk_lds[];
    T *tile = (T *)rk_lds;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % g.tiles_x) * kRkTileX;
    b /= g.tiles_x;
    const int y0 = (int)(b % g.tiles_y) * g.TY;
    b /= g.tiles_y;
    const int z0 = (int)(b % g.tiles_z) * g.TZ;
    const size_t base = (size_t)(b / g.tiles_z) * g.Z * g.Y * g.X;

    const int total = g.FZ * g.FY * g.FX;
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
        const int fx = idx % g.FX, fy = (idx / g.FX) % g.FY, fz = idx / (g.FX * g.FY);
        const int qz = mc_fold(z0 - g.rz + fz, g.Z, g.mode), qy = mc_fold(y0 - g.ry + fy, g.Y, g.mode),
                  qx = mc_fold(x0 - g.rx + fx, g.X, g.mode);
        tile[idx] = (qz >= 0 && qy >= 0 && qx >= 0) ? x[base + ((size_t)qz * g.Y + qy) * g.X + qx] : cval;
    }
    __syncthreads();

    const int lx = threadIdx.x % NRT_WAVE;
    if (x0 + lx >= g.X) return;
    for (int rr = threadIdx.x / NRT_WAVE; rr < g.TZ * g.TY; rr += kWaves) {
        const int tz = rr / g.TY, ty = rr % g.TY;
        if (z0 + tz >= g.Z || y0 + ty >= g.Y) continue;
        const T *first = tile + (tz * g.FY + ty) * g.FX + lx;
        T v[P];
#pragma unroll
        for (int i = 0; i < P; ++i) v[i] = (i < kRkMaxSamples && i < g.n) ? first[g.off[i < kRkMaxSamples ? i : 0]] : rk_pad<T>();
        // the bitonic network: every index below is a compile-time constant
#pragma unroll
        for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const int l = i ^ j;
                    if (l > i) {
                        if ((i & k) == 0) rk_exchange(v[i], v[l]);
                        else rk_exchange(v[l], v[i]);
                    }
                }
            }
        }
        T res = v[0];
#pragma unroll
        for (int i = 1; i < P; ++i) res = (g.rank == i) ? v[i] : res;
        out[base + ((size_t)(z0 + tz) * g.Y + (y0 + ty)) * g.X + (x0 + lx)] = res;
    }
}

// ---- the checks the entry points share -----------------------------------------------------------------------------------------------
int check_geometry(int batch, const int shape[], int nd, long long *voxels) {
    if (!shape || batch < 1 || (nd != 2 && nd != 3)) return NRT_ERR_INVALID_ARG;
    long long v = 1;
    bool wide = false;
    for (int a = 0; a < nd; ++a) {
        if (shape[a] < 1) return NRT_ERR_INVALID_ARG;
        v *= shape[a];
        if (v >= (1LL << 31)) wide = true, v = 1;
    }
    *voxels = wide ? (1LL << 31) : v;
    return NRT_OK;
}

int check_limits(int batch, long long voxels) {
    return (batch > kMaxBatch || voxels >= (1LL << 31) || voxels * batch >= (1LL << 31)) ? NRT_ERR_UNSUPPORTED : NRT_OK;
}

int passes_of(const int size[], int nd) {
    int p = 0;
    for (int a = 0; a < nd; ++a) p += size[a] > 1 ? 1 : 0;
    return p;
}

template <typename T, bool MAX>
void mm_launch(const T *x, T *out, size_t outer, int n, size_t inner, int size, int mode, T cval, hipStream_t st) {
    if (inner == 1) {
        const unsigned chunks = (unsigned)((n + kMmChunk - 1) / kMmChunk);
        const size_t blocks = ((outer + kMmLines - 1) / kMmLines) * chunks;
        hipLaunchKernelGGL((mm_last_axis<T, MAX>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, out, (unsigned)outer, n, size, mode, cval,
                           chunks);
    } else {
        const unsigned tiles_i = (unsigned)((inner + kMmInnerTile - 1) / kMmInnerTile);
        const unsigned tiles_a = (unsigned)((n + kMmAxisTile - 1) / kMmAxisTile);
        hipLaunchKernelGGL((mm_strided_axis<T, MAX>), dim3((unsigned)(outer * tiles_a * tiles_i)), dim3(kThreads), 0, st, x, out, n,
                           (int)inner, size, mode, cval, tiles_i, tiles_a);
    }
}

template <typename T>
int mm_run(const void *x, void *out, void *ws, int batch, const int shape[], int nd, const int size[], int mode, T cval, int want_max,
           hipStream_t st) {
    int left = passes_of(size, nd);
    const void *from = x;
    const bool identity = left == 0;                                        // every size is 1: one pass of size 1 copies
    if (identity) left = 1;
    for (int a = 0; a < nd; ++a) {
        if (!(size[a] > 1 || (identity && a == nd - 1))) continue;
        size_t outer = (size_t)batch, inner = 1;
        for (int b = 0; b < a; ++b) outer *= (size_t)shape[b];
        for (int b = a + 1; b < nd; ++b) inner *= (size_t)shape[b];
        --left;
        void *to = (left % 2 == 0) ? out : ws;                              // the last pass writes out
        if (want_max) mm_launch<T, true>((const T *)from, (T *)to, outer, shape[a], inner, size[a], mode, cval, st);
        else mm_launch<T, false>((const T *)from, (T *)to, outer, shape[a], inner, size[a], mode, cval, st);
        NRT_CHECK_LAUNCH();
        from = to;
    }
    return NRT_OK;
}

template <typename T>
int rk_run(const void *x, void *out, int batch, const RkGeom &g, size_t lds, T cval, hipStream_t st) {
    const unsigned blocks = g.tiles_x * g.tiles_y * g.tiles_z * (unsigned)batch;
    if (g.n <= 16) hipLaunchKernelGGL((rk_filter<T, 16>), dim3(blocks), dim3(kThreads), lds, st, (const T *)x, (T *)out, g, cval);
    else hipLaunchKernelGGL((rk_filter<T, 32>), dim3(blocks), dim3(kThreads), lds, st, (const T *)x, (T *)out, g, cval);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

}  // namespace

extern "C" size_t nrt_binary_morph_workspace_bytes(int batch, const int shape[], int nd, int iterations) {
    long long voxels = 0;
    if (check_geometry(batch, shape, nd, &voxels) != NRT_OK || check_limits(batch, voxels) != NRT_OK) return 0;
    return iterations > kMbSteps ? (size_t)batch * (size_t)voxels : 0;
}

extern "C" int nrt_binary_morph(const void *x, int dtype, int batch, const int shape[], int nd, int structure, int iterations,
                                int border_value, int dilate, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !out) return NRT_ERR_INVALID_ARG;
    if (dtype != NRT_DT_U8 && dtype != NRT_DT_I32 && dtype != NRT_DT_F32) return NRT_ERR_INVALID_ARG;
    long long voxels = 0;
    if (check_geometry(batch, shape, nd, &voxels) != NRT_OK) return NRT_ERR_INVALID_ARG;
    if (structure < 0 || ((unsigned)structure & ~kMcStructureBits) || (nd == 2 && ((unsigned)structure & ~mc_plane_mask())))
        return NRT_ERR_INVALID_ARG;
    if (iterations < 1 || (border_value != 0 && border_value != 1) || (dilate != 0 && dilate != 1)) return NRT_ERR_INVALID_ARG;
    if (check_limits(batch, voxels) != NRT_OK || shape[nd - 1] > kMcMaxWords * kMcWordBits) return NRT_ERR_UNSUPPORTED;
    // (the row tiles along the first of three axes are the grid's second dimension: 65535 tiles of at least 8 rows)
    if (nd == 3 && (shape[0] + kMbFootprint - 2 * kMbSteps - 1) / (kMbFootprint - 2 * kMbSteps) > 65535) return NRT_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)batch * (size_t)voxels;
    if (iterations > kMbSteps && (!workspace || workspace_bytes < bytes)) return NRT_ERR_WORKSPACE;

    hipStream_t st = nrt_stream(stream);
    MbGeom g;
    g.Z = nd == 3 ? shape[0] : 1;
    g.Y = shape[nd - 2];
    g.X = shape[nd - 1];
    g.W = mc_words(g.X);
    g.FZ = nd == 3 ? kMbFootprint : 1;
    g.FY = nd == 3 ? kMbFootprint : kMbRows2d;
    g.structure = dilate ? mc_reflect((unsigned)structure) : (unsigned)structure;
    g.any = dilate;
    g.border = border_value;
    int launches = (iterations + kMbSteps - 1) / kMbSteps, todo = iterations;
    const void *from = x;
    g.dtype = dtype;
    while (todo > 0) {
        g.k = todo < kMbSteps ? todo : kMbSteps;
        g.hz = nd == 3 ? g.k : 0;
        todo -= g.k;
        --launches;
        void *to = (launches % 2 == 0) ? out : workspace;                   // the last launch writes out
        const int TZ = g.FZ - 2 * g.hz, TY = g.FY - 2 * g.k;
        const dim3 grid((unsigned)((g.Y + TY - 1) / TY), (unsigned)((g.Z + TZ - 1) / TZ), (unsigned)batch);
        const size_t lds = 2 * (size_t)g.FZ * g.FY * g.W * sizeof(uint64_t);
        hipLaunchKernelGGL(mb_morph, grid, dim3(kThreads), lds, st, from, (unsigned char *)to, g);
        NRT_CHECK_LAUNCH();
        from = to;
        g.dtype = NRT_DT_U8;
    }
    return NRT_OK;
}

static int filter_checks(const void *x, int dtype, int batch, const int shape[], int nd, const int size[], int max_size, int mode,
                         double cval, const void *out, long long *voxels) {
    if (!x || !out || !size) return NRT_ERR_INVALID_ARG;
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_I32) return NRT_ERR_INVALID_ARG;
    if (check_geometry(batch, shape, nd, voxels) != NRT_OK) return NRT_ERR_INVALID_ARG;
    for (int a = 0; a < nd; ++a)
        if (size[a] < 1 || size[a] % 2 == 0) return NRT_ERR_INVALID_ARG;
    if (mode < kMcReflect || mode > kMcConstant || cval != cval) return NRT_ERR_INVALID_ARG;
    if (dtype == NRT_DT_I32 && (cval < (double)INT_MIN || cval > (double)INT_MAX)) return NRT_ERR_INVALID_ARG;
    for (int a = 0; a < nd; ++a)
        if (size[a] > max_size) return NRT_ERR_UNSUPPORTED;
    return check_limits(batch, *voxels);
}

extern "C" size_t nrt_minmax_filter_workspace_bytes(int batch, const int shape[], int nd, const int size[]) {
    long long voxels = 0;
    if (!size || check_geometry(batch, shape, nd, &voxels) != NRT_OK || check_limits(batch, voxels) != NRT_OK) return 0;
    return passes_of(size, nd) > 1 ? (size_t)batch * (size_t)voxels * 4 : 0;
}

extern "C" int nrt_minmax_filter(const void *x, int dtype, int batch, const int shape[], int nd, const int size[], int mode, double cval,
                                 int want_max, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    long long voxels = 0;
    const int rc = filter_checks(x, dtype, batch, shape, nd, size, kMmMaxSize, mode, cval, out, &voxels);
    if (rc != NRT_OK) return rc;
    if (want_max != 0 && want_max != 1) return NRT_ERR_INVALID_ARG;
    if (passes_of(size, nd) > 1 && (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < (size_t)batch * (size_t)voxels * 4))
        return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    if (dtype == NRT_DT_F32) return mm_run<float>(x, out, workspace, batch, shape, nd, size, mode, (float)cval, want_max, st);
    return mm_run<int>(x, out, workspace, batch, shape, nd, size, mode, (int)cval, want_max, st);
}

extern "C" int nrt_rank_filter(const void *x, int dtype, int batch, const int shape[], int nd, const int size[], int rank, int mode,
                               double cval, void *out, void *stream) {
    long long voxels = 0;
    const int rc = filter_checks(x, dtype, batch, shape, nd, size, kRkMaxSamples, mode, cval, out, &voxels);
    if (rc != NRT_OK) return rc;
    long long n = 1;
    for (int a = 0; a < nd; ++a) n *= size[a];
    if (n > kRkMaxSamples) return NRT_ERR_UNSUPPORTED;
    if (rank < 0 || rank >= n) return NRT_ERR_INVALID_ARG;

    RkGeom g;
    g.Z = nd == 3 ? shape[0] : 1;
    g.Y = shape[nd - 2];
    g.X = shape[nd - 1];
    const int sz = nd == 3 ? size[0] : 1, sy = size[nd - 2], sx = size[nd - 1];
    g.rz = sz / 2;
    g.ry = sy / 2;
    g.rx = sx / 2;
    g.TZ = g.Z == 1 ? 1 : 4;
    g.TY = g.Z == 1 ? 32 : 8;
    g.FX = kRkTileX + 2 * g.rx;
    size_t lds;
    for (;;) {                                                              // the footprint has to fit: halve the tile until it does
        g.FZ = g.TZ + 2 * g.rz;
        g.FY = g.TY + 2 * g.ry;
        lds = (size_t)g.FZ * g.FY * g.FX * 4;
        if (lds <= kRkMaxLds || (g.TZ == 1 && g.TY == 1)) break;
        if (g.TY > 1) g.TY /= 2;
        else g.TZ /= 2;
    }
    if (lds > kRkMaxLds) return NRT_ERR_UNSUPPORTED;
    g.tiles_x = (unsigned)((g.X + kRkTileX - 1) / kRkTileX);
    g.tiles_y = (unsigned)((g.Y + g.TY - 1) / g.TY);
    g.tiles_z = (unsigned)((g.Z + g.TZ - 1) / g.TZ);
    if ((unsigned long long)g.tiles_x * g.tiles_y * g.tiles_z * (unsigned long long)batch >= (1ull << 31)) return NRT_ERR_UNSUPPORTED;
    g.n = (int)n;
    g.rank = rank;
    g.mode = mode;
    int i = 0;
    for (int dz = 0; dz < sz; ++dz)
        for (int dy = 0; dy < sy; ++dy)
            for (int dx = 0; dx < sx; ++dx) g.off[i++] = (dz * g.FY + dy) * g.FX + dx;
    for (; i < kRkMaxSamples; ++i) g.off[i] = 0;

    hipStream_t st = nrt_stream(stream);
    if (dtype == NRT_DT_F32) return rk_run<float>(x, out, batch, g, lds, (float)cval, st);
    return rk_run<int>(x, out, batch, g, lds, (int)cval, st);
}
