// SpatialTransformer on an affine matrix in one kernel, and the gradient wrt the matrix, gfx950.
//
// The two-kernel path (vxm.hip affine_shift, then a warp kernel of interpn.hip in NRT_LOC_SHIFT mode) writes a dense [B, *S', D] field and
// reads it back: at one channel in 3-D 12 B written, 12 B read, 4 B gathered, 4 B stored per voxel, of which the result needs 8.  Here the
// location of an output voxel is formed in registers from the 12 floats of the matrix, with the same roundings in the same order
// (affine_shift's p = (float)q - c, the row products added left to right, + M[i][D], - p_i; then load_loc's (float)q + shift), and the
// corner arithmetic, blend order and fill are interpn_generic's, so the result is bit for bit what the two kernels give.
//
// Lane mapping, forward and backward alike: one thread per work item, an item being one channel (any C), the whole 8- or 12-byte row of
// a voxel at two and three channels (a thread per channel repeats the index arithmetic per channel: 0.259 against 0.228 ms for the
// two-kernel path at 4 x 160^3 x 3) or, where C % 4 == 0 and the pointers allow, four channels moved as 16 bytes; items are numbered
// voxel-major, channel fastest, so a wave's stores (and its loads of
// grad_out) are one contiguous run, and neighbouring voxels along the last axis sample source points one matrix column apart: for the
// near-identity transforms of registration a wave's corner loads are nearly contiguous rows too.  The matrix is read through a
// block-uniform address (scalar loads).
//
// Backward wrt the matrix: grad_matrix[b][i][j] = sum_q gloc_i(q) p_j(q), p_D = 1, with gloc the d / d loc of backward.hip
// (interpn_bwd_generic).  The sum is linear in the channels, so every thread keeps D (D + 1) partial sums over its items, whatever
// channels they hold; they are added across the wave by shuffles, across the block's four waves through LDS, and the block stores one row
// into the workspace.  A second launch adds the rows of a matrix (of the whole batch when the transform is shared) in a fixed order in
// float64.  No gradient field, no atomics; the grid depends on the shapes only, so two runs give the same bits.

#include "affine_core.h"

namespace {

template <int V> struct Vec;
template <> struct Vec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float *p) { v[0] = *p; }
    __device__ __forceinline__ void store(float *p) const { __builtin_nontemporal_store(v[0], p); }
};
// two and three channels: the whole row of a voxel in one 8- or 12-byte access (global memory needs dword alignment only)
typedef float aw_f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float aw_f3u __attribute__((ext_vector_type(3), aligned(4)));
template <> struct Vec<2> {
    float v[2];
    __device__ __forceinline__ void load(const float *p) {
        const aw_f2u t = *(const aw_f2u *)p;
        v[0] = t[0]; v[1] = t[1];
    }
    __device__ __forceinline__ void store(float *p) const { __builtin_nontemporal_store((aw_f2u){v[0], v[1]}, (aw_f2u *)p); }
};
template <> struct Vec<3> {
    float v[3];
    __device__ __forceinline__ void load(const float *p) {
        const aw_f3u t = *(const aw_f3u *)p;
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
    }
    __device__ __forceinline__ void store(float *p) const { __builtin_nontemporal_store((aw_f3u){v[0], v[1], v[2]}, (aw_f3u *)p); }
};
template <> struct Vec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float *p) {
        const nrt_f4 t = *(const nrt_f4 *)p;
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    }
    __device__ __forceinline__ void store(float *p) const { __builtin_nontemporal_store((nrt_f4){v[0], v[1], v[2], v[3]}, (nrt_f4 *)p); }
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <int D, int METHOD, int V>
__global__ __launch_bounds__(256) void affine_warp_fwd(AffWarpArgs a) {
    const int b = blockIdx.y;
    float M[D][D + 1];
    load_matrix<D>(a, b, M);
    const float *vol = a.vol + (long long)b * a.vol_bs;
    float *out = a.out + (long long)b * a.out_bs;
    const unsigned CG = (unsigned)a.CG, C = (unsigned)a.C;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < a.nitems; e += gridDim.x * 256u) {
        const unsigned q = e / CG, ch = (e - q * CG) * V;
        float p[D], loc[D];
        affine_loc<D>(a, M, q, p, loc);
        const bool oob = a.has_fill ? affine_oob<D>(a, loc) : false;
        Vec<V> acc;
        if (METHOD == NRT_INTERP_NEAREST) {
            unsigned idx = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) idx = idx * (unsigned)a.S[d] + (unsigned)nearest_1d(loc[d], a.S[d]);
            acc.load(vol + (size_t)idx * C + ch);
        } else {
            int i0[D], i1[D];
            float w0[D], w1[D];
#pragma unroll
            for (int d = 0; d < D; ++d) corner_1d(loc[d], a.S[d], i0[d], i1[d], w0[d], w1[d]);
            Vec<V> v[1 << D];
            float wt[1 << D];
#pragma unroll
            for (int corner = 0; corner < (1 << D); ++corner) {                  // product([0,1], repeat=D) order
                unsigned idx = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int bit = (corner >> (D - 1 - d)) & 1;
                    idx = idx * (unsigned)a.S[d] + (unsigned)(bit ? i1[d] : i0[d]);
                    const float w = bit ? w1[d] : w0[d];
                    wt[corner] = (d == 0) ? w : nrt_mul(wt[corner], w);
                }
                v[corner].load(vol + (size_t)idx * C + ch);
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int corner = 0; corner < (1 << D); ++corner) s = nrt_add(s, nrt_mul(wt[corner], v[corner].v[k]));
                acc.v[k] = s;
            }
        }
        if (a.has_fill) {
#pragma unroll
            for (int k = 0; k < V; ++k) acc.v[k] = apply_fill(acc.v[k], oob, a.fill);
        }
        acc.store(out + (size_t)q * C + ch);
    }
}

// ---- backward wrt the matrix -----------------------------------------------------------------------------------------------------
template <int D, int V>
__global__ __launch_bounds__(256) void affine_warp_bwd(AffWarpArgs a) {
    constexpr int K = D * (D + 1);
    const int b = blockIdx.y;
    float M[D][D + 1];
    load_matrix<D>(a, b, M);
    const float *vol = a.vol + (long long)b * a.vol_bs;
    const float *go = a.gout + (long long)b * a.out_bs;
    const unsigned CG = (unsigned)a.CG, C = (unsigned)a.C;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0f;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < a.nitems; e += gridDim.x * 256u) {
        const unsigned q = e / CG, ch = (e - q * CG) * V;
        float p[D], loc[D];
        affine_loc<D>(a, M, q, p, loc);
        if (a.has_fill && affine_oob<D>(a, loc)) continue;                       // masked by 1 - oob
        int i0[D], i1[D];
        float w0[D], w1[D], m[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            corner_1d(loc[d], a.S[d], i0[d], i1[d], w0[d], w1[d]);
            m[d] = (loc[d] >= 0.0f && loc[d] <= (float)(a.S[d] - 1)) ? 1.0f : 0.0f;   // clip passes the gradient on the closed range
        }
        Vec<V> g;
        g.load(go + (size_t)q * C + ch);
        Vec<V> v[1 << D];
#pragma unroll
        for (int corner = 0; corner < (1 << D); ++corner) {
            unsigned idx = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) idx = idx * (unsigned)a.S[d] + (unsigned)(((corner >> (D - 1 - d)) & 1) ? i1[d] : i0[d]);
            v[corner].load(vol + (size_t)idx * C + ch);
        }
        float gl[D];
#pragma unroll
        for (int d = 0; d < D; ++d) gl[d] = 0.0f;
#pragma unroll
        for (int corner = 0; corner < (1 << D); ++corner) {
            float dot = 0.0f;
#pragma unroll
            for (int k = 0; k < V; ++k) dot = __builtin_fmaf(g.v[k], v[corner].v[k], dot);
            // the weight product with one dimension's factor replaced by its derivative: d w0 = -m, d w1 = +m
#pragma unroll
            for (int d = 0; d < D; ++d) {
                float wexc = 1.0f;
#pragma unroll
                for (int e2 = 0; e2 < D; ++e2) {
                    const int bit = (corner >> (D - 1 - e2)) & 1;
                    wexc *= (e2 == d) ? (bit ? m[e2] : -m[e2]) : (bit ? w1[e2] : w0[e2]);
                }
                gl[d] = __builtin_fmaf(dot, wexc, gl[d]);
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int j = 0; j < D; ++j) acc[i * (D + 1) + j] = __builtin_fmaf(gl[i], p[j], acc[i * (D + 1) + j]);
            acc[i * (D + 1) + D] += gl[i];
        }
    }
    // wave, then block: fixed order
    __shared__ float s_part[4][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
// (a butterfly like nrt_wave_sum, but DESCENDING, 32 ... 1: another association, other bits; by hand, a helper changed the registers)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const float t = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
        a.rows[((size_t)b * gridDim.x + blockIdx.x) * K + threadIdx.x] = t;
    }
}

// grad_matrix[o][k] = the sum of rows [o * nrows, (o + 1) * nrows) in float64: sixteen interleaved runs in row order, then the runs in
// order.  nrows == 0 (nearest interpolation) stores zeros.
__global__ __launch_bounds__(256) void affine_warp_rows_sum(const float *__restrict__ rows, unsigned nrows, int K, float *__restrict__ gm) {
    __shared__ double s_run[16][16];
    const unsigned k = threadIdx.x & 15u, run = threadIdx.x >> 4;
    const float *r = rows + (size_t)blockIdx.x * nrows * K;
    double t = 0.0;
    if ((int)k < K)
        for (unsigned row = run; row < nrows; row += 16u) t += (double)r[(size_t)row * K + k];
    s_run[run][k] = t;
    __syncthreads();
    if ((int)threadIdx.x < K) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += s_run[i][threadIdx.x];
        gm[(size_t)blockIdx.x * K + threadIdx.x] = (float)sum;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// blocks per batch entry of the backward: about 2048 items per block, at most 4096 rows per launch (64 per entry for large batches)
unsigned bwd_blocks(unsigned long long nitems, int batch) {
    unsigned long long nb = (nitems + 2047) / 2048, cap = 4096ull / (unsigned)batch;
    if (cap < 64) cap = 64;
    if (nb > cap) nb = cap;
    return nb < 1 ? 1u : (unsigned)nb;
}

// everything but the pointers; NRT_OK or the refusal
int geometry(AffWarpArgs &a, int ndim, const int *vol_shape, const int *out_shape, int channels, int batch, int matrix_batch,
             int shift_center) {
    if (!vol_shape || !out_shape || channels < 1 || batch < 1) return NRT_ERR_INVALID_ARG;
    if (ndim != 2 && ndim != 3) return NRT_ERR_UNSUPPORTED;
    for (int d = 0; d < ndim; ++d)
        if (vol_shape[d] < 1 || out_shape[d] < 1) return NRT_ERR_INVALID_ARG;
    if (matrix_batch != 1 && matrix_batch != batch) return NRT_ERR_INVALID_ARG;
    if (batch > 65535) return NRT_ERR_UNSUPPORTED;
    const unsigned long long LIM = 1ull << 31;
    unsigned long long nin = (unsigned long long)batch * (unsigned)channels, no = nin, nvox_in = 1, nvox_out = 1;
    if (nin >= LIM) return NRT_ERR_UNSUPPORTED;
    for (int d = 0; d < NRT_MAXD; ++d) {
        a.S[d] = d < ndim ? vol_shape[d] : 1;
        a.O[d] = d < ndim ? out_shape[d] : 1;
        a.c[d] = (shift_center && d < ndim) ? (float)(a.O[d] - 1) / 2.0f : 0.0f;
        nin *= (unsigned)a.S[d]; no *= (unsigned)a.O[d];
        nvox_in *= (unsigned)a.S[d]; nvox_out *= (unsigned)a.O[d];
        if (nin >= LIM || no >= LIM) return NRT_ERR_UNSUPPORTED;              // (each factor < 2^31: no overflow before the test)
    }
    a.C = channels; a.CG = channels;
    a.nout = (unsigned)nvox_out;
    a.nitems = a.nout * (unsigned)channels;
    a.vol_bs = (long long)nvox_in * channels;
    a.out_bs = (long long)nvox_out * channels;
    a.m_bs = matrix_batch == 1 ? 0 : ndim * (ndim + 1);
    a.has_fill = 0; a.fill = 0.0f;
    a.vol = nullptr; a.matrix = nullptr; a.gout = nullptr; a.out = nullptr; a.rows = nullptr;
    return NRT_OK;
}

// channels per item: 4 where C % 4 == 0 and the pointers allow 16-byte accesses, the whole row of a voxel at 2 and 3 channels, else 1
int item_width(AffWarpArgs &a, const void *p0, const void *p1) {
    int V = 1;
    if ((a.C & 3) == 0 && ((((uintptr_t)p0 | (uintptr_t)p1) & 15) == 0)) V = 4;
    else if (a.C == 2 || a.C == 3) V = a.C;
    a.CG = a.C / V;
    a.nitems = a.nout * (unsigned)a.CG;
    return V;
}

template <int D, int V>
void launch_fwd_m(const AffWarpArgs &a, dim3 grid, int method, hipStream_t st) {
    if (method == NRT_INTERP_NEAREST) hipLaunchKernelGGL((affine_warp_fwd<D, NRT_INTERP_NEAREST, V>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((affine_warp_fwd<D, NRT_INTERP_LINEAR, V>), grid, dim3(256), 0, st, a);
}

template <int D>
void launch_fwd(const AffWarpArgs &a, int V, dim3 grid, int method, hipStream_t st) {
    switch (V) {
        case 4: launch_fwd_m<D, 4>(a, grid, method, st); break;
        case 3: launch_fwd_m<D, 3>(a, grid, method, st); break;
        case 2: launch_fwd_m<D, 2>(a, grid, method, st); break;
        default: launch_fwd_m<D, 1>(a, grid, method, st); break;
    }
}

template <int D>
void launch_bwd(const AffWarpArgs &a, int V, dim3 grid, hipStream_t st) {
    switch (V) {
        case 4: hipLaunchKernelGGL((affine_warp_bwd<D, 4>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((affine_warp_bwd<D, 3>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((affine_warp_bwd<D, 2>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((affine_warp_bwd<D, 1>), grid, dim3(256), 0, st, a); break;
    }
}

}  // namespace

extern "C" size_t nrt_affine_warp_workspace_bytes(int ndim, const int *out_shape, int channels, int batch) {
    AffWarpArgs a;
    if (geometry(a, ndim, out_shape, out_shape, channels, batch, 1, 0) != NRT_OK) return 0;
    // sized for the one-channel items: the wider arms have fewer of them and never more blocks
    return (size_t)batch * bwd_blocks(a.nitems, batch) * (size_t)(ndim * (ndim + 1)) * sizeof(float);
}

extern "C" int nrt_affine_warp_f32(const float *vol, const float *matrix, float *out, int ndim, const int *vol_shape, const int *out_shape,
                                   int channels, int batch, int matrix_batch, int shift_center, int method, int has_fill,
                                   float fill_value, void *stream) {
    if (!vol || !matrix || !out) return NRT_ERR_INVALID_ARG;
    AffWarpArgs a;
    const int rc = geometry(a, ndim, vol_shape, out_shape, channels, batch, matrix_batch, shift_center);
    if (rc != NRT_OK) return rc;
    if (method != NRT_INTERP_LINEAR && method != NRT_INTERP_NEAREST) return NRT_ERR_INVALID_ARG;
    a.vol = vol; a.matrix = matrix; a.out = out;
    a.has_fill = has_fill ? 1 : 0; a.fill = fill_value;
    const int V = item_width(a, vol, out);
    unsigned blocks = (a.nitems + 1023u) / 1024u;                                // four items per thread, the rest on the grid stride
    if (blocks > (1u << 20)) blocks = 1u << 20;
    const dim3 grid(blocks, (unsigned)batch);
    hipStream_t st = nrt_stream(stream);
    if (ndim == 2) launch_fwd<2>(a, V, grid, method, st);
    else launch_fwd<3>(a, V, grid, method, st);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_affine_warp_bwd_f32(const float *vol, const float *matrix, const float *grad_out, float *grad_matrix, int ndim,
                                       const int *vol_shape, const int *out_shape, int channels, int batch, int matrix_batch,
                                       int shift_center, int method, int has_fill, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    if (!vol || !matrix || !grad_out || !grad_matrix) return NRT_ERR_INVALID_ARG;
    AffWarpArgs a;
    const int rc = geometry(a, ndim, vol_shape, out_shape, channels, batch, matrix_batch, shift_center);
    if (rc != NRT_OK) return rc;
    if (method != NRT_INTERP_LINEAR && method != NRT_INTERP_NEAREST) return NRT_ERR_INVALID_ARG;
    const size_t need = nrt_affine_warp_workspace_bytes(ndim, out_shape, channels, batch);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3)) return NRT_ERR_WORKSPACE;
    a.vol = vol; a.matrix = matrix; a.gout = grad_out; a.rows = (float *)workspace;
    a.has_fill = has_fill ? 1 : 0;
    hipStream_t st = nrt_stream(stream);
    const int K = ndim * (ndim + 1);
    unsigned nrows = 0;                                                          // nearest: tf.round has no gradient
    if (method == NRT_INTERP_LINEAR) {
        const int V = item_width(a, vol, grad_out);
        const unsigned nb = bwd_blocks(a.nitems, batch);                         // <= the blocks the workspace was sized for
        const dim3 grid(nb, (unsigned)batch);
        if (ndim == 2) launch_bwd<2>(a, V, grid, st);
        else launch_bwd<3>(a, V, grid, st);
        NRT_CHECK_LAUNCH();
        nrows = matrix_batch == 1 ? nb * (unsigned)batch : nb;
    }
    hipLaunchKernelGGL(affine_warp_rows_sum, dim3((unsigned)matrix_batch), dim3(256), 0, st, (const float *)workspace, nrows, K, grad_matrix);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
