// Global max over the spatial axes, per batch entry and channel, with tf.reduce_max's gradient; and the MaxNorm weight constraint.
//
//   x [B, V, C] float32, channels-last  ->  y [B, C] = max_v x[b, v, c],  count [B, C] = how many v attain it (int32)
//
// Keras GlobalMaxPooling{1,2,3}D is this with V = the product of the spatial sizes; design_dnn's flatten-then-max lambda
// (neurite/tf/models.py:1640-1642) is C = 1 with V = V * C.  One pass over x, HBM bound: 4 bytes per compare.
//
//   stage 1   grid (blocks, B, channel tiles).  A block owns a contiguous range of rows of one batch entry.  Its 256 threads are
//             cw channel lanes x R row lanes (cw = min(channel units, 256), R = 256 / cw), so that a wave's loads are one contiguous run
//             of a row-major [rows, C] slab; a thread keeps (max, count) of its channel unit over the rows r, r + R, ..., four loads in
//             flight.  The row lanes are merged through LDS and the block leaves one (max, count) per channel in the workspace.
//             quad arm (16-byte lane groups): a channel unit is 4 adjacent channels; taken where C % 4 == 0 and x is 16-byte aligned.
//             folded quad arm: C = 1 or 2 with V * C % 4 == 0 and x aligned runs as [V * C / 4, 4]: pseudo-channel j is channel j % C.
//             element arm: everything else.  Which arm runs is a dispatch decision; each is correct at every shape it is given.
//   stage 2   one block per (batch entry, channel tile) merges the blocks' (and the folded pseudo-channels') pairs the same way.
//
// The merge of two pairs -- the larger max wins, equal maxima add their counts, a NaN on either side gives (NaN, 0) -- is exact,
// commutative and associative, so the result does not depend on the partition or the order: run-to-run bit-identical with no atomics,
// no host synchronisation (both directions capture into a graph).  The accumulator starts at (-inf, 0).  -0.0 == +0.0 as in IEEE
// (and in tf.equal): they tie, and which zero y carries follows the fixed merge order.
//
//   backward  gx[b, v, c] = x == y ? (1.0f / count) * g : 0   (TensorFlow's _MinOrMaxGrad: divide(indicators, num_selected) * grad, the
//             reciprocal rounded first); a slice whose max is NaN gets NaN throughout (TensorFlow's 0 / 0).  A one-block-per-entry
//             kernel leaves coef[b, c] = (1.0f / count) * g in the workspace, then one streaming read of x and write of gx.
#include "nrt_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr long long kBlockElems = 16384;       // elements of x a stage-1 block covers at least (64 per thread)
constexpr long long kMaxBlocks = 2048;         // stage-1 blocks over the whole batch (8 per CU)

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// blocks per batch entry: the launcher's grid rule (nrt_global_max_workspace_bytes reports it through the size)
inline long long gm_blocks(int batch, long long v, int channels) {
    long long nb = (v * channels + kBlockElems - 1) / kBlockElems;
    const long long cap = kMaxBlocks / batch > 1 ? kMaxBlocks / batch : 1;
    if (nb > cap) nb = cap;
    if (nb > v) nb = v;                          // (a block owns whole rows)
    return nb < 1 ? 1 : nb;
}
inline int gm_padded_channels(int channels) { return channels < 4 ? 4 : channels; }

__device__ __forceinline__ void gm_take(float &m, int &c, float v) {
    const bool gt = v > m, nn = v != v;
    c = gt ? 1 : c + (v == m ? 1 : 0);
    m = (gt || nn) ? v : m;
    c = nn ? 0 : c;
}
__device__ __forceinline__ void gm_merge(float &m, int &c, float m2, int c2) {
    const bool gt = m2 > m, nn = m2 != m2;
    c = gt ? c2 : c + (m2 == m ? c2 : 0);
    m = (gt || nn) ? m2 : m;
    c = nn ? 0 : c;
}

// merge the R row lanes of every channel lane: lane (r, cu) = thread r * cw + cu; the result is left in row lane 0
template <int W>
__device__ __forceinline__ void gm_block_merge(float (&m)[W], int (&c)[W], int r, int cu, int cw, int R, float *sm, int *sc) {
    const int t = r * cw + cu;
    const bool lane = r < R;
    if (lane) {
#pragma unroll
        for (int k = 0; k < W; ++k) { sm[t * W + k] = m[k]; sc[t * W + k] = c[k]; }
    }
    for (int n = R; n > 1;) {
        const int half = (n + 1) >> 1;
        __syncthreads();
        if (lane && r + half < n) {
            const int o = (r + half) * cw + cu;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                gm_merge(m[k], c[k], sm[o * W + k], sc[o * W + k]);
                sm[t * W + k] = m[k]; sc[t * W + k] = c[k];
            }
        }
        n = half;
    }
}

template <int W>
__device__ __forceinline__ void gm_load(const float *p, float (&v)[W]) {
    if (W == 4) {
        const nrt_f4 t = *(const nrt_f4 *)p;
        v[0] = t.x; v[1 % W] = t.y; v[2 % W] = t.z; v[3 % W] = t.w;
    } else {
        v[0] = p[0];
    }
}

// stage 1.  x: this call's [B, rows, units * W]; pm / pc: [B, gridDim.x, units * W]
template <int W>
__global__ void __launch_bounds__(kThreads)
global_max_stage1(const float *__restrict__ x, long long rows, int units, float *__restrict__ pm, int *__restrict__ pc) {
    __shared__ float sm[kThreads * W];
    __shared__ int sc[kThreads * W];
    const int b = blockIdx.y;
    const int cw = units < kThreads ? units : kThreads, R = kThreads / cw;
    const int r = threadIdx.x / cw, cu = threadIdx.x - r * cw;
    const long long unit = (long long)blockIdx.z * kThreads + cu;
    const bool live = r < R && unit < units;
    const long long per = (rows + gridDim.x - 1) / gridDim.x;
    const long long r0 = (long long)blockIdx.x * per < rows ? (long long)blockIdx.x * per : rows;
    const long long r1 = r0 + per < rows ? r0 + per : rows;
    const long long rs = (long long)units * W;                              // floats per row

    float m[W];
    int c[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { m[k] = -INFINITY; c[k] = 0; }
    if (live) {
        const float *p = x + (long long)b * rows * rs + unit * W;
        long long row = r0 + r;
        for (; row + 3ll * R < r1; row += 4ll * R) {                         // four rows in flight per lane
            float v0[W], v1[W], v2[W], v3[W];
            gm_load<W>(p + row * rs, v0);
            gm_load<W>(p + (row + R) * rs, v1);
            gm_load<W>(p + (row + 2ll * R) * rs, v2);
            gm_load<W>(p + (row + 3ll * R) * rs, v3);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                gm_take(m[k], c[k], v0[k]);
                gm_take(m[k], c[k], v1[k]);
                gm_take(m[k], c[k], v2[k]);
                gm_take(m[k], c[k], v3[k]);
            }
        }
        for (; row < r1; row += R) {
            float v0[W];
            gm_load<W>(p + row * rs, v0);
#pragma unroll
            for (int k = 0; k < W; ++k) gm_take(m[k], c[k], v0[k]);
        }
    }
    gm_block_merge<W>(m, c, r, cu, cw, R, sm, sc);
    if (live && r == 0) {
        const long long o = ((long long)b * gridDim.x + blockIdx.x) * rs + unit * W;
#pragma unroll
        for (int k = 0; k < W; ++k) { pm[o + k] = m[k]; pc[o + k] = c[k]; }
    }
}

// stage 2.  pm / pc: [B, rows, C] pairs (rows = stage-1 blocks x folded pseudo-channel groups)  ->  y, count [B, C]
__global__ void __launch_bounds__(kThreads)
global_max_stage2(const float *__restrict__ pm, const int *__restrict__ pc, int rows, int C, float *__restrict__ y,
                  int *__restrict__ count) {
    __shared__ float sm[kThreads];
    __shared__ int sc[kThreads];
    const int b = blockIdx.y;
    const int cw = C < kThreads ? C : kThreads, R = kThreads / cw;
    const int r = threadIdx.x / cw, cu = threadIdx.x - r * cw;
    const long long ch = (long long)blockIdx.z * kThreads + cu;
    const bool live = r < R && ch < C;
    float m[1] = {-INFINITY};
    int c[1] = {0};
    if (live) {
        const long long o = (long long)b * rows * C + ch;
        for (int row = r; row < rows; row += R) gm_merge(m[0], c[0], pm[o + (long long)row * C], pc[o + (long long)row * C]);
    }
    gm_block_merge<1>(m, c, r, cu, cw, R, sm, sc);
    if (live && r == 0) { y[(long long)b * C + ch] = m[0]; count[(long long)b * C + ch] = c[0]; }
}

// coef[b, c] = (1.0f / count) * g: the reciprocal is rounded before the product, as divide(indicators, num_selected) * grad does
__global__ void __launch_bounds__(kThreads)
global_max_coef(const int *__restrict__ count, const float *__restrict__ g, long long n, float *__restrict__ coef) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        coef[i] = nrt_mul(1.0f / (float)count[i], g[i]);
}

// x == y ? coef : 0; a NaN max compares unequal to everything and is handed on as the value (0 / 0 in TensorFlow)
__device__ __forceinline__ float gm_grad(float xv, float yv, float cf) { return xv == yv ? cf : (yv != yv ? yv : 0.0f); }

// backward.  MODE 0: per element, channel e % C.  MODE 1: quads, C % 4 == 0.  MODE 2: quads of the flat entry, C = 1 or 2 (channel
// j % C of quad element j).  n = elements (MODE 0) or quads per batch entry; each block streams one contiguous range.
template <int MODE>
__global__ void __launch_bounds__(kThreads)
global_max_bwd(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ coef, float *__restrict__ gx,
               long long n, int C) {
    const int b = blockIdx.y;
    const float *yb = y + (long long)b * C, *cb = coef + (long long)b * C;
    long long beg, end;
    nrt_block_range(n, kThreads, beg, end);
    if (MODE == 0) {
        const float *xb = x + (long long)b * n;
        float *gb = gx + (long long)b * n;
        long long e = beg + threadIdx.x;
        int c = (int)(e % C);
        const int cstep = kThreads % C;
        for (; e < end; e += kThreads) {
            gb[e] = gm_grad(xb[e], yb[c], cb[c]);
            c += cstep;
            if (c >= C) c -= C;
        }
    } else {
        const nrt_f4 *xb = (const nrt_f4 *)x + (long long)b * n;
        nrt_f4 *gb = (nrt_f4 *)gx + (long long)b * n;
        const int C4 = MODE == 1 ? C / 4 : 1;
        long long e = beg + threadIdx.x;
        int c = MODE == 1 ? (int)(e % C4) : 0;
        const int cstep = MODE == 1 ? kThreads % C4 : 0;
        nrt_f4 yv, cf;
        if (MODE == 2) {
            yv = (nrt_f4){yb[0], yb[C - 1], yb[0], yb[C - 1]};
            cf = (nrt_f4){cb[0], cb[C - 1], cb[0], cb[C - 1]};
        }
        for (; e < end; e += kThreads) {
            if (MODE == 1) {
                yv = (nrt_f4){yb[4 * c], yb[4 * c + 1], yb[4 * c + 2], yb[4 * c + 3]};       // (y and the workspace may be 4-byte aligned only)
                cf = (nrt_f4){cb[4 * c], cb[4 * c + 1], cb[4 * c + 2], cb[4 * c + 3]};
            }
            const nrt_f4 xv = xb[e];
            nrt_f4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = gm_grad(xv[k], yv[k], cf[k]);
            __builtin_nontemporal_store(o, gb + e);
            if (MODE == 1) {
                c += cstep;
                if (c >= C4) c -= C4;
            }
        }
    }
}

// Keras MaxNorm(max_value, axis=0) in place on w [k0, rest]: a thread owns a column
__global__ void __launch_bounds__(kThreads)
maxnorm_cols(float *__restrict__ w, int k0, long long rest, float max_value, float eps) {
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < rest; j += (long long)gridDim.x * kThreads) {
        // norm and factor in double (a few values per column; exact products, no cancellation), rounded once: the factor of a column is
        // then within half a unit of the last place of the real-number formula, and so a second application moves nothing by more
        double s = 0.0;
        for (int i = 0; i < k0; ++i) {
            const double v = (double)w[(long long)i * rest + j];
            s += v * v;
        }
        const double n = sqrt(s);
        const float scale = (float)(fmin(fmax(n, 0.0), (double)max_value) / ((double)eps + n));
        for (int i = 0; i < k0; ++i) w[(long long)i * rest + j] *= scale;
    }
}

int gm_check(int batch, long long v, int channels) {
    if (batch < 1 || v < 1 || channels < 1) return NRT_ERR_INVALID_ARG;
    if (batch > 65535) return NRT_ERR_UNSUPPORTED;
    if (v >= (1ll << 31) || v * channels >= (1ll << 31) || (long long)batch * v * channels >= (1ll << 31)) return NRT_ERR_UNSUPPORTED;
    return NRT_OK;
}

}  // namespace

extern "C" size_t nrt_global_max_workspace_bytes(int batch, long long v, int channels) {
    if (gm_check(batch, v, channels) != NRT_OK) return 0;
    return (size_t)batch * (size_t)gm_blocks(batch, v, channels) * (size_t)gm_padded_channels(channels) * (sizeof(float) + sizeof(int));
}

extern "C" int nrt_global_max_f32(const float *x, int batch, long long v, int channels, float *y, int *count, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!x || !y || !count) return NRT_ERR_INVALID_ARG;
    const int rc = gm_check(batch, v, channels);
    if (rc != NRT_OK) return rc;
    if (!workspace || workspace_bytes < nrt_global_max_workspace_bytes(batch, v, channels)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    const long long nb = gm_blocks(batch, v, channels);
    float *pm = (float *)workspace;
    int *pc = (int *)workspace + (size_t)batch * nb * gm_padded_channels(channels);
    const bool al = aligned16(x);
    int rows2;                                                               // rows of C pairs per batch entry that stage 2 merges
    if (al && channels % 4 == 0) {
        const int units = channels / 4;
        hipLaunchKernelGGL((global_max_stage1<4>), dim3((unsigned)nb, batch, (units + kThreads - 1) / kThreads), dim3(kThreads), 0, st, x,
                           v, units, pm, pc);
        rows2 = (int)nb;
    } else if (al && channels <= 2 && (v * channels) % 4 == 0) {
        const long long rows = v * channels / 4;
        const long long nbf = nb < rows ? nb : rows;
        hipLaunchKernelGGL((global_max_stage1<4>), dim3((unsigned)nbf, batch, 1), dim3(kThreads), 0, st, x, rows, 1, pm, pc);
        rows2 = (int)nbf * (4 / channels);
    } else {
        hipLaunchKernelGGL((global_max_stage1<1>), dim3((unsigned)nb, batch, (channels + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                           x, v, channels, pm, pc);
        rows2 = (int)nb;
    }
    hipLaunchKernelGGL(global_max_stage2, dim3(1, batch, (channels + kThreads - 1) / kThreads), dim3(kThreads), 0, st, pm, pc, rows2,
                       channels, y, count);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_global_max_bwd_f32(const float *x, const float *y, const int *count, const float *g, int batch, long long v,
                                      int channels, float *gx, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !y || !count || !g || !gx) return NRT_ERR_INVALID_ARG;
    const int rc = gm_check(batch, v, channels);
    if (rc != NRT_OK) return rc;
    if (!workspace || workspace_bytes < nrt_global_max_workspace_bytes(batch, v, channels)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    float *coef = (float *)workspace;                                        // [B, C]: fits, the forward's pairs take at least 8 B C bytes
    const long long nbc = (long long)batch * channels;
    hipLaunchKernelGGL(global_max_coef, dim3((unsigned)((nbc + kThreads - 1) / kThreads < 256 ? (nbc + kThreads - 1) / kThreads : 256)),
                       dim3(kThreads), 0, st, count, g, nbc, coef);
    const long long n = v * channels;
    const bool al = aligned16(x) && aligned16(gx) && n % 4 == 0;              // (n % 4: every batch entry starts aligned)
    const int mode = al && channels % 4 == 0 ? 1 : (al && channels <= 2 ? 2 : 0);
    const long long items = mode ? n / 4 : n;
    long long nb = (items + kThreads * 16 - 1) / (kThreads * 16);
    const long long cap = kMaxBlocks / batch > 1 ? kMaxBlocks / batch : 1;
    if (nb > cap) nb = cap;
    const dim3 grid((unsigned)nb, batch);
    if (mode == 1) hipLaunchKernelGGL((global_max_bwd<1>), grid, dim3(kThreads), 0, st, x, y, coef, gx, items, channels);
    else if (mode == 2) hipLaunchKernelGGL((global_max_bwd<2>), grid, dim3(kThreads), 0, st, x, y, coef, gx, items, channels);
    else hipLaunchKernelGGL((global_max_bwd<0>), grid, dim3(kThreads), 0, st, x, y, coef, gx, items, channels);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_maxnorm_f32(float *w, int k0, long long rest, float max_value, float eps, void *stream) {
    if (!w || k0 < 1 || rest < 1 || !(max_value > 0.0f) || !(eps >= 0.0f)) return NRT_ERR_INVALID_ARG;
    if ((long long)k0 * rest >= (1ll << 31)) return NRT_ERR_UNSUPPORTED;
    const long long nb = (rest + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(maxnorm_cols, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(kThreads), 0, nrt_stream(stream), w, k0, rest,
                       max_value, eps);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
