// Layers with one parameter (or one small matrix) per voxel, and the streaming-statistics layers (include/neurite_amd.h, "Local and
// stream layers"; neurite/tf/layers.py:746-808, 1535-1607, 1711-1844, 1915-2073).
//
// Everything here is memory bound.  The shapes of the kernels:
//   * a thread owns one 16-byte group of the CONTIGUOUS parameter axis (or one element where the rows are not 16-byte aligned: n or
//     cout not a multiple of 4, or an unaligned pointer) and runs the batch loop itself, so a parameter is read once for all batch
//     entries and its gradient is a sum over b = 0 .. B-1 in that order by one thread: no atomics, run-to-run bit-identical
//   * `count` (the stream layers) is read by the voxel kernels and written by a one-thread kernel that FOLLOWS them in stream order
//     (stream_finalize), so no block writes it while another still reads it and nothing travels to the host
//   * the library is built with -ffp-contract=off: every product and sum below is rounded on its own, in the reference's order
#include "nrt_common.h"

#include <initializer_list>

namespace {

constexpr int kThreads = 256;
constexpr int kBatchChunk = 8;             // batch entries whose accumulators a thread of the cross-linear kernels keeps in registers

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// blocks of kThreads for `units` work items; false where the count does not fit the grid
inline bool blocks_for(long long units, unsigned &blocks) {
    const long long b = (units + kThreads - 1) / kThreads;
    if (b > 0x7fffffffLL) return false;
    blocks = (unsigned)(b < 1 ? 1 : b);
    return true;
}

// Work item u of a row of n floats that is processed as nvec 16-byte groups followed by n - 4 * nvec single elements.
__device__ __forceinline__ bool unit_of(long long u, long long nvec, long long n, long long &i, bool &vec) {
    vec = u < nvec;
    i = vec ? 4 * u : 4 * nvec + (u - nvec);
    return i < n;
}

__device__ __forceinline__ nrt_f4 ld4(const float *p) { return *(const nrt_f4 *)p; }
__device__ __forceinline__ void st4(float *p, nrt_f4 v) { *(nrt_f4 *)p = v; }

// the factor of batch entry b of LocalParamWithInput (:1837-1838): x[b, 0] * 0 + 1 -- 1 for a finite element, NaN otherwise
__device__ __forceinline__ float probe_factor(const float *probe, long long stride, int b) {
    return probe ? nrt_add(nrt_mul(probe[(long long)b * stride], 0.0f), 1.0f) : 1.0f;
}

// ------------------------------------------------------------------------------------------------------------------------------
// affine family
// ------------------------------------------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void affine_item(const float *x, const float *probe, long long probe_stride, const float *mult,
                                            const float *bias, float bias_scale, float *y, int batch, long long n, long long i) {
    float bt[W], m[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        bt[k] = nrt_mul(bias[i + k], bias_scale);
        m[k] = mult ? mult[i + k] : 1.0f;
    }
    for (int b = 0; b < batch; ++b) {
        const long long o = (long long)b * n + i;
        float r[W];
        if (x) {
            float xv[W];
            if (W == 4) {
                const nrt_f4 v = ld4(x + o);
                xv[0] = v.x; xv[1 % W] = v.y; xv[2 % W] = v.z; xv[3 % W] = v.w;
            } else {
                xv[0] = x[o];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) r[k] = nrt_add(mult ? nrt_mul(xv[k], m[k]) : xv[k], bt[k]);
        } else {
            const float e = probe_factor(probe, probe_stride, b);
#pragma unroll
            for (int k = 0; k < W; ++k) r[k] = probe ? nrt_mul(e, bt[k]) : bt[k];
        }
        if (W == 4) st4(y + o, (nrt_f4){r[0], r[1 % W], r[2 % W], r[3 % W]});
        else y[o] = r[0];
    }
}

__global__ void __launch_bounds__(kThreads)
local_affine(const float *__restrict__ x, const float *__restrict__ probe, long long probe_stride, const float *__restrict__ mult,
             const float *__restrict__ bias, float bias_scale, float *__restrict__ y, int batch, long long n, long long nvec) {
    long long i;
    bool vec;
    if (!unit_of((long long)blockIdx.x * kThreads + threadIdx.x, nvec, n, i, vec)) return;
    if (vec) affine_item<4>(x, probe, probe_stride, mult, bias, bias_scale, y, batch, n, i);
    else affine_item<1>(x, probe, probe_stride, mult, bias, bias_scale, y, batch, n, i);
}

template <int W>
__device__ __forceinline__ void affine_bwd_item(const float *g, const float *x, const float *probe, long long probe_stride,
                                                const float *mult, float bias_scale, float *gx, float *gmult, float *gbias, int batch,
                                                long long n, long long i) {
    float m[W], sm[W], sb[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        m[k] = gx ? mult[i + k] : 0.0f;
        sm[k] = 0.0f;
        sb[k] = 0.0f;
    }
    for (int b = 0; b < batch; ++b) {
        const long long o = (long long)b * n + i;
        float gv[W], xv[W];
        if (W == 4) {
            const nrt_f4 v = ld4(g + o);
            gv[0] = v.x; gv[1 % W] = v.y; gv[2 % W] = v.z; gv[3 % W] = v.w;
            if (gmult) {
                const nrt_f4 t = ld4(x + o);
                xv[0] = t.x; xv[1 % W] = t.y; xv[2 % W] = t.z; xv[3 % W] = t.w;
            }
        } else {
            gv[0] = g[o];
            if (gmult) xv[0] = x[o];
        }
        const float e = probe_factor(probe, probe_stride, b);
        float r[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (gx) r[k] = nrt_mul(gv[k], m[k]);
            if (gmult) sm[k] = nrt_add(sm[k], nrt_mul(gv[k], xv[k]));
            if (gbias) sb[k] = nrt_add(sb[k], probe ? nrt_mul(e, gv[k]) : gv[k]);
        }
        if (gx) {
            if (W == 4) st4(gx + o, (nrt_f4){r[0], r[1 % W], r[2 % W], r[3 % W]});
            else gx[o] = r[0];
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (gmult) gmult[i + k] = sm[k];
        if (gbias) gbias[i + k] = nrt_mul(bias_scale, sb[k]);
    }
}

__global__ void __launch_bounds__(kThreads)
local_affine_bwd(const float *__restrict__ g, const float *__restrict__ x, const float *__restrict__ probe, long long probe_stride,
                 const float *__restrict__ mult, float bias_scale, float *__restrict__ gx, float *__restrict__ gmult,
                 float *__restrict__ gbias, int batch, long long n, long long nvec) {
    long long i;
    bool vec;
    if (!unit_of((long long)blockIdx.x * kThreads + threadIdx.x, nvec, n, i, vec)) return;
    if (vec) affine_bwd_item<4>(g, x, probe, probe_stride, mult, bias_scale, gx, gmult, gbias, batch, n, i);
    else affine_bwd_item<1>(g, x, probe, probe_stride, mult, bias_scale, gx, gmult, gbias, batch, n, i);
}

// rows of n floats, `batch` of them n apart: 16-byte groups where every row starts on a 16-byte boundary
inline long long row_vectors(long long n, int batch, std::initializer_list<const void *> ptrs) {
    if (n % 4 != 0 && batch > 1) return 0;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return 0;
    return n / 4;
}

// ------------------------------------------------------------------------------------------------------------------------------
// LocalCrossLinear: y[b, v, :] = x[b, v, :] @ W[v] (+ bias[v]).  A thread owns W floats of the output row of one voxel and walks the
// cin rows of W[v] once per chunk of kBatchChunk batch entries (once for B <= 8), a row of W[v] being read as one 16-byte group.
// ------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kThreads)
cross_linear(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ y, int batch,
             long long nvox, int cin, int cout) {
    const int groups = cout / W;
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= nvox * groups) return;
    const long long v = u / groups;
    const int o = (int)(u - v * groups) * W;
    const float *wv = w + (v * cin) * cout + o;
    for (int b0 = 0; b0 < batch; b0 += kBatchChunk) {
        const int nb = min(kBatchChunk, batch - b0);
        float acc[kBatchChunk][W];
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j)
#pragma unroll
            for (int k = 0; k < W; ++k) acc[j][k] = 0.0f;
        for (int c = 0; c < cin; ++c) {
            float wr[W];
            if (W == 4) {
                const nrt_f4 t = ld4(wv + (long long)c * cout);
                wr[0] = t.x; wr[1 % W] = t.y; wr[2 % W] = t.z; wr[3 % W] = t.w;
            } else {
                wr[0] = wv[(long long)c * cout];
            }
#pragma unroll
            for (int j = 0; j < kBatchChunk; ++j) {
                if (j < nb) {
                    const float xv = x[((long long)(b0 + j) * nvox + v) * cin + c];
#pragma unroll
                    for (int k = 0; k < W; ++k) acc[j][k] = nrt_add(acc[j][k], nrt_mul(xv, wr[k]));
                }
            }
        }
        float bv[W];
#pragma unroll
        for (int k = 0; k < W; ++k) bv[k] = bias ? bias[v * cout + o + k] : 0.0f;
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j) {
            if (j < nb) {
                float *yo = y + ((long long)(b0 + j) * nvox + v) * cout + o;
                float r[W];
#pragma unroll
                for (int k = 0; k < W; ++k) r[k] = bias ? nrt_add(acc[j][k], bv[k]) : acc[j][k];
                if (W == 4) st4(yo, (nrt_f4){r[0], r[1 % W], r[2 % W], r[3 % W]});
                else yo[0] = r[0];
            }
        }
    }
}

// gx[b, v, c] = sum_o g[b, v, o] * W[v, c, o]: a thread owns (v, c) and walks the row W[v, c, :] in 16-byte groups
template <int W>
__global__ void __launch_bounds__(kThreads)
cross_linear_gx(const float *__restrict__ g, const float *__restrict__ w, float *__restrict__ gx, int batch, long long nvox, int cin,
                int cout) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= nvox * cin) return;
    const long long v = u / cin;
    const float *wr = w + u * cout;                       // row (v, c)
    for (int b0 = 0; b0 < batch; b0 += kBatchChunk) {
        const int nb = min(kBatchChunk, batch - b0);
        float acc[kBatchChunk];
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j) acc[j] = 0.0f;
        for (int o = 0; o < cout; o += W) {
            float wk[W];
            if (W == 4) {
                const nrt_f4 t = ld4(wr + o);
                wk[0] = t.x; wk[1 % W] = t.y; wk[2 % W] = t.z; wk[3 % W] = t.w;
            } else {
                wk[0] = wr[o];
            }
#pragma unroll
            for (int j = 0; j < kBatchChunk; ++j) {
                if (j < nb) {
                    const float *gp = g + ((long long)(b0 + j) * nvox + v) * cout + o;
                    float gk[W];
                    if (W == 4) {
                        const nrt_f4 t = ld4(gp);
                        gk[0] = t.x; gk[1 % W] = t.y; gk[2 % W] = t.z; gk[3 % W] = t.w;
                    } else {
                        gk[0] = gp[0];
                    }
#pragma unroll
                    for (int k = 0; k < W; ++k) acc[j] = nrt_add(acc[j], nrt_mul(gk[k], wk[k]));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j)
            if (j < nb) gx[(long long)(b0 + j) * nvox * cin + u] = acc[j];
    }
}

// gW[v, c, o] = sum_b x[b, v, c] * g[b, v, o] (c < cin) and gbias[v, o] = sum_b g[b, v, o] (the extra row c == cin of the item space)
template <int W>
__global__ void __launch_bounds__(kThreads)
cross_linear_gw(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gw, float *__restrict__ gbias, int batch,
                long long nvox, int cin, int cout) {
    const int groups = cout / W;
    const int rows = cin + 1;
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= nvox * rows * groups) return;
    const long long vc = u / groups;
    const int o = (int)(u - vc * groups) * W;
    const long long v = vc / rows;
    const int c = (int)(vc - v * rows);
    const bool is_bias = c == cin;
    if (is_bias ? !gbias : !gw) return;
    float acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0f;
    for (int b = 0; b < batch; ++b) {
        const float *gp = g + ((long long)b * nvox + v) * cout + o;
        float gk[W];
        if (W == 4) {
            const nrt_f4 t = ld4(gp);
            gk[0] = t.x; gk[1 % W] = t.y; gk[2 % W] = t.z; gk[3 % W] = t.w;
        } else {
            gk[0] = gp[0];
        }
        if (is_bias) {
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] = nrt_add(acc[k], gk[k]);
        } else {
            const float xv = x[((long long)b * nvox + v) * cin + c];
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] = nrt_add(acc[k], nrt_mul(xv, gk[k]));
        }
    }
    float *out = is_bias ? gbias + v * cout + o : gw + (v * cin + c) * cout + o;
    if (W == 4) st4(out, (nrt_f4){acc[0], acc[1 % W], acc[2 % W], acc[3 % W]});
    else out[0] = acc[0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// stream layers.  The scalars every thread derives from the OLD count (neurite/tf/layers.py:2059-2073, 1962, 1972, 2043-2045):
// ------------------------------------------------------------------------------------------------------------------------------
struct StreamScalars {
    float new_count, alpha, scale;
};

__device__ __forceinline__ StreamScalars stream_scalars(float count, float cap, int batch, int training) {
    StreamScalars s;
    const float bs = (float)batch;
    if (training) {
        s.new_count = nrt_add(count, bs);
        s.alpha = bs / fminf(s.new_count, cap);
    } else {
        s.new_count = count;
        s.alpha = 0.0f;
    }
    s.scale = fminf(1.0f, s.new_count / cap);
    return s;
}

// new_mean = mean * (1 - alpha) + (sum_b x / B) * alpha
__device__ __forceinline__ float mean_step(float mean, float sum, float bs, float alpha) {
    return nrt_add(nrt_mul(mean, nrt_sub(1.0f, alpha)), nrt_mul(sum / bs, alpha));
}

template <int W>
__device__ __forceinline__ void stream_mean_item(const float *x, float *mean, const float *count, float cap, float *y, int batch,
                                                 long long n, int training, long long i) {
    const StreamScalars s = stream_scalars(count[0], cap, batch, training);
    float m[W];
#pragma unroll
    for (int k = 0; k < W; ++k) m[k] = mean[i + k];
    if (training) {
        float sum[W];
#pragma unroll
        for (int k = 0; k < W; ++k) sum[k] = 0.0f;
        for (int b = 0; b < batch; ++b) {
            const long long o = (long long)b * n + i;
            if (W == 4) {
                const nrt_f4 v = ld4(x + o);
                sum[0] = nrt_add(sum[0], v.x); sum[1 % W] = nrt_add(sum[1 % W], v.y);
                sum[2 % W] = nrt_add(sum[2 % W], v.z); sum[3 % W] = nrt_add(sum[3 % W], v.w);
            } else {
                sum[0] = nrt_add(sum[0], x[o]);
            }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            m[k] = mean_step(m[k], sum[k], (float)batch, s.alpha);
            mean[i + k] = m[k];
        }
    }
    if (!y) return;
    float r[W];
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = nrt_mul(s.scale, m[k]);
    for (int b = 0; b < batch; ++b) {
        const long long o = (long long)b * n + i;
        if (W == 4) st4(y + o, (nrt_f4){r[0], r[1 % W], r[2 % W], r[3 % W]});
        else y[o] = r[0];
    }
}

// y may be NULL (the mean update of CovStream).  `mean` is read and written by the thread that owns the element only.
__global__ void __launch_bounds__(kThreads)
stream_mean(const float *__restrict__ x, float *__restrict__ mean, const float *__restrict__ count, float cap, float *__restrict__ y,
            int batch, long long n, long long nvec, int training) {
    long long i;
    bool vec;
    if (!unit_of((long long)blockIdx.x * kThreads + threadIdx.x, nvec, n, i, vec)) return;
    if (vec) stream_mean_item<4>(x, mean, count, cap, y, batch, n, training, i);
    else stream_mean_item<1>(x, mean, count, cap, y, batch, n, training, i);
}

// the one writer of `count`, after the voxel kernels of the call in stream order; coef = scale * alpha / B for the backward
__global__ void stream_finalize(float *count, float cap, int batch, float *coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const StreamScalars s = stream_scalars(count[0], cap, batch, 1);
    if (coef) coef[0] = nrt_mul(s.scale, s.alpha) / (float)batch;
    count[0] = s.new_count;
}

template <int W>
__device__ __forceinline__ void stream_mean_bwd_item(const float *g, const float *coef, float *gx, int batch, long long n, long long i) {
    float sum[W];
#pragma unroll
    for (int k = 0; k < W; ++k) sum[k] = 0.0f;
    for (int b = 0; b < batch; ++b) {
        const long long o = (long long)b * n + i;
        if (W == 4) {
            const nrt_f4 v = ld4(g + o);
            sum[0] = nrt_add(sum[0], v.x); sum[1 % W] = nrt_add(sum[1 % W], v.y);
            sum[2 % W] = nrt_add(sum[2 % W], v.z); sum[3 % W] = nrt_add(sum[3 % W], v.w);
        } else {
            sum[0] = nrt_add(sum[0], g[o]);
        }
    }
    const float c = coef[0];
#pragma unroll
    for (int k = 0; k < W; ++k) sum[k] = nrt_mul(c, sum[k]);
    for (int b = 0; b < batch; ++b) {
        const long long o = (long long)b * n + i;
        if (W == 4) st4(gx + o, (nrt_f4){sum[0], sum[1 % W], sum[2 % W], sum[3 % W]});
        else gx[o] = sum[0];
    }
}

__global__ void __launch_bounds__(kThreads)
stream_mean_bwd(const float *__restrict__ g, const float *__restrict__ coef, float *__restrict__ gx, int batch, long long n,
                long long nvec) {
    long long i;
    bool vec;
    if (!unit_of((long long)blockIdx.x * kThreads + threadIdx.x, nvec, n, i, vec)) return;
    if (vec) stream_mean_bwd_item<4>(g, coef, gx, batch, n, i);
    else stream_mean_bwd_item<1>(g, coef, gx, batch, n, i);
}

// CovStream: a block owns a tile of kCovRows rows x 16 * W columns of the v x v matrix, a thread W contiguous columns of one row.
// The rows of X that the tile needs (X[b, r0 .. r0 + 15] and X[b, c0 .. c0 + 16 W - 1]) are staged in LDS kCovBatch batch entries
// at a time; cov is read once and written once, y[b] written once.
constexpr int kCovRows = 16, kCovBatch = 8;

template <int W>
__global__ void __launch_bounds__(kThreads)
stream_cov(const float *__restrict__ x, float *__restrict__ cov, const float *__restrict__ count, float cap, float *__restrict__ y,
           int batch, int v, int training) {
    constexpr int kCols = 16 * W;
    __shared__ float xr[kCovBatch][kCovRows];
    __shared__ __attribute__((aligned(16))) float xc[kCovBatch][kCols];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r0 = blockIdx.y * kCovRows, c0 = blockIdx.x * kCols;
    const int r = r0 + ty, c = c0 + tx * W;
    const bool live = r < v && c < v;                       // v is a multiple of W where W == 4: a live group is whole
    const float old_count = count[0];
    const StreamScalars s = stream_scalars(old_count, cap, batch, training);
    const long long at = (long long)r * v + c;
    float cv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) cv[k] = 0.0f;
    if (live) {
        if (W == 4) {
            const nrt_f4 t = ld4(cov + at);
            cv[0] = t.x; cv[1 % W] = t.y; cv[2 % W] = t.z; cv[3 % W] = t.w;
        } else {
            cv[0] = cov[at];
        }
    }
    if (training) {
        float sum[W];
#pragma unroll
        for (int k = 0; k < W; ++k) sum[k] = 0.0f;
        for (int b0 = 0; b0 < batch; b0 += kCovBatch) {
            const int nb = min(kCovBatch, batch - b0);
            __syncthreads();
            for (int t = threadIdx.x; t < nb * kCovRows; t += kThreads) {
                const int j = t / kCovRows, q = t - j * kCovRows;
                xr[j][q] = r0 + q < v ? x[(long long)(b0 + j) * v + r0 + q] : 0.0f;
            }
            for (int t = threadIdx.x; t < nb * kCols; t += kThreads) {
                const int j = t / kCols, q = t - j * kCols;
                xc[j][q] = c0 + q < v ? x[(long long)(b0 + j) * v + c0 + q] : 0.0f;
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) {
                const float a = xr[j][ty];
#pragma unroll
                for (int k = 0; k < W; ++k) sum[k] = nrt_add(sum[k], nrt_mul(a, xc[j][tx * W + k]));
            }
        }
        const float prev_cap = fminf(old_count, cap);
        const float keep = nrt_sub(prev_cap, 1.0f);
        const float denom = nrt_sub(nrt_add(prev_cap, (float)batch), 1.0f);
#pragma unroll
        for (int k = 0; k < W; ++k) cv[k] = nrt_add(nrt_mul(cv[k], keep), sum[k]) / denom;       // IEEE: 0 denominators included
        if (live) {
            if (W == 4) st4(cov + at, (nrt_f4){cv[0], cv[1 % W], cv[2 % W], cv[3 % W]});
            else cov[at] = cv[0];
        }
    }
    if (!live) return;
    float o[W];
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = nrt_mul(s.scale, cv[k]);
    const long long vv = (long long)v * v;
    for (int b = 0; b < batch; ++b) {
        if (W == 4) st4(y + b * vv + at, (nrt_f4){o[0], o[1 % W], o[2 % W], o[3 % W]});
        else y[b * vv + at] = o[0];
    }
}

template <typename... Args>
inline void launch_w(bool wide, void (*k4)(Args...), void (*k1)(Args...), dim3 grid, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(wide ? k4 : k1, grid, dim3(kThreads), 0, st, args...);
}

}  // namespace

extern "C" int nrt_local_affine_f32(const float *x, const float *probe, long long probe_stride, const float *mult, const float *bias,
                                    float bias_scale, float *y, int batch, long long n, void *stream) {
    if (!bias || !y || batch < 1 || n < 1) return NRT_ERR_INVALID_ARG;
    if (x && probe) return NRT_ERR_INVALID_ARG;
    if (!x && mult) return NRT_ERR_INVALID_ARG;
    if (n > (1LL << 62) / batch) return NRT_ERR_UNSUPPORTED;
    const long long nvec = row_vectors(n, batch, {x, mult, bias, y});
    unsigned blocks;
    if (!blocks_for(nvec + (n - 4 * nvec), blocks)) return NRT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(local_affine, dim3(blocks), dim3(kThreads), 0, nrt_stream(stream), x, probe, probe_stride, mult, bias, bias_scale,
                       y, batch, n, nvec);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_local_affine_bwd_f32(const float *g, const float *x, const float *probe, long long probe_stride, const float *mult,
                                        float bias_scale, float *gx, float *gmult, float *gbias, int batch, long long n, void *stream) {
    if (!g || batch < 1 || n < 1) return NRT_ERR_INVALID_ARG;
    if ((gx && !mult) || (gmult && !x)) return NRT_ERR_INVALID_ARG;
    if (!gx && !gmult && !gbias) return NRT_OK;
    if (n > (1LL << 62) / batch) return NRT_ERR_UNSUPPORTED;
    const long long nvec = row_vectors(n, batch, {g, gmult ? x : nullptr, gx ? mult : nullptr, gx, gmult, gbias});
    unsigned blocks;
    if (!blocks_for(nvec + (n - 4 * nvec), blocks)) return NRT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(local_affine_bwd, dim3(blocks), dim3(kThreads), 0, nrt_stream(stream), g, x, probe, probe_stride, mult, bias_scale,
                       gx, gmult, gbias, batch, n, nvec);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

static int cross_linear_limits(int batch, long long nvox, int cin, int cout) {
    if (batch < 1 || nvox < 1) return NRT_ERR_INVALID_ARG;
    if (cin < 1 || cin > 64 || cout < 1 || cout > 64) return NRT_ERR_UNSUPPORTED;
    if (nvox > (1LL << 62) / ((long long)batch * 65 * 64)) return NRT_ERR_UNSUPPORTED;
    return NRT_OK;
}

extern "C" int nrt_local_cross_linear_f32(const float *x, const float *w, const float *bias, float *y, int batch, long long nvox,
                                          int cin, int cout, void *stream) {
    if (!x || !w || !y) return NRT_ERR_INVALID_ARG;
    const int rc = cross_linear_limits(batch, nvox, cin, cout);
    if (rc != NRT_OK) return rc;
    const bool wide = cout % 4 == 0 && aligned16(w) && aligned16(y) && (!bias || aligned16(bias));
    unsigned blocks;
    if (!blocks_for(nvox * (wide ? cout / 4 : cout), blocks)) return NRT_ERR_UNSUPPORTED;
    launch_w(wide, cross_linear<4>, cross_linear<1>, dim3(blocks), nrt_stream(stream), x, w, bias, y, batch, nvox, cin, cout);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_local_cross_linear_bwd_f32(const float *g, const float *x, const float *w, float *gx, float *gw, float *gbias,
                                              int batch, long long nvox, int cin, int cout, void *stream) {
    if (!g || (gx && !w) || (gw && !x)) return NRT_ERR_INVALID_ARG;
    const int rc = cross_linear_limits(batch, nvox, cin, cout);
    if (rc != NRT_OK) return rc;
    hipStream_t st = nrt_stream(stream);
    unsigned blocks;
    if (gx) {
        const bool wide = cout % 4 == 0 && aligned16(w) && aligned16(g);
        if (!blocks_for(nvox * cin, blocks)) return NRT_ERR_UNSUPPORTED;
        launch_w(wide, cross_linear_gx<4>, cross_linear_gx<1>, dim3(blocks), st, g, w, gx, batch, nvox, cin, cout);
        NRT_CHECK_LAUNCH();
    }
    if (gw || gbias) {
        const bool wide = cout % 4 == 0 && aligned16(g) && (!gw || aligned16(gw)) && (!gbias || aligned16(gbias));
        if (!blocks_for(nvox * (cin + 1) * (wide ? cout / 4 : cout), blocks)) return NRT_ERR_UNSUPPORTED;
        launch_w(wide, cross_linear_gw<4>, cross_linear_gw<1>, dim3(blocks), st, x, g, gw, gbias, batch, nvox, cin, cout);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}

extern "C" int nrt_stream_mean_f32(const float *x, float *mean, float *count, float cap, float *y, float *coef, int batch, long long n,
                                   int training, void *stream) {
    if (!mean || !count || !y || batch < 1 || n < 1 || (training && !x)) return NRT_ERR_INVALID_ARG;
    if (n > (1LL << 62) / batch) return NRT_ERR_UNSUPPORTED;
    const long long nvec = row_vectors(n, batch, {training ? x : nullptr, mean, y});
    unsigned blocks;
    if (!blocks_for(nvec + (n - 4 * nvec), blocks)) return NRT_ERR_UNSUPPORTED;
    hipStream_t st = nrt_stream(stream);
    hipLaunchKernelGGL(stream_mean, dim3(blocks), dim3(kThreads), 0, st, x, mean, (const float *)count, cap, y, batch, n, nvec,
                       training ? 1 : 0);
    NRT_CHECK_LAUNCH();
    if (training) {
        hipLaunchKernelGGL(stream_finalize, dim3(1), dim3(64), 0, st, count, cap, batch, coef);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}

extern "C" int nrt_stream_mean_bwd_f32(const float *g, const float *coef, float *gx, int batch, long long n, void *stream) {
    if (!g || !coef || !gx || batch < 1 || n < 1) return NRT_ERR_INVALID_ARG;
    if (n > (1LL << 62) / batch) return NRT_ERR_UNSUPPORTED;
    const long long nvec = row_vectors(n, batch, {g, gx});
    unsigned blocks;
    if (!blocks_for(nvec + (n - 4 * nvec), blocks)) return NRT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stream_mean_bwd, dim3(blocks), dim3(kThreads), 0, nrt_stream(stream), g, coef, gx, batch, n, nvec);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_stream_cov_f32(const float *x, float *mean, float *cov, float *count, float cap, float *y, int batch, int v,
                                  int training, void *stream) {
    if (!cov || !count || !y || batch < 1 || v < 1 || (training && (!x || !mean))) return NRT_ERR_INVALID_ARG;
    if ((long long)v * v > (1LL << 62) / batch) return NRT_ERR_UNSUPPORTED;
    const bool wide = v % 4 == 0 && aligned16(cov) && aligned16(y);
    const int cols = wide ? 64 : 16;
    const long long gy = ((long long)v + kCovRows - 1) / kCovRows;
    if (gy > 65535) return NRT_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((v + cols - 1) / cols), (unsigned)gy);
    hipStream_t st = nrt_stream(stream);
    launch_w(wide, stream_cov<4>, stream_cov<1>, grid, st, x, cov, (const float *)count, cap, y, batch, v, training ? 1 : 0);
    NRT_CHECK_LAUNCH();
    if (training) {
        const long long nvec = row_vectors(v, batch, {x, mean});
        unsigned blocks;
        if (!blocks_for(nvec + (v - 4 * nvec), blocks)) return NRT_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(stream_mean, dim3(blocks), dim3(kThreads), 0, st, x, mean, (const float *)count, cap, (float *)nullptr, batch,
                           (long long)v, nvec, 1);
        NRT_CHECK_LAUNCH();
        hipLaunchKernelGGL(stream_finalize, dim3(1), dim3(64), 0, st, count, cap, batch, (float *)nullptr);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}
