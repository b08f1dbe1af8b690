// Dense (fully connected) layer on a SHARED weight matrix: the bottleneck of models.ae / models.single_ae (neurite/tf/models.py:499, 558,
// 618).  float32; W is [in, out] row-major, the Keras `Dense` kernel layout, read as it is stored (no transpose, no pack step).
//
// At the batch sizes these models train at (1 .. 16) every product below is a stream of W through HBM: two flops per four bytes per
// batch entry.  So W is read ONCE per call for up to kMaxChunk = 16 batch entries (a larger batch runs in chunks of 16, W once per chunk),
// each lane keeps the accumulators of all of them, and nothing is staged that is used once.
//
//   forward   y[b, o] = act(sum_i x[b, i] w[i, o] + bias[o])
//     reduce arm (in >> out)   a block owns a slab of `in` and a tile of columns; lanes run along `out` (16-byte loads where rows are
//                              16-byte aligned), the rows of the slab are dealt to the block's row lanes, the slab's x sits in LDS as
//                              [row][batch] (one broadcast read per row).  The row lanes are summed through LDS in lane order, the slab's
//                              partial [batch, out] goes to the workspace, and dense_sum_partials adds the slabs in slab order.
//     expand arm (out >> in)   a thread owns W adjacent columns and walks all of `in`; no second stage.
//   backward  gx[b, i] = sum_o g[b, o] w[i, o]      a wave owns a segment of 64 * W columns of a row, with its g values in registers, and
//                              walks the block's rows; the NB sums of a row are reduced over the wave by a halving butterfly (17
//                              shuffles for 16 values).  The block's 4 waves take 4 adjacent segments and are added through LDS in wave
//                              order; a row wider than 4 segments leaves one partial per block in the workspace (dense_sum_partials).
//             gw[i, o] = sum_b x[b, i] g[b, o]      one streaming write of W's size: a thread owns W columns of 16 rows
//             gbias[o] = sum_b g[b, o]              one thread per column, b ascending
//
// Every sum has a fixed order that depends on the shapes only: no atomics, run-to-run bit-identical.  Products are accumulated with
// fmaf (one rounding per term).  Unaligned base pointers and out % 4 != 0 select the 4-byte forms; that is a dispatch decision.
#include "activations.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunk = 16;          // batch entries per pass over W
constexpr int kTileRows = 128;         // rows of x staged in LDS at a time (forward)
constexpr int kBlockRows = 64;         // rows of W a block of the row-dot kernel walks
constexpr int kGwRows = 16;            // rows of gw a thread owns
constexpr int kMaxSlabs = 1024;        // slabs of `in` of the reduce arm (grid.y)
constexpr int kTargetBlocks = 1024;    // the reduce arm cuts `in` until about this many blocks exist (4 per CU)

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

template <int W>
__device__ __forceinline__ void ldw(const float *p, float (&v)[W]) {
    if (W == 4) {
        const nrt_f4 t = *(const nrt_f4 *)p;
        v[0] = t.x; v[1 % W] = t.y; v[2 % W] = t.z; v[3 % W] = t.w;
    } else {
        v[0] = p[0];
    }
}
template <int W>
__device__ __forceinline__ void stw(float *p, const float (&v)[W]) {
    if (W == 4) *(nrt_f4 *)p = (nrt_f4){v[0], v[1 % W], v[2 % W], v[3 % W]};
    else p[0] = v[0];
}

template <int NB, int W>
__device__ __forceinline__ void fma_row(float (&acc)[NB][W], const float *xs, const float (&wv)[W]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float xv = xs[b];
#pragma unroll
        for (int k = 0; k < W; ++k) acc[b][k] = fmaf(xv, wv[k], acc[b][k]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// forward.  SPLIT (reduce arm): grid (column tiles, slabs); the block is lanes_x column lanes x (kThreads / lanes_x) row lanes and
// writes dst = partials [slab][nb][out].  !SPLIT (expand arm): grid (column tiles); dst = y with bias and activation applied.
// ------------------------------------------------------------------------------------------------------------------------------
template <int NB, int W, bool SPLIT>
__global__ void __launch_bounds__(kThreads)
dense_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ dst, int nb,
          int in, int out, int act, int slab_rows, int lanes_x) {
    __shared__ float xs[kTileRows * NB];
    __shared__ float red[SPLIT ? kThreads * W : 1];
    const int tid = threadIdx.x;
    const int tx = SPLIT ? (tid & (lanes_x - 1)) : tid;
    const int ty = SPLIT ? tid / lanes_x : 0;
    const int nty = SPLIT ? kThreads / lanes_x : 1;
    const long long col = ((long long)blockIdx.x * (SPLIT ? lanes_x : kThreads) + tx) * W;
    const bool live = col < out;                          // (W == 4 only where out % 4 == 0: a live group is whole)
    const int r_beg = SPLIT ? blockIdx.y * slab_rows : 0;
    const int r_end = SPLIT ? min(in, r_beg + slab_rows) : in;

    float acc[NB][W];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[b][k] = 0.0f;

    for (int t0 = r_beg; t0 < r_end; t0 += kTileRows) {
        const int rows = min(kTileRows, r_end - t0);
        __syncthreads();                                  // the previous tile has been read
        for (int e = tid; e < kTileRows * NB; e += kThreads) {
            const int b = e / kTileRows, r = e - b * kTileRows;           // consecutive threads: consecutive rows of one batch entry
            xs[r * NB + b] = (b < nb && r < rows) ? x[(long long)b * in + t0 + r] : 0.0f;
        }
        __syncthreads();
        if (live) {
            const float *wp = w + (long long)t0 * out + col;
            int r = ty;
            for (; r + 3 * nty < rows; r += 4 * nty) {                    // four rows in flight per lane
                float w0[W], w1[W], w2[W], w3[W];
                ldw<W>(wp + (long long)r * out, w0);
                ldw<W>(wp + (long long)(r + nty) * out, w1);
                ldw<W>(wp + (long long)(r + 2 * nty) * out, w2);
                ldw<W>(wp + (long long)(r + 3 * nty) * out, w3);
                fma_row<NB, W>(acc, xs + r * NB, w0);
                fma_row<NB, W>(acc, xs + (r + nty) * NB, w1);
                fma_row<NB, W>(acc, xs + (r + 2 * nty) * NB, w2);
                fma_row<NB, W>(acc, xs + (r + 3 * nty) * NB, w3);
            }
            for (; r < rows; r += nty) {
                float w0[W];
                ldw<W>(wp + (long long)r * out, w0);
                fma_row<NB, W>(acc, xs + r * NB, w0);
            }
        }
    }

    if (!SPLIT) {
        if (!live) return;
        float bv[W];
#pragma unroll
        for (int k = 0; k < W; ++k) bv[k] = bias ? bias[col + k] : 0.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b < nb) {
                float r[W];
#pragma unroll
                for (int k = 0; k < W; ++k) r[k] = nrt_activate(acc[b][k] + bv[k], act);
                stw<W>(dst + (long long)b * out + col, r);
            }
        }
        return;
    }
    // reduce arm: the row lanes of a column, added in lane order ty = 0, 1, ...
    float *part = dst + (long long)blockIdx.y * nb * out;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b < nb) {                                     // (uniform)
            if (nty > 1) {
                __syncthreads();
#pragma unroll
                for (int k = 0; k < W; ++k) red[tid * W + k] = acc[b][k];
                __syncthreads();
            }
            if (ty == 0 && live) {
                float s[W];
#pragma unroll
                for (int k = 0; k < W; ++k) s[k] = acc[b][k];
                for (int j = 1; j < nty; ++j)
#pragma unroll
                    for (int k = 0; k < W; ++k) s[k] += red[(j * lanes_x + tx) * W + k];
                stw<W>(part + (long long)b * out + col, s);
            }
        }
    }
}

// dst[b, c] = act(sum_s part[s][b][c] + bias[c]), s ascending within each of 16 runs of slabs, the runs then added in run order.
// grid (ceil(n / W / 16), nb); block = 16 column lanes x 16 slab runs.
template <int W>
__global__ void __launch_bounds__(kThreads)
dense_sum_partials(const float *__restrict__ part, const float *__restrict__ bias, float *__restrict__ dst, int nslabs, int nb,
                   long long n, int act) {
    __shared__ float red[kThreads * W];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.y;
    const long long col = ((long long)blockIdx.x * 16 + tx) * W;
    const bool live = col < n;
    const int per = (nslabs + 15) / 16;
    const int s0 = min(nslabs, ty * per), s1 = min(nslabs, s0 + per);
    float s[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = 0.0f;
    if (live) {
        for (int sl = s0; sl < s1; ++sl) {
            float v[W];
            ldw<W>(part + ((long long)sl * nb + b) * n + col, v);
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) red[tid * W + k] = s[k];
    __syncthreads();
    if (ty != 0 || !live) return;
    for (int j = 1; j < 16; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] += red[(j * 16 + tx) * W + k];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = nrt_activate(s[k] + (bias ? bias[col + k] : 0.0f), act);
    stw<W>(dst + (long long)b * n + col, s);
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward wrt x.  grid (ceil(segments / 4), ceil(in / kBlockRows)); wave v of a block owns segment 4 * blockIdx.x + v (64 * W columns)
// for the block's rows.  dst: gx itself (one block column) or partials [blockIdx.x][nb][in].
// ------------------------------------------------------------------------------------------------------------------------------
// v[0 .. NB) of 64 lanes -> the sum over the wave of value b = lane >> (6 - log2 NB), in every lane of that group
template <int NB>
__device__ __forceinline__ float wave_sums(float (&v)[NB], int lane) {
    int off = 32;
#pragma unroll
    for (int n = NB; n > 1; n >>= 1, off >>= 1) {
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int j = 0; j < n / 2; ++j) {
            const float keep = up ? v[j + n / 2] : v[j];
            const float send = up ? v[j] : v[j + n / 2];
            v[j] = keep + __shfl_xor(send, off);
        }
    }
    float s = v[0];
    // (the rest of the wave, offsets descending: not nrt_wave_sum, which adds ascending and so rounds differently)
    for (; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

template <int NB> struct Log2;
template <> struct Log2<4> { static constexpr int v = 2; };
template <> struct Log2<16> { static constexpr int v = 4; };

template <int NB, int W>
__global__ void __launch_bounds__(kThreads)
dense_rowdot(const float *__restrict__ g, const float *__restrict__ w, float *__restrict__ dst, int nb, int in, int out) {
    __shared__ float red[4 * kBlockRows * NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long col = (((long long)blockIdx.x * 4 + wave) * 64 + lane) * W;
    const bool live = col < out;
    const int r_beg = blockIdx.y * kBlockRows;
    const int rows = min(kBlockRows, in - r_beg);
    constexpr int kShift = 6 - Log2<NB>::v;

    float gv[NB][W];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int k = 0; k < W; ++k) gv[b][k] = 0.0f;
        if (live && b < nb) ldw<W>(g + (long long)b * out + col, gv[b]);
    }
    const float *wp = w + (long long)r_beg * out + col;
    for (int r0 = 0; r0 < rows; r0 += 4) {                               // four rows in flight per lane (a row past the end: the last one again)
        float wv[4][W];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < W; ++k) wv[j][k] = 0.0f;
            if (live) ldw<W>(wp + (long long)min(r0 + j, rows - 1) * out, wv[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                s[b] = 0.0f;
#pragma unroll
                for (int k = 0; k < W; ++k) s[b] = fmaf(gv[b][k], wv[j][k], s[b]);
            }
            const float tot = wave_sums<NB>(s, lane);
            if (r0 + j < rows && (lane & ((1 << kShift) - 1)) == 0) red[(wave * kBlockRows + r0 + j) * NB + (lane >> kShift)] = tot;
        }
    }
    __syncthreads();
    float *o = dst + (long long)blockIdx.x * nb * in;
    for (int e = tid; e < rows * NB; e += kThreads) {
        const int r = e / NB, b = e - r * NB;
        if (b < nb) {
            float s = red[r * NB + b];
            for (int v = 1; v < 4; ++v) s += red[(v * kBlockRows + r) * NB + b];
            o[(long long)b * in + r_beg + r] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward wrt W and bias (the whole batch, b ascending)
// ------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kThreads)
dense_gw(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gw, int batch, int in, int out, unsigned col_blocks) {
    const unsigned rb = blockIdx.x / col_blocks, cb = blockIdx.x - rb * col_blocks;
    const long long col = ((long long)cb * kThreads + threadIdx.x) * W;
    if (col >= out) return;
    const int r_beg = rb * kGwRows;
    const int rows = min(kGwRows, in - r_beg);
    float acc[kGwRows][W];
#pragma unroll
    for (int r = 0; r < kGwRows; ++r)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[r][k] = 0.0f;
    for (int b = 0; b < batch; ++b) {
        float gv[W];
        ldw<W>(g + (long long)b * out + col, gv);
        const float *xb = x + (long long)b * in + r_beg;
#pragma unroll
        for (int r = 0; r < kGwRows; ++r) {
            const float xv = r < rows ? xb[r] : 0.0f;                      // (uniform over the block)
#pragma unroll
            for (int k = 0; k < W; ++k) acc[r][k] = fmaf(xv, gv[k], acc[r][k]);
        }
    }
#pragma unroll
    for (int r = 0; r < kGwRows; ++r)
        if (r < rows) stw<W>(gw + (long long)(r_beg + r) * out + col, acc[r]);
}

__global__ void __launch_bounds__(kThreads)
dense_gbias(const float *__restrict__ g, float *__restrict__ gbias, int batch, int out) {
    const long long o = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (o >= out) return;
    float s = 0.0f;
    for (int b = 0; b < batch; ++b) s += g[(long long)b * out + o];
    gbias[o] = s;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int pow2_at_least(long long v, int cap) {
    int p = 1;
    while (p < cap && p < v) p <<= 1;
    return p;
}

struct FwdPlan {
    bool split;
    int lanes_x, slab_rows, nslabs;
    unsigned col_blocks;
};

// variant 0: the expand arm once its one-thread-per-column-group grid fills half the chip (128 blocks) or there is nothing to cut
// (fewer than 32 rows); the reduce arm otherwise.
inline FwdPlan fwd_plan(int in, int out, int w, int variant) {
    FwdPlan p;
    const long long groups = ((long long)out + w - 1) / w;
    const long long expand_blocks = (groups + kThreads - 1) / kThreads;
    p.split = variant == 1 || (variant == 0 && expand_blocks < 128 && in >= 32);
    if (!p.split) {
        p.lanes_x = kThreads;
        p.slab_rows = in;
        p.nslabs = 1;
        p.col_blocks = (unsigned)expand_blocks;
        return p;
    }
    p.lanes_x = pow2_at_least(groups, 64);
    p.col_blocks = (unsigned)((groups + p.lanes_x - 1) / p.lanes_x);
    long long want = kTargetBlocks / (long long)p.col_blocks;
    want = want < 1 ? 1 : (want > kMaxSlabs ? kMaxSlabs : want);
    const long long most = ((long long)in + 15) / 16;                     // a slab is at least 16 rows
    if (want > most) want = most;
    p.slab_rows = (int)(((long long)in + want - 1) / want);
    p.nslabs = (in + p.slab_rows - 1) / p.slab_rows;
    return p;
}

inline long long gx_block_cols(int out, int w) {                          // blocks along `out` of dense_rowdot
    const long long segs = ((long long)out + 64 * w - 1) / (64 * w);
    return (segs + 3) / 4;
}

inline int chunk_of(int batch) { return batch < kMaxChunk ? batch : kMaxChunk; }

inline bool valid_sizes(int batch, int in, int out, int &rc) {
    if (batch < 1 || in < 1 || out < 1) { rc = NRT_ERR_INVALID_ARG; return false; }
    if ((long long)in * out >= (1LL << 31)) { rc = NRT_ERR_UNSUPPORTED; return false; }
    return true;
}

template <int W>
int sum_partials(const float *part, const float *bias, float *dst, int nslabs, int nb, long long n, int act, hipStream_t st) {
    const long long bx = ((n + W - 1) / W + 15) / 16;
    hipLaunchKernelGGL(dense_sum_partials<W>, dim3((unsigned)bx, (unsigned)nb), dim3(kThreads), 0, st, part, bias, dst, nslabs, nb, n, act);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

template <int NB, int W>
int launch_fwd(const FwdPlan &p, const float *x, const float *w, const float *bias, float *dst, int nb, int in, int out, int act,
               hipStream_t st) {
    if (p.split)
        hipLaunchKernelGGL((dense_fwd<NB, W, true>), dim3(p.col_blocks, (unsigned)p.nslabs), dim3(kThreads), 0, st, x, w, bias, dst, nb, in,
                           out, act, p.slab_rows, p.lanes_x);
    else
        hipLaunchKernelGGL((dense_fwd<NB, W, false>), dim3(p.col_blocks), dim3(kThreads), 0, st, x, w, bias, dst, nb, in, out, act,
                           p.slab_rows, p.lanes_x);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

template <int NB, int W>
int launch_rowdot(const float *g, const float *w, float *dst, int nb, int in, int out, hipStream_t st) {
    const dim3 grid((unsigned)gx_block_cols(out, W), (unsigned)((in + kBlockRows - 1) / kBlockRows));
    hipLaunchKernelGGL((dense_rowdot<NB, W>), grid, dim3(kThreads), 0, st, g, w, dst, nb, in, out);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

}  // namespace

// The larger of what the forward and the backward of this shape ask for under `variant`, whichever of the 16-byte and 4-byte forms the
// pointers of the call select; 0 = no workspace needed.
extern "C" size_t nrt_dense_workspace_bytes(int batch, int in, int out, int variant) {
    int rc;
    if (!valid_sizes(batch, in, out, rc) || variant < 0 || variant > 2) return 0;
    const int nb = chunk_of(batch);
    size_t need = 0;
    for (int w = 1; w <= 4; w += 3) {
        if (w == 4 && out % 4 != 0) continue;
        const FwdPlan p = fwd_plan(in, out, w, variant);
        if (p.split) need = std::max(need, (size_t)p.nslabs * nb * out * sizeof(float));
        const long long bc = gx_block_cols(out, w);
        if (bc > 1 || variant == 1) need = std::max(need, (size_t)bc * nb * in * sizeof(float));
    }
    return need;
}

extern "C" int nrt_dense_f32(const float *x, const float *w, const float *bias, float *y, int batch, int in, int out, int act,
                             int variant, void *workspace, size_t workspace_bytes, void *stream) {
    int rc;
    if (!x || !w || !y || act < 0 || act > ACT_LAST || variant < 0 || variant > 2) return NRT_ERR_INVALID_ARG;
    if (!valid_sizes(batch, in, out, rc)) return rc;
    hipStream_t st = nrt_stream(stream);
    float *ws = (float *)workspace;
    for (int b0 = 0; b0 < batch; b0 += kMaxChunk) {
        const int nb = std::min(kMaxChunk, batch - b0);
        const float *xc = x + (long long)b0 * in;
        float *yc = y + (long long)b0 * out;
        const bool vec = out % 4 == 0 && aligned16(w) && aligned16(yc) && aligned16(ws);
        const FwdPlan p = fwd_plan(in, out, vec ? 4 : 1, variant);
        float *dst = yc;
        if (p.split) {
            if (!ws || workspace_bytes < (size_t)p.nslabs * nb * out * sizeof(float)) return NRT_ERR_WORKSPACE;
            dst = ws;
        }
        if (vec) rc = nb <= 4 ? launch_fwd<4, 4>(p, xc, w, bias, dst, nb, in, out, act, st)
                              : launch_fwd<16, 4>(p, xc, w, bias, dst, nb, in, out, act, st);
        else rc = nb <= 4 ? launch_fwd<4, 1>(p, xc, w, bias, dst, nb, in, out, act, st)
                          : launch_fwd<16, 1>(p, xc, w, bias, dst, nb, in, out, act, st);
        if (rc != NRT_OK) return rc;
        if (p.split) {
            rc = vec ? sum_partials<4>(ws, bias, yc, p.nslabs, nb, out, act, st) : sum_partials<1>(ws, bias, yc, p.nslabs, nb, out, act, st);
            if (rc != NRT_OK) return rc;
        }
    }
    return NRT_OK;
}

// variant 0 / 2: gx is written by the row-dot kernel itself where one block spans a row (out <= 4 * 64 * W columns), through
// partials otherwise; variant 1: always through partials and the second stage.
extern "C" int nrt_dense_bwd_f32(const float *g, const float *x, const float *w, float *gx, float *gw, float *gbias, int batch, int in,
                                 int out, int variant, void *workspace, size_t workspace_bytes, void *stream) {
    int rc;
    if (!g || variant < 0 || variant > 2 || (gx && !w) || (gw && !x)) return NRT_ERR_INVALID_ARG;
    if (!valid_sizes(batch, in, out, rc)) return rc;
    hipStream_t st = nrt_stream(stream);
    float *ws = (float *)workspace;
    for (int b0 = 0; gx && b0 < batch; b0 += kMaxChunk) {
        const int nb = std::min(kMaxChunk, batch - b0);
        const float *gc = g + (long long)b0 * out;
        float *gxc = gx + (long long)b0 * in;
        const bool vec = out % 4 == 0 && aligned16(w) && aligned16(gc);
        const long long bc = gx_block_cols(out, vec ? 4 : 1);
        const bool partials = bc > 1 || variant == 1;
        float *dst = gxc;
        if (partials) {
            if (!ws || workspace_bytes < (size_t)bc * nb * in * sizeof(float)) return NRT_ERR_WORKSPACE;
            dst = ws;
        }
        if (vec) rc = nb <= 4 ? launch_rowdot<4, 4>(gc, w, dst, nb, in, out, st) : launch_rowdot<16, 4>(gc, w, dst, nb, in, out, st);
        else rc = nb <= 4 ? launch_rowdot<4, 1>(gc, w, dst, nb, in, out, st) : launch_rowdot<16, 1>(gc, w, dst, nb, in, out, st);
        if (rc != NRT_OK) return rc;
        if (partials) {
            const bool v4 = in % 4 == 0 && aligned16(ws) && aligned16(gxc);
            rc = v4 ? sum_partials<4>(ws, nullptr, gxc, (int)bc, nb, in, ACT_NONE, st)
                    : sum_partials<1>(ws, nullptr, gxc, (int)bc, nb, in, ACT_NONE, st);
            if (rc != NRT_OK) return rc;
        }
    }
    if (gw) {
        const bool vec = out % 4 == 0 && aligned16(g) && aligned16(gw);
        const long long groups = ((long long)out + (vec ? 4 : 1) - 1) / (vec ? 4 : 1);
        const unsigned cb = (unsigned)((groups + kThreads - 1) / kThreads);
        const long long blocks = (long long)cb * ((in + kGwRows - 1) / kGwRows);
        if (blocks > 0x7fffffffLL) return NRT_ERR_UNSUPPORTED;
        if (vec) hipLaunchKernelGGL(dense_gw<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, g, gw, batch, in, out, cb);
        else hipLaunchKernelGGL(dense_gw<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, g, gw, batch, in, out, cb);
        NRT_CHECK_LAUNCH();
    }
    if (gbias) {
        hipLaunchKernelGGL(dense_gbias, dim3((unsigned)((out + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g, gbias, batch, out);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}
