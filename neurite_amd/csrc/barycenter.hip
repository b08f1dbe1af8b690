// Barycenter (centre of mass) of feature maps: neurite/tf/utils/utils.py:512-573 in one pass over the input, and its gradient.
//
// The kernels see x [outer, R = r_0 * ... * r_{k-1}, inner] (1 <= k <= 8 reduced dimensions, the last one innermost), stored as
// float32, bfloat16 or float16 and widened to float32 in registers, and produce
//     sums[o, i, d] = sum_r g_d(r) x[o, r, i]  (d < k),   sums[o, i, k] = D = sum_r x[o, r, i]        (float32)
//     y[o, i, d]    = divide_no_nan(sums[o, i, d], D)                                                  (exactly 0 where D == 0)
// g_d(r) = ((float)i_d - (v_d - 1) / 2 if shift_center) / v_d if normalize: the reference's float32 grid value, bit for bit (the
// subtraction is exact for v_d < 2^24, the division is the correctly rounded one).  The grid is never materialised: where the sizes of
// the reduced dimensions add up to at most kTab values every block computes them once into LDS, otherwise they are computed where used.
//
// A line is a run along the innermost reduced dimension.  The coordinates of the other k - 1 dimensions are constant over a line, so a
// thread adds x up over its part of a line and multiplies that sum in once at the end of the line: an element costs one add and one
// fmaf (for g_{k-1}), not k + 1 fmaf.
//
//   forward, first stage     a block owns a slab of R of one `outer` entry (and a tile of columns) and leaves [k + 1][inner] float32
//                            partials in the workspace.
//     inner arm              lanes run along `inner` in 16-byte groups (4 floats / 8 halves), the rows of the slab are dealt to the
//                            block's row lanes, four rows in flight per lane; row lanes are added by wave shuffles, waves through LDS.
//     trailing arm           inner == 1: lanes run along R with 16-byte loads, the elements of a slab in front of and behind the
//                            16-byte groups go one by one through the same body.
//     Where inner is no multiple of the group or a base pointer is not 16-byte aligned both arms run per element (the same body,
//     W = 1).  Which arm and which width run is decided by the dispatch below; each is correct at every shape it is given.
//   forward, second stage    bc_finish: the slabs of an output are dealt to up to 256 runs, each run is added in slab order in float64,
//                            the runs are added by a halving tree in LDS, then the IEEE division with the D == 0 case.
//   backward                 bc_bwd_coef forms b_d = gy_d / D and a = -sum_d gy_d y_d / D per (outer, inner) (all 0 where D == 0); one
//                            streaming kernel per arm writes gx = a + sum_d b_d g_d(r) in x's storage type with 16-byte stores: the
//                            part that is constant over a line is formed once per line, an element costs one fmaf.
//
// No atomics.  Every sum has a fixed partition and a fixed order given the shapes and the alignment of the pointers: results are
// run-to-run bit-identical.  Products are accumulated with fmaf (one rounding per term).
#include "wave_ops.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 8;
constexpr int kTab = 4096;               // coordinate values a block keeps in LDS (16 KB)
constexpr int kTargetBlocks = 2048;      // the first stage cuts R until about this many blocks exist (8 per CU)
constexpr int kFlagNormalize = 1, kFlagShift = 2;

typedef unsigned nrt_u4 __attribute__((ext_vector_type(4)));
typedef _Float16 nrt_h8 __attribute__((ext_vector_type(8)));
struct Bf16 { unsigned short bits; };

struct BcDims {
    int k, flags, use_tab;
    int rk;                              // v[k - 1], the length of a line
    int nlines;                          // R / rk
    int v[kMaxK];                        // sizes of the reduced dimensions
    int off[kMaxK];                      // where dimension d starts in the LDS table
    int off_k;                           // off[k - 1]
};

// the reference's grid value of index i along a dimension of size v (utils.py:557-561)
__device__ __forceinline__ float bc_grid(int i, int v, int flags) {
    float g = (float)i;
    if (flags & kFlagShift) g = nrt_sub(g, 0.5f * (float)(v - 1));       // both exact below 2^24
    if (flags & kFlagNormalize) g = g / (float)v;                        // correctly rounded
    return g;
}

__device__ __forceinline__ void bc_fill_table(float *tab, const BcDims &P) {
    if (P.use_tab) {
#pragma unroll
        for (int d = 0; d < kMaxK; ++d)
            if (d < P.k)
                for (int i = threadIdx.x; i < P.v[d]; i += kThreads) tab[P.off[d] + i] = bc_grid(i, P.v[d], P.flags);
    }
    __syncthreads();
}

// ---- storage types: W elements at element index e of `base` <-> float32 ---------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {                                     // round to nearest even
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <typename ST, int W> struct BcIO;
template <> struct BcIO<float, 1> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[1]) { v[0] = ((const float *)b)[e]; }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[1]) { ((float *)b)[e] = v[0]; }
};
template <> struct BcIO<float, 4> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[4]) {
        const nrt_f4 t = __builtin_nontemporal_load((const nrt_f4 *)((const float *)b + e));
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[4]) {
        *(nrt_f4 *)((float *)b + e) = (nrt_f4){v[0], v[1], v[2], v[3]};
    }
};
template <> struct BcIO<Bf16, 1> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[1]) { v[0] = bf16_to_f32(((const unsigned short *)b)[e]); }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[1]) { ((unsigned short *)b)[e] = f32_to_bf16(v[0]); }
};
template <> struct BcIO<Bf16, 8> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[8]) {
        const nrt_u4 t = __builtin_nontemporal_load((const nrt_u4 *)((const unsigned short *)b + e));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(t[j] << 16);
            v[2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[8]) {
        nrt_u4 t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (unsigned)f32_to_bf16(v[2 * j]) | ((unsigned)f32_to_bf16(v[2 * j + 1]) << 16);
        *(nrt_u4 *)((unsigned short *)b + e) = t;
    }
};
template <> struct BcIO<_Float16, 1> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[1]) { v[0] = (float)((const _Float16 *)b)[e]; }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[1]) { ((_Float16 *)b)[e] = (_Float16)v[0]; }
};
template <> struct BcIO<_Float16, 8> {
    static __device__ __forceinline__ void load(const void *b, long long e, float (&v)[8]) {
        const nrt_h8 t = __builtin_nontemporal_load((const nrt_h8 *)((const _Float16 *)b + e));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
    }
    static __device__ __forceinline__ void store(void *b, long long e, const float (&v)[8]) {
        nrt_h8 t;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (_Float16)v[j];
        *(nrt_h8 *)((_Float16 *)b + e) = t;
    }
};

// ---- where a thread is in R: line q, index ik within the line, and the coordinates of the line's other dimensions ------------------
struct BcPos {
    int q, ik;
    float gd[kMaxK - 1];

    __device__ __forceinline__ float grid(const BcDims &P, const float *tab, int d, int i) const {
        return P.use_tab ? tab[P.off[d] + i] : bc_grid(i, P.v[d], P.flags);
    }
    // coordinate along the innermost dimension of the element j places further along the line
    __device__ __forceinline__ float gk(const BcDims &P, const float *tab, int j = 0) const {
        return P.use_tab ? tab[P.off_k + ik + j] : bc_grid(ik + j, P.rk, P.flags);
    }
    __device__ __forceinline__ void set_line(const BcDims &P, const float *tab) {
        int rem = q;
#pragma unroll
        for (int d = kMaxK - 2; d >= 0; --d) {
            if (d < P.k - 1) {
                const int vd = P.v[d], hi = rem / vd;
                gd[d] = grid(P, tab, d, rem - hi * vd);
                rem = hi;
            }
        }
    }
    __device__ __forceinline__ void init(const BcDims &P, const float *tab, int r) {
        q = r / P.rk;
        ik = r - q * P.rk;
#pragma unroll
        for (int d = 0; d < kMaxK - 1; ++d) gd[d] = 0.0f;
        set_line(P, tab);
    }
    __device__ __forceinline__ bool leaves_line(const BcDims &P, int n) const { return ik + n >= P.rk; }
    // n places on; past the last line the coordinates keep their last values (nothing is read or written there)
    __device__ __forceinline__ void advance(const BcDims &P, const float *tab, int n) {
        ik += n;
        if (ik >= P.rk) {
            const int dq = ik / P.rk;
            ik -= dq * P.rk;
            q += dq;
            if (q < P.nlines) set_line(P, tab);
        }
    }
};

// ---- the sums of NC columns ---------------------------------------------------------------------------------------------------
template <int NC>
struct BcAcc {
    float s[NC];                         // sum of x over the thread's part of the current line
    float t[NC];                         // sum of g_{k-1} x
    float den[NC];                       // D
    float acc[kMaxK - 1][NC];            // sum of g_d x, d < k - 1

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            s[c] = t[c] = den[c] = 0.0f;
#pragma unroll
            for (int d = 0; d < kMaxK - 1; ++d) acc[d][c] = 0.0f;
        }
    }
    __device__ __forceinline__ void add(const float (&x)[NC], float gk) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            s[c] += x[c];
            t[c] = fmaf(gk, x[c], t[c]);
        }
    }
    // the end of the thread's part of a line
    __device__ __forceinline__ void flush(const BcDims &P, const BcPos &pos) {
#pragma unroll
        for (int d = 0; d < kMaxK - 1; ++d) {
            if (d < P.k - 1) {
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[d][c] = fmaf(pos.gd[d], s[c], acc[d][c]);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            den[c] += s[c];
            s[c] = 0.0f;
        }
    }
};

struct BcPlan {
    int lanes_x;                         // column lanes of a block (inner arm; a power of two up to 64)
    int col_tiles;                       // blocks along `inner`
    int nslabs, slab_rows;               // slabs of R and their length
};

// one row of a block's partials (inner arm): lanes that agree in lane % lanes_x hold the same columns
template <int W>
__device__ __forceinline__ void bc_block_sum(const float (&v)[W], float (*red)[NRT_WAVE * W], int lanes_x, bool writer, float *dst) {
    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    float s[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        s[c] = v[c];
        // (nrt_wave_sum_from by hand: through the helper bc_fwd_inner<., 8> changes its SGPRs)
        for (int off = lanes_x; off < NRT_WAVE; off <<= 1) s[c] += __shfl_xor(s[c], off, NRT_WAVE);
    }
    __syncthreads();                                        // the previous row has been read
#pragma unroll
    for (int c = 0; c < W; ++c) red[wave][lane * W + c] = s[c];
    __syncthreads();
    if (writer) {
        for (int w2 = 1; w2 < kThreads / NRT_WAVE; ++w2)
#pragma unroll
            for (int c = 0; c < W; ++c) s[c] += red[w2][lane * W + c];
#pragma unroll
        for (int c = 0; c < W; ++c) dst[c] = s[c];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// forward, inner arm.  grid = outer * nslabs * col_tiles; part [outer][nslabs][k + 1][inner]
// ------------------------------------------------------------------------------------------------------------------------------
template <typename ST, int W>
__global__ void __launch_bounds__(kThreads)
bc_fwd_inner(const void *__restrict__ x, float *__restrict__ part, BcDims P, BcPlan pl, int R, int inner) {
    __shared__ float tab[kTab];
    __shared__ float red[kThreads / NRT_WAVE][NRT_WAVE * W];
    bc_fill_table(tab, P);
    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const unsigned ct = bid % pl.col_tiles, so = bid / pl.col_tiles;
    const unsigned slab = so % pl.nslabs, o = so / pl.nslabs;
    const int tx = tid & (pl.lanes_x - 1), ty = tid / pl.lanes_x, nty = kThreads / pl.lanes_x;
    const long long col = ((long long)ct * pl.lanes_x + tx) * W;
    const bool live = col < inner;                          // (W > 1 only where inner % W == 0: a live group is whole)
    const int r_beg = slab * pl.slab_rows;
    const int r_end = min(R, r_beg + pl.slab_rows);

    BcAcc<W> a;
    a.zero();
    BcPos pos;
    if (live && r_beg + ty < r_end) {
        pos.init(P, tab, r_beg + ty);
        const long long base = (long long)o * R * inner + col;
        for (int r = r_beg + ty; r < r_end; r += 4 * nty) {                     // four rows in flight per lane
            float v[4][W];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rr = r + j * nty;
                if (rr < r_end) BcIO<ST, W>::load(x, base + (long long)rr * inner, v[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r + j * nty < r_end) {
                    a.add(v[j], pos.gk(P, tab));
                    if (pos.leaves_line(P, nty)) a.flush(P, pos);
                    pos.advance(P, tab, nty);
                }
            }
        }
        a.flush(P, pos);
    }

    // row lanes of a column: the lanes of a wave by shuffles, then the waves through LDS in wave order
    float *dst = part + ((long long)o * pl.nslabs + slab) * (P.k + 1) * inner + col;
    const bool writer = ty == 0 && live;                    // lanes 0 .. lanes_x - 1 of wave 0
#pragma unroll
    for (int d = 0; d < kMaxK - 1; ++d)
        if (d < P.k - 1) bc_block_sum<W>(a.acc[d], red, pl.lanes_x, writer, dst + (long long)d * inner);
    bc_block_sum<W>(a.t, red, pl.lanes_x, writer, dst + (long long)(P.k - 1) * inner);
    bc_block_sum<W>(a.den, red, pl.lanes_x, writer, dst + (long long)P.k * inner);
}

// ------------------------------------------------------------------------------------------------------------------------------
// forward, trailing arm (inner == 1).  grid = outer * nslabs; part [outer][nslabs][k + 1]
// ------------------------------------------------------------------------------------------------------------------------------
// the elements in front of and behind a slab's 16-byte groups: [r_beg, r_beg + head) and [r_end - tail, r_end)
struct BcSplit { int head, groups, tail; };
template <int W>
__device__ __forceinline__ BcSplit bc_split(long long flat_beg, int len) {
    BcSplit sp;
    sp.head = W > 1 ? (int)((W - flat_beg % W) % W) : 0;
    if (sp.head > len) sp.head = len;
    sp.groups = (len - sp.head) / W;
    sp.tail = len - sp.head - sp.groups * W;
    return sp;
}

template <typename ST, int W>
__global__ void __launch_bounds__(kThreads)
bc_fwd_trail(const void *__restrict__ x, float *__restrict__ part, BcDims P, BcPlan pl, int R) {
    __shared__ float tab[kTab];
    __shared__ float red[kThreads / NRT_WAVE][kMaxK + 1];
    bc_fill_table(tab, P);
    const int tid = threadIdx.x;
    const unsigned slab = blockIdx.x % pl.nslabs, o = blockIdx.x / pl.nslabs;
    const int r_beg = slab * pl.slab_rows;
    const int r_end = min(R, r_beg + pl.slab_rows);
    const long long base = (long long)o * R;
    const BcSplit sp = bc_split<W>(base + r_beg, r_end - r_beg);

    BcAcc<1> a;
    a.zero();
    BcPos pos;
    // the ragged ends, one element per thread
    if (tid < sp.head + sp.tail) {
        const int r = tid < sp.head ? r_beg + tid : r_end - sp.tail + (tid - sp.head);
        float v[1];
        BcIO<ST, 1>::load(x, base + r, v);
        pos.init(P, tab, r);
        a.add(v, pos.gk(P, tab));
        a.flush(P, pos);
    }
    if (tid < sp.groups) {
        const int g_beg = r_beg + sp.head;
        pos.init(P, tab, g_beg + tid * W);
        for (int g = tid; g < sp.groups; g += 4 * kThreads) {                  // four groups in flight per lane
            float v[4][W];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gg = g + j * kThreads;
                if (gg < sp.groups) BcIO<ST, W>::load(x, base + g_beg + (long long)gg * W, v[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g + j * kThreads < sp.groups) {
                    if (pos.ik + W <= P.rk) {                                  // the group lies within a line
#pragma unroll
                        for (int c = 0; c < W; ++c) {
                            const float one[1] = {v[j][c]};
                            a.add(one, pos.gk(P, tab, c));
                        }
                        if (pos.leaves_line(P, kThreads * W)) a.flush(P, pos);
                        pos.advance(P, tab, kThreads * W);
                    } else {
#pragma unroll
                        for (int c = 0; c < W; ++c) {
                            const float one[1] = {v[j][c]};
                            a.add(one, pos.gk(P, tab));
                            if (pos.leaves_line(P, 1)) a.flush(P, pos);
                            pos.advance(P, tab, 1);
                        }
                        if (pos.leaves_line(P, (kThreads - 1) * W)) a.flush(P, pos);
                        pos.advance(P, tab, (kThreads - 1) * W);
                    }
                }
            }
        }
        a.flush(P, pos);
    }

    const int lane = tid & (NRT_WAVE - 1), wave = tid / NRT_WAVE;
#pragma unroll
    for (int d = 0; d < kMaxK - 1; ++d) {
        if (d < P.k - 1) {
            const float s = nrt_wave_sum(a.acc[d][0]);
            if (lane == 0) red[wave][d] = s;
        }
    }
    const float st = nrt_wave_sum(a.t[0]), sd = nrt_wave_sum(a.den[0]);
    if (lane == 0) {
        red[wave][P.k - 1] = st;
        red[wave][P.k] = sd;
    }
    __syncthreads();
    if (tid <= P.k) {
        float s = red[0][tid];
        for (int w2 = 1; w2 < kThreads / NRT_WAVE; ++w2) s += red[w2][tid];
        part[((long long)o * pl.nslabs + slab) * (P.k + 1) + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// second stage.  A block is cl column lanes x nrun runs of slabs x (256 / (cl nrun)) `outer` entries; run j adds slabs
// [j per, (j + 1) per) in slab order in float64, the runs are added by a halving tree.  grid (col tiles, ceil(outer / entries)).
// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
bc_finish(const float *__restrict__ part, float *__restrict__ y, float *__restrict__ sums, int k, long long outer, int inner, int nslabs,
          int cl, int nrun, unsigned col_tiles) {
    __shared__ double sh[kMaxK + 1][kThreads];
    const int tid = threadIdx.x;
    const int tx = tid % cl, run = (tid / cl) % nrun, oo = tid / (cl * nrun);
    const unsigned ct = blockIdx.x % col_tiles, ob = blockIdx.x / col_tiles;
    const long long o = (long long)ob * (kThreads / (cl * nrun)) + oo;
    const int i = ct * cl + tx;
    const bool live = o < outer && i < inner;
    const int per = (nslabs + nrun - 1) / nrun;
    const int s0 = min(nslabs, run * per), s1 = min(nslabs, s0 + per);
    double a[kMaxK + 1];
#pragma unroll
    for (int d = 0; d <= kMaxK; ++d) a[d] = 0.0;
    if (live) {
        for (int s = s0; s < s1; ++s) {
            const float *p = part + ((o * nslabs + s) * (k + 1)) * inner + i;
            float v[kMaxK + 1];
#pragma unroll
            for (int d = 0; d <= kMaxK; ++d) v[d] = d <= k ? p[(long long)d * inner] : 0.0f;
#pragma unroll
            for (int d = 0; d <= kMaxK; ++d) a[d] += (double)v[d];
        }
    }
#pragma unroll
    for (int d = 0; d <= kMaxK; ++d) sh[d][tid] = a[d];
    for (int h = nrun >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (run < h) {
#pragma unroll
            for (int d = 0; d <= kMaxK; ++d) sh[d][tid] += sh[d][tid + h * cl];
        }
    }
    if (run != 0 || !live) return;
    // (a thread of run 0 reads back only what it wrote itself last)
    float den = 0.0f;
#pragma unroll
    for (int d = 0; d <= kMaxK; ++d)
        if (d == k) den = (float)sh[d][tid];
    const long long oi = o * inner + i;
#pragma unroll
    for (int d = 0; d < kMaxK; ++d) {
        if (d < k) {
            const float num = (float)sh[d][tid];
            sums[oi * (k + 1) + d] = num;
            y[oi * k + d] = den == 0.0f ? 0.0f : num / den;              // tf.math.divide_no_nan
        }
    }
    sums[oi * (k + 1) + k] = den;
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward.  coef [outer][k + 1][inner]: rows d < k are b_d, row k is a.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
bc_bwd_coef(const float *__restrict__ gy, const float *__restrict__ y, const float *__restrict__ sums, float *__restrict__ coef, int k,
            long long outer, int inner) {
    const long long oi = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (oi >= outer * inner) return;
    const long long o = oi / inner;
    const int i = (int)(oi - o * inner);
    const float den = sums[oi * (k + 1) + k];
    float *c = coef + o * (k + 1) * inner + i;
    float dot = 0.0f;
    for (int d = 0; d < k; ++d) {
        const float g = gy[oi * k + d];
        dot = fmaf(g, y[oi * k + d], dot);
        c[(long long)d * inner] = den == 0.0f ? 0.0f : g / den;
    }
    c[(long long)k * inner] = den == 0.0f ? 0.0f : -dot / den;
}

// the coefficients of NC columns and the part of gx that is constant over a line
template <int NC>
struct BcGrad {
    float a[NC], bk[NC], line[NC];
    float b[kMaxK - 1][NC];

    __device__ __forceinline__ void load(const float *coef /* at [o][0][col] */, const BcDims &P, int inner) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a[c] = coef[(long long)P.k * inner + c];
            bk[c] = coef[(long long)(P.k - 1) * inner + c];
#pragma unroll
            for (int d = 0; d < kMaxK - 1; ++d) b[d][c] = d < P.k - 1 ? coef[(long long)d * inner + c] : 0.0f;
        }
    }
    __device__ __forceinline__ void set_line(const BcDims &P, const BcPos &pos) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float v = a[c];
#pragma unroll
            for (int d = 0; d < kMaxK - 1; ++d)
                if (d < P.k - 1) v = fmaf(b[d][c], pos.gd[d], v);
            line[c] = v;
        }
    }
};

template <typename ST, int W>
__global__ void __launch_bounds__(kThreads)
bc_bwd_inner(const float *__restrict__ coef, void *__restrict__ gx, BcDims P, BcPlan pl, int R, int inner) {
    __shared__ float tab[kTab];
    bc_fill_table(tab, P);
    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const unsigned ct = bid % pl.col_tiles, so = bid / pl.col_tiles;
    const unsigned slab = so % pl.nslabs, o = so / pl.nslabs;
    const int tx = tid & (pl.lanes_x - 1), ty = tid / pl.lanes_x, nty = kThreads / pl.lanes_x;
    const long long col = ((long long)ct * pl.lanes_x + tx) * W;
    const int r_beg = slab * pl.slab_rows;
    const int r_end = min(R, r_beg + pl.slab_rows);
    if (col >= inner || r_beg + ty >= r_end) return;

    BcGrad<W> g;
    g.load(coef + (long long)o * (P.k + 1) * inner + col, P, inner);
    BcPos pos;
    pos.init(P, tab, r_beg + ty);
    g.set_line(P, pos);
    const long long base = (long long)o * R * inner + col;
    for (int r = r_beg + ty; r < r_end; r += nty) {
        const float gk = pos.gk(P, tab);
        float v[W];
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = fmaf(g.bk[c], gk, g.line[c]);
        BcIO<ST, W>::store(gx, base + (long long)r * inner, v);
        const int q = pos.q;
        pos.advance(P, tab, nty);
        if (pos.q != q) g.set_line(P, pos);
    }
}

template <typename ST, int W>
__global__ void __launch_bounds__(kThreads)
bc_bwd_trail(const float *__restrict__ coef, void *__restrict__ gx, BcDims P, BcPlan pl, int R) {
    __shared__ float tab[kTab];
    bc_fill_table(tab, P);
    const int tid = threadIdx.x;
    const unsigned slab = blockIdx.x % pl.nslabs, o = blockIdx.x / pl.nslabs;
    const int r_beg = slab * pl.slab_rows;
    const int r_end = min(R, r_beg + pl.slab_rows);
    const long long base = (long long)o * R;
    const BcSplit sp = bc_split<W>(base + r_beg, r_end - r_beg);

    BcGrad<1> g;
    g.load(coef + (long long)o * (P.k + 1), P, 1);
    BcPos pos;
    if (tid < sp.head + sp.tail) {
        const int r = tid < sp.head ? r_beg + tid : r_end - sp.tail + (tid - sp.head);
        pos.init(P, tab, r);
        g.set_line(P, pos);
        const float v[1] = {fmaf(g.bk[0], pos.gk(P, tab), g.line[0])};
        BcIO<ST, 1>::store(gx, base + r, v);
    }
    if (tid >= sp.groups) return;
    const int g_beg = r_beg + sp.head;
    pos.init(P, tab, g_beg + tid * W);
    g.set_line(P, pos);
    for (int gi = tid; gi < sp.groups; gi += kThreads) {
        float v[W];
        int q = pos.q;
        if (pos.ik + W <= P.rk) {                                              // the group lies within a line
#pragma unroll
            for (int c = 0; c < W; ++c) v[c] = fmaf(g.bk[0], pos.gk(P, tab, c), g.line[0]);
            pos.advance(P, tab, kThreads * W);
        } else {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                v[c] = fmaf(g.bk[0], pos.gk(P, tab), g.line[0]);
                pos.advance(P, tab, 1);
                if (pos.q != q) { g.set_line(P, pos); q = pos.q; }
            }
            pos.advance(P, tab, (kThreads - 1) * W);
        }
        if (pos.q != q) g.set_line(P, pos);
        BcIO<ST, W>::store(gx, base + g_beg + (long long)gi * W, v);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

inline int pow2_at_least(long long v, int cap) {
    int p = 1;
    while (p < cap && p < v) p <<= 1;
    return p;
}

// inner >= 2: the inner arm; inner == 1: the trailing arm (the inner arm with one column lane computes the same sums, lanes idle)
inline BcPlan make_plan(long long outer, long long R, long long inner, int w) {
    BcPlan p;
    long long unit;                                         // rows a slab has at least: four per (row) lane
    if (inner == 1) {
        p.lanes_x = 1;
        p.col_tiles = 1;
        unit = 4LL * kThreads * w;
    } else {
        const long long groups = (inner + w - 1) / w;
        p.lanes_x = pow2_at_least(groups, NRT_WAVE);
        p.col_tiles = (int)((groups + p.lanes_x - 1) / p.lanes_x);
        unit = 4LL * (kThreads / p.lanes_x);
    }
    long long want = kTargetBlocks / (outer * p.col_tiles > kTargetBlocks ? kTargetBlocks : outer * p.col_tiles);
    const long long most = std::max(1LL, R / unit);
    want = std::max(1LL, std::min(want, most));
    p.slab_rows = (int)((R + want - 1) / want);
    p.nslabs = (int)((R + p.slab_rows - 1) / p.slab_rows);
    return p;
}

struct BcShape {
    BcDims P;
    long long outer, R, inner;
};

// argument checks shared by the three entry points; NRT_OK or the refusal
inline int check_shape(int dtype, long long outer, const int *red_shape, int k, long long inner, int normalize, int shift_center,
                       BcShape &s) {
    if (k < 1 || k > kMaxK || !red_shape || outer < 1 || inner < 1) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < k; ++d)
        if (red_shape[d] < 1) return NRT_ERR_INVALID_ARG;
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_BF16 && dtype != NRT_DT_F16) return NRT_ERR_UNSUPPORTED;
    long long R = 1, total = 0;
    for (int d = 0; d < k; ++d) {
        if (red_shape[d] >= (1 << 24)) return NRT_ERR_UNSUPPORTED;
        R *= red_shape[d];
        if (R >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
        total += red_shape[d];
    }
    if (outer >= (1LL << 31) || inner >= (1LL << 31) || outer * R >= (1LL << 31) || outer * R * inner >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    BcDims &P = s.P;
    P.k = k;
    P.flags = (normalize ? kFlagNormalize : 0) | (shift_center ? kFlagShift : 0);
    P.use_tab = total <= kTab;
    P.rk = red_shape[k - 1];
    P.nlines = (int)(R / P.rk);
    int off = 0;
    for (int d = 0; d < kMaxK; ++d) {
        P.v[d] = d < k ? red_shape[d] : 1;
        P.off[d] = P.use_tab ? off : 0;
        if (d == k - 1) P.off_k = P.off[d];
        off += d < k ? red_shape[d] : 0;
    }
    s.outer = outer;
    s.R = R;
    s.inner = inner;
    return NRT_OK;
}

inline size_t part_bytes(const BcShape &s, int w) {
    const BcPlan p = make_plan(s.outer, s.R, s.inner, w);
    return (size_t)s.outer * p.nslabs * (s.P.k + 1) * s.inner * sizeof(float);
}
inline size_t coef_bytes(const BcShape &s) { return (size_t)s.outer * (s.P.k + 1) * s.inner * sizeof(float); }
inline int vec_width(int dtype) { return dtype == NRT_DT_F32 ? 4 : 8; }

template <typename ST, int W>
int launch_fwd(const void *x, float *part, const BcShape &s, const BcPlan &p, hipStream_t st) {
    const long long blocks = s.outer * p.nslabs * p.col_tiles;
    if (blocks > 0x7fffffffLL) return NRT_ERR_UNSUPPORTED;
    if (s.inner == 1)
        hipLaunchKernelGGL((bc_fwd_trail<ST, W>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, part, s.P, p, (int)s.R);
    else
        hipLaunchKernelGGL((bc_fwd_inner<ST, W>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, part, s.P, p, (int)s.R, (int)s.inner);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

template <typename ST, int W>
int launch_bwd(const float *coef, void *gx, const BcShape &s, const BcPlan &p, hipStream_t st) {
    const long long blocks = s.outer * p.nslabs * p.col_tiles;
    if (blocks > 0x7fffffffLL) return NRT_ERR_UNSUPPORTED;
    if (s.inner == 1)
        hipLaunchKernelGGL((bc_bwd_trail<ST, W>), dim3((unsigned)blocks), dim3(kThreads), 0, st, coef, gx, s.P, p, (int)s.R);
    else
        hipLaunchKernelGGL((bc_bwd_inner<ST, W>), dim3((unsigned)blocks), dim3(kThreads), 0, st, coef, gx, s.P, p, (int)s.R, (int)s.inner);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

// the 16-byte forms where the tensor allows them: aligned base and, in the inner arm, rows that are whole groups
inline bool use_vec(const void *p, int dtype, long long inner) {
    return aligned16(p) && (inner == 1 || inner % vec_width(dtype) == 0);
}

}  // namespace

// What nrt_barycenter and nrt_barycenter_bwd of this shape need at most, whichever of the 16-byte and per-element forms the pointers of
// the call select; 0 for a shape the calls refuse.
extern "C" size_t nrt_barycenter_workspace_bytes(int dtype, long long outer, const int *red_shape, int k, long long inner) {
    BcShape s;
    if (check_shape(dtype, outer, red_shape, k, inner, 0, 0, s) != NRT_OK) return 0;
    return std::max(std::max(part_bytes(s, 1), part_bytes(s, vec_width(dtype))), coef_bytes(s));
}

extern "C" int nrt_barycenter(const void *x, int dtype, long long outer, const int *red_shape, int k, long long inner, int normalize,
                              int shift_center, float *y, float *sums, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !y || !sums) return NRT_ERR_INVALID_ARG;
    BcShape s;
    int rc = check_shape(dtype, outer, red_shape, k, inner, normalize, shift_center, s);
    if (rc != NRT_OK) return rc;
    const bool vec = use_vec(x, dtype, inner);
    const int w = vec ? vec_width(dtype) : 1;
    const BcPlan p = make_plan(s.outer, s.R, s.inner, w);
    if (!workspace || workspace_bytes < part_bytes(s, w)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    float *part = (float *)workspace;
    switch (dtype) {
        case NRT_DT_F32: rc = vec ? launch_fwd<float, 4>(x, part, s, p, st) : launch_fwd<float, 1>(x, part, s, p, st); break;
        case NRT_DT_BF16: rc = vec ? launch_fwd<Bf16, 8>(x, part, s, p, st) : launch_fwd<Bf16, 1>(x, part, s, p, st); break;
        default: rc = vec ? launch_fwd<_Float16, 8>(x, part, s, p, st) : launch_fwd<_Float16, 1>(x, part, s, p, st); break;
    }
    if (rc != NRT_OK) return rc;
    const int cl = pow2_at_least(inner, 16), nrun = pow2_at_least(p.nslabs, kThreads / cl);
    const long long col_tiles = (inner + cl - 1) / cl, per_block = kThreads / (cl * nrun);
    const long long blocks = col_tiles * ((outer + per_block - 1) / per_block);
    if (blocks > 0x7fffffffLL) return NRT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(bc_finish, dim3((unsigned)blocks), dim3(kThreads), 0, st, (const float *)part, y, sums, k, outer, (int)inner,
                       p.nslabs, cl, nrun, (unsigned)col_tiles);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_barycenter_bwd(const float *gy, const float *y, const float *sums, int dtype, long long outer, const int *red_shape,
                                  int k, long long inner, int normalize, int shift_center, void *gx, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!gy || !y || !sums || !gx) return NRT_ERR_INVALID_ARG;
    BcShape s;
    int rc = check_shape(dtype, outer, red_shape, k, inner, normalize, shift_center, s);
    if (rc != NRT_OK) return rc;
    if (!workspace || workspace_bytes < coef_bytes(s)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    float *coef = (float *)workspace;
    const long long n = outer * inner;
    hipLaunchKernelGGL(bc_bwd_coef, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, gy, y, sums, coef, k, outer,
                       (int)inner);
    NRT_CHECK_LAUNCH();
    const bool vec = use_vec(gx, dtype, inner);
    const BcPlan p = make_plan(s.outer, s.R, s.inner, vec ? vec_width(dtype) : 1);
    switch (dtype) {
        case NRT_DT_F32: return vec ? launch_bwd<float, 4>(coef, gx, s, p, st) : launch_bwd<float, 1>(coef, gx, s, p, st);
        case NRT_DT_BF16: return vec ? launch_bwd<Bf16, 8>(coef, gx, s, p, st) : launch_bwd<Bf16, 1>(coef, gx, s, p, st);
        default: return vec ? launch_bwd<_Float16, 8>(coef, gx, s, p, st) : launch_bwd<_Float16, 1>(coef, gx, s, p, st);
    }
}
