// The two losses an unsupervised VoxelMorph registration run optimises: the windowed normalised cross-correlation of two images
// (vxm.losses.NCC) and the smoothness penalty on a displacement field (vxm.losses.Grad), each with its gradient.  float32,
// channels-last [B, *S, C]; spatial ranks below 3 arrive with leading extents of 1.  voxelmorph is not in the reference tree: the
// semantics are restated in DESIGN 8, not pinned.
//
// NCC.  n = prod(win) C.  The five box sums S_I, S_J, S_II, S_JJ, S_IJ of I, J, I I, J J, I J run over the window and over all channels,
// zero padded as TensorFlow's 'SAME' pads ((w - 1) / 2 zeros in front).  One kernel, ncc_box, does every box sum of the file:
//     a block owns a kTY x kTZ tile of the two inner spatial axes plus its halo and marches along the outer axis through one chunk of
//     kXChunk output planes.  Per input plane: (A) the threads load the halo points of I and J, looping over channels, and leave the
//     five products in LDS; (B) box sum along z; (C) box sum along y, into slot (plane % win_x) of a ring of the last win_x plane sums
//     of every output (LDS, [slot][field][thread]: a thread only ever touches its own column, conflict free); then the output plane
//     that the new input plane completes is the sum of the ring, slot by slot.  No running add-and-subtract anywhere: every window
//     sum is a plain sum of its terms (exact on small-integer images; error within the order-free bound otherwise).
//   epilogue kFwd    uI = S_I / n, uJ = S_J / n, cross = max(((S_IJ - uJ S_I) - uI S_J) + (uI uJ) n, eps),
//                    Ivar = max((S_II - (2 uI) S_I) + (uI uI) n, eps), Jvar likewise, cc = (cross / Ivar) (cross / Jvar): one rounding
//                    per operation, IEEE division.  Writes the sums and / or cc, and adds cc into a per-block partial; ncc_finish
//                    adds the partials of a batch entry in block order (float64) and forms -mean.
//   epilogue kCoef   (backward, first launch) the same sums; with g the upstream gradient of cc (gcc, or -gloss[b] / V, or their sum)
//                    it leaves five coefficient fields per voxel in the workspace:
//                        A  = c0 >= eps  ?  2 cross / (Ivar Jvar) g : 0          (c0, vI0, vJ0: the values before the max)
//                        BJ = vJ0 >= eps ? -2 cross^2 / (Ivar Jvar^2) g : 0      BI = vI0 >= eps ? -2 cross^2 / (Ivar^2 Jvar) g : 0
//                        KJ = A uI + BJ uJ                                       KI = A uJ + BI uI
//   epilogue kComb   (backward, second launch) the same kernel box-sums those five fields with the MIRRORED padding (w - 1 - (w - 1) / 2
//                    zeros in front: the transpose of the forward window, different for even windows) and combines, for every channel c
//                    of voxel q:  gI = J_qc W(A) + I_qc W(BI) - W(KI),   gJ = I_qc W(A) + J_qc W(BJ) - W(KJ).
//                    (W is linear, so W(A uI) + W(BJ uJ) = W(KJ): five fields instead of seven.)
// Nothing of the forward is kept for the backward but I and J.
//
// Grad.  d_i = y[.., 1:, ..] - y[.., :-1, ..] along each spatial axis i, m_i = mean over everything but the batch of |d_i| ('l1') or d_i^2
// ('l2'), loss = ((m_0 + m_1) + m_2) / ndims * loss_mult.  grad_fwd streams y once by rows (a row = one line along the innermost axis with
// its channels), each element reads its successor along each axis; per-block partials per (batch, axis), grad_finish adds them in block
// order (float64) and applies the operation order above in float32.  grad_bwd writes gy_q = sum_i s_i (phi(y_q - y_{q - e_i}) -
// phi(y_{q + e_i} - y_q)), phi = sign ('l1', sign(0) = 0) or 2 d ('l2'), s_i = gloss[b] loss_mult / (ndims count_i), in one pass.  16-byte
// accesses where channels % 4 == 0 and the pointers allow; per element otherwise.
//
// No atomics, no host synchronisation (every call captures into a graph); all sums have a fixed partition and order: run-to-run
// bit-identical.  Partials travel as (hi, lo) float pairs (a float64 sum to 48 bits), so the workspace needs 4-byte alignment only.
#include "wave_ops.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kTY = 8, kTZ = 32;                     // outputs of a block per plane: one per thread
constexpr int kXChunk = 32;                          // output planes a block marches through
constexpr int kMaxWin = 15, kMaxC = 16, kFields = 5;
constexpr int kMaxPts = ((kTY + kMaxWin - 1) * (kTZ + kMaxWin - 1) + kThreads - 1) / kThreads;      // halo points per thread: 4
constexpr int kGradBlocks = 256;                     // first-stage blocks per batch entry of the Grad loss, at most
constexpr int kFwd = 0, kCoef = 1, kComb = 2;

static_assert(kTY * kTZ == kThreads, "one output per thread and plane");

struct NccGeom {
    int B, X, Y, Z, C;
    int wx, wy, wz;
    int px, py, pz;                                  // zeros in front of each axis
    int HY, HZ;                                      // the tile with its halo
    int nxc, nty, ntz;                               // chunks of x, tiles of y and z
    float n, eps;
    long long V;
};

struct NccIO {
    float *sums, *cc, *part;                         // kFwd (each may be NULL)
    const float *gcc, *gloss;                        // kCoef (either may be NULL)
    float *coef;                                     // kCoef writes, kComb reads: [B, V, 5]
    float *gI, *gJ;                                  // kComb (either may be NULL)
};

__device__ __forceinline__ void split_store(float *p, double s) {
    const float hi = (float)s;
    p[0] = hi;
    p[1] = (float)(s - (double)hi);
}
__device__ __forceinline__ double split_load(const float *p) { return (double)p[0] + (double)p[1]; }

// the epilogue's arithmetic, one rounding per operation (the library is built with -ffp-contract=off; the helpers say so again)
struct NccStats { float uI, uJ, c0, vI0, vJ0, cross, Ivar, Jvar; };
__device__ __forceinline__ NccStats ncc_stats(const float (&S)[kFields], float n, float eps) {
    NccStats t;
    t.uI = S[0] / n;
    t.uJ = S[1] / n;
    t.c0 = nrt_add(nrt_sub(nrt_sub(S[4], nrt_mul(t.uJ, S[0])), nrt_mul(t.uI, S[1])), nrt_mul(nrt_mul(t.uI, t.uJ), n));
    t.vI0 = nrt_add(nrt_sub(S[2], nrt_mul(nrt_mul(2.0f, t.uI), S[0])), nrt_mul(nrt_mul(t.uI, t.uI), n));
    t.vJ0 = nrt_add(nrt_sub(S[3], nrt_mul(nrt_mul(2.0f, t.uJ), S[1])), nrt_mul(nrt_mul(t.uJ, t.uJ), n));
    t.cross = fmaxf(t.c0, eps);
    t.Ivar = fmaxf(t.vI0, eps);
    t.Jvar = fmaxf(t.vJ0, eps);
    return t;
}

// grid = B * nxc * nty * ntz; dynamic LDS = (5 HY HZ + 5 HY kTZ + 5 wx 256) floats.  ONEC: one channel (its own instantiation: with both
// load paths in one kernel the scalar registers spill)
template <int MODE, bool ONEC>
__global__ void __launch_bounds__(kThreads)
ncc_box(const float *__restrict__ I, const float *__restrict__ J, NccGeom g, NccIO io) {
    extern __shared__ float ncc_lds[];
    __shared__ double red[kThreads / NRT_WAVE];
    const int npts = g.HY * g.HZ, nzo = g.HY * kTZ;
    float *P = ncc_lds;                              // [5][HY][HZ]   products of the halo points of one plane
    float *Q = P + kFields * npts;                   // [5][HY][kTZ]  summed along z
    float *ring = Q + kFields * nzo;                 // [wx][5][256]  summed along z and y: the last wx planes
    const int tid = threadIdx.x;
    unsigned bid = blockIdx.x;
    const int tz = bid % g.ntz; bid /= g.ntz;
    const int ty = bid % g.nty; bid /= g.nty;
    const int xc = bid % g.nxc;
    const int b = bid / g.nxc;
    const int x0 = xc * kXChunk, x1 = min(g.X, x0 + kXChunk);
    const int y0 = ty * kTY, z0 = tz * kTZ;
    const long long plane = (long long)g.Y * g.Z;    // voxels of a plane

    // the halo points this thread loads, the same in every plane: the voxel's offset in its plane, -1 for a point in the zero padding,
    // -2 for no point
    int pvox[kMaxPts];
#pragma unroll
    for (int j = 0; j < kMaxPts; ++j) {
        const int idx = tid + j * kThreads;
        pvox[j] = -2;
        if (idx < npts) {
            const int hy = idx / g.HZ, hz = idx - hy * g.HZ;
            const int y = y0 - g.py + hy, z = z0 - g.pz + hz;
            pvox[j] = (y >= 0 && y < g.Y && z >= 0 && z < g.Z) ? y * g.Z + z : -1;
        }
    }
    const int oy = tid / kTZ, oz = tid % kTZ;
    const int yo = y0 + oy, zo = z0 + oz;
    const bool live = yo < g.Y && zo < g.Z;
    float acc = 0.0f;

    const int xin0 = x0 - g.px, steps = (x1 - x0) + g.wx - 1;
    for (int step = 0; step < steps; ++step) {
        const int xin = xin0 + step, slot = step % g.wx;
        float *mine = ring + slot * (kFields * kThreads) + tid;
        if (xin >= 0 && xin < g.X) {                                            // (the same for the whole block)
            const long long vbase = ((long long)b * g.X + xin) * plane;
            // (A) the five fields of the halo points
            if (MODE == kComb) {
                float v[kMaxPts][kFields];
#pragma unroll
                for (int j = 0; j < kMaxPts; ++j) {
#pragma unroll
                    for (int f = 0; f < kFields; ++f) v[j][f] = pvox[j] >= 0 ? io.coef[(vbase + pvox[j]) * kFields + f] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < kMaxPts; ++j) {
                    if (pvox[j] != -2) {
#pragma unroll
                        for (int f = 0; f < kFields; ++f) P[f * npts + tid + j * kThreads] = v[j][f];
                    }
                }
            } else if (ONEC) {
                float a[kMaxPts], c[kMaxPts];
#pragma unroll
                for (int j = 0; j < kMaxPts; ++j) {
                    a[j] = pvox[j] >= 0 ? I[vbase + pvox[j]] : 0.0f;
                    c[j] = pvox[j] >= 0 ? J[vbase + pvox[j]] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < kMaxPts; ++j) {
                    if (pvox[j] != -2) {
                        float *p = P + tid + j * kThreads;
                        p[0] = a[j];
                        p[npts] = c[j];
                        p[2 * npts] = nrt_mul(a[j], a[j]);
                        p[3 * npts] = nrt_mul(c[j], c[j]);
                        p[4 * npts] = nrt_mul(a[j], c[j]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kMaxPts; ++j) {
                    if (pvox[j] != -2) {
                        float s[kFields] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                        if (pvox[j] >= 0) {
                            const float *pi = I + (vbase + pvox[j]) * g.C, *pj = J + (vbase + pvox[j]) * g.C;
                            for (int ch = 0; ch < g.C; ++ch) {
                                const float a = pi[ch], c = pj[ch];
                                s[0] = nrt_add(s[0], a);
                                s[1] = nrt_add(s[1], c);
                                s[2] = nrt_add(s[2], nrt_mul(a, a));
                                s[3] = nrt_add(s[3], nrt_mul(c, c));
                                s[4] = nrt_add(s[4], nrt_mul(a, c));
                            }
                        }
#pragma unroll
                        for (int f = 0; f < kFields; ++f) P[f * npts + tid + j * kThreads] = s[f];
                    }
                }
            }
            __syncthreads();
            // (B) along z
#pragma unroll 1
            for (int idx = tid; idx < nzo; idx += kThreads) {
                {
                    const float *p = P + (idx / kTZ) * g.HZ + (idx % kTZ);
                    float s[kFields] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    for (int k = 0; k < g.wz; ++k) {
#pragma unroll
                        for (int f = 0; f < kFields; ++f) s[f] = nrt_add(s[f], p[f * npts + k]);
                    }
#pragma unroll
                    for (int f = 0; f < kFields; ++f) Q[f * nzo + idx] = s[f];
                }
            }
            __syncthreads();
            // (C) along y, into the ring.  (The next plane's (A) writes P, which nobody reads here; its (B) writes Q behind (A)'s barrier.)
            {
                const float *q = Q + oy * kTZ + oz;
                float s[kFields] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = 0; k < g.wy; ++k) {
#pragma unroll
                    for (int f = 0; f < kFields; ++f) s[f] = nrt_add(s[f], q[f * nzo + k * kTZ]);
                }
#pragma unroll
                for (int f = 0; f < kFields; ++f) mine[f * kThreads] = s[f];
            }
        } else {
#pragma unroll
            for (int f = 0; f < kFields; ++f) mine[f * kThreads] = 0.0f;          // a plane of the zero padding
        }
        if (step < g.wx - 1 || !live) continue;                                  // (a thread reads back only its own ring column)
        const int xo = x0 + step - (g.wx - 1);                                   // the output plane that plane xin completes
        float S[kFields] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < g.wx; ++k) {
#pragma unroll
            for (int f = 0; f < kFields; ++f) S[f] = nrt_add(S[f], ring[(k * kFields + f) * kThreads + tid]);
        }
        const long long v = (((long long)b * g.X + xo) * g.Y + yo) * g.Z + zo;
        if (MODE == kComb) {
            // S = W(A), W(BJ), W(BI), W(KJ), W(KI)
            for (int ch = 0; ch < g.C; ++ch) {
                const float a = I[v * g.C + ch], c = J[v * g.C + ch];
                if (io.gI) io.gI[v * g.C + ch] = c * S[0] + a * S[2] - S[4];
                if (io.gJ) io.gJ[v * g.C + ch] = a * S[0] + c * S[1] - S[3];
            }
        } else {
            const NccStats t = ncc_stats(S, g.n, g.eps);
            if (MODE == kFwd) {
                const float cc = nrt_mul(t.cross / t.Ivar, t.cross / t.Jvar);
                if (io.sums) {
#pragma unroll
                    for (int f = 0; f < kFields; ++f) io.sums[v * kFields + f] = S[f];
                }
                if (io.cc) io.cc[v] = cc;
                acc += cc;
            } else {
                float gp = io.gcc ? io.gcc[v] : 0.0f;
                if (io.gloss) gp -= io.gloss[b] / (float)g.V;
                const float r = t.cross / (t.Ivar * t.Jvar);                     // cross / (Ivar Jvar)
                const float A = t.c0 >= g.eps ? 2.0f * r * gp : 0.0f;
                const float BJ = t.vJ0 >= g.eps ? -2.0f * (t.cross * r / t.Jvar) * gp : 0.0f;
                const float BI = t.vI0 >= g.eps ? -2.0f * (t.cross * r / t.Ivar) * gp : 0.0f;
                float *o = io.coef + v * kFields;
                o[0] = A;
                o[1] = BJ;
                o[2] = BI;
                o[3] = A * t.uI + BJ * t.uJ;
                o[4] = A * t.uJ + BI * t.uI;
            }
        }
    }
    if (MODE == kFwd && io.part) {
        const double s = nrt_block_sum<kThreads / NRT_WAVE>((double)acc, red);
        if (tid == 0) split_store(io.part + 2LL * blockIdx.x, s);
    }
}

// loss[b] = -mean: the partials of batch entry b (nper of them, in block order) in float64.  grid = B
__global__ void __launch_bounds__(kThreads) ncc_finish(const float *__restrict__ part, int nper, long long V, float *__restrict__ loss) {
    __shared__ double red[kThreads / NRT_WAVE];
    const float *p = part + 2LL * blockIdx.x * nper;
    double a = 0.0;
    for (int k = threadIdx.x; k < nper; k += kThreads) a += split_load(p + 2LL * k);
    const double s = nrt_block_sum<kThreads / NRT_WAVE>(a, red);
    if (threadIdx.x == 0) loss[blockIdx.x] = -(float)(s / (double)V);
}

// ---- Grad ----------------------------------------------------------------------------------------------------------------------
struct GradGeom {
    int B, X, Y, Z, C, nd, l2;
    int L;                                           // Z * C: elements of a row
    int lanes_c;                                     // lanes along a row (a power of two); 256 / lanes_c rows in flight per block
    int nb, rows_per_block;                          // blocks per batch entry
    long long rows;                                  // X * Y
    long long cnt[3];                                // differences per batch entry along x, y, z
    float mult;
};

// W adjacent floats; W == 4 needs 16-byte alignment
template <int W> struct GradVec {
    float a[W];
    __device__ __forceinline__ float operator[](int k) const { return a[k]; }
    __device__ __forceinline__ float &operator[](int k) { return a[k]; }
};
template <int W> __device__ __forceinline__ GradVec<W> grad_load(const float *p);
template <> __device__ __forceinline__ GradVec<1> grad_load<1>(const float *p) { return GradVec<1>{{p[0]}}; }
template <> __device__ __forceinline__ GradVec<4> grad_load<4>(const float *p) {
    const nrt_f4 t = *(const nrt_f4 *)p;
    return GradVec<4>{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void grad_store(float *p, const GradVec<1> &v) { p[0] = v.a[0]; }
__device__ __forceinline__ void grad_store(float *p, const GradVec<4> &v) { *(nrt_f4 *)p = (nrt_f4){v.a[0], v.a[1], v.a[2], v.a[3]}; }

__device__ __forceinline__ float grad_phi(float d, int l2) { return l2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)); }

// grid = B * nb; part [B][nb][3] (hi, lo) pairs
template <int W>
__global__ void __launch_bounds__(kThreads) grad_fwd(const float *__restrict__ y, float *__restrict__ part, GradGeom g) {
    typedef GradVec<W> VT;
    __shared__ double red[kThreads / NRT_WAVE];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / g.nb, blk = blockIdx.x % g.nb;
    const int tc = tid & (g.lanes_c - 1), tr = tid / g.lanes_c, nrl = kThreads / g.lanes_c;
    const long long r_beg = (long long)blk * g.rows_per_block, r_end = std::min(g.rows, r_beg + g.rows_per_block);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (long long r = r_beg + tr; r < r_end; r += nrl) {
        const int x = (int)(r / g.Y), yy = (int)(r - (long long)x * g.Y);
        const float *row = y + ((long long)b * g.rows + r) * g.L;
        const bool hx = x + 1 < g.X, hy = yy + 1 < g.Y;
        for (int e = tc * W; e < g.L; e += g.lanes_c * W) {
            const bool hz = e + g.C < g.L;
            const VT v = grad_load<W>(row + e);
            VT ux = v, uy = v, uz = v;
            if (hx) ux = grad_load<W>(row + e + (long long)g.Y * g.L);
            if (hy) uy = grad_load<W>(row + e + g.L);
            if (hz) uz = grad_load<W>(row + e + g.C);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float dx = ux[k] - v[k], dy = uy[k] - v[k], dz = uz[k] - v[k];         // 0 where there is no successor
                acc[0] += g.l2 ? dx * dx : fabsf(dx);
                acc[1] += g.l2 ? dy * dy : fabsf(dy);
                acc[2] += g.l2 ? dz * dz : fabsf(dz);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double s = nrt_block_sum<kThreads / NRT_WAVE>((double)acc[d], red);
        if (tid == 0) split_store(part + 2LL * ((long long)blockIdx.x * 3 + d), s);
    }
}

// grid = B
__global__ void __launch_bounds__(kThreads) grad_finish(const float *__restrict__ part, float *__restrict__ loss, GradGeom g) {
    __shared__ double red[kThreads / NRT_WAVE];
    __shared__ double tot[3];
    const float *p = part + 2LL * blockIdx.x * g.nb * 3;
    for (int d = 0; d < 3; ++d) {
        double a = 0.0;
        for (int k = threadIdx.x; k < g.nb; k += kThreads) a += split_load(p + 2LL * (k * 3 + d));
        const double s = nrt_block_sum<kThreads / NRT_WAVE>(a, red);
        if (threadIdx.x == 0) tot[d] = s;
    }
    if (threadIdx.x != 0) return;
    float sum = 0.0f;
    for (int d = 3 - g.nd; d < 3; ++d) {
        const float m = (float)tot[d] / (float)g.cnt[d];                          // an axis of extent 1 has no differences: 0 / 0
        sum = d == 3 - g.nd ? m : nrt_add(sum, m);
    }
    loss[blockIdx.x] = nrt_mul(sum / (float)g.nd, g.mult);
}

// grid = B * nb
template <int W>
__global__ void __launch_bounds__(kThreads) grad_bwd(const float *__restrict__ y, const float *__restrict__ gloss, float *__restrict__ gy,
                                                     GradGeom g) {
    typedef GradVec<W> VT;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / g.nb, blk = blockIdx.x % g.nb;
    const int tc = tid & (g.lanes_c - 1), tr = tid / g.lanes_c, nrl = kThreads / g.lanes_c;
    const long long r_beg = (long long)blk * g.rows_per_block, r_end = std::min(g.rows, r_beg + g.rows_per_block);
    const float up = gloss[b] * g.mult;
    float s[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = g.cnt[d] > 0 ? up / ((float)g.nd * (float)g.cnt[d]) : 0.0f;
    const long long sx = (long long)g.Y * g.L;
    for (long long r = r_beg + tr; r < r_end; r += nrl) {
        const int x = (int)(r / g.Y), yy = (int)(r - (long long)x * g.Y);
        const long long base = ((long long)b * g.rows + r) * g.L;
        const float *row = y + base;
        for (int e = tc * W; e < g.L; e += g.lanes_c * W) {
            const VT v = grad_load<W>(row + e);
            VT px = v, nx = v, py = v, ny = v, pz = v, nz = v;
            if (x > 0) px = grad_load<W>(row + e - sx);
            if (x + 1 < g.X) nx = grad_load<W>(row + e + sx);
            if (yy > 0) py = grad_load<W>(row + e - g.L);
            if (yy + 1 < g.Y) ny = grad_load<W>(row + e + g.L);
            if (e >= g.C) pz = grad_load<W>(row + e - g.C);
            if (e + g.C < g.L) nz = grad_load<W>(row + e + g.C);
            VT o;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                // (a missing neighbour was given the element's own value: d = 0 and phi(0) = 0 under both penalties)
                float t = s[0] * (grad_phi(v[k] - px[k], g.l2) - grad_phi(nx[k] - v[k], g.l2));
                t += s[1] * (grad_phi(v[k] - py[k], g.l2) - grad_phi(ny[k] - v[k], g.l2));
                t += s[2] * (grad_phi(v[k] - pz[k], g.l2) - grad_phi(nz[k] - v[k], g.l2));
                o[k] = t;
            }
            grad_store(gy + base + e, o);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// argument checks shared by the NCC entry points; the padding is the forward's
inline int ncc_geom(int batch, const int *shape, int channels, const int *win, float eps, NccGeom &g) {
    if (!shape || !win || batch < 1) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < 3; ++d)
        if (shape[d] < 1) return NRT_ERR_INVALID_ARG;
    if (!(eps >= 0.0f)) return NRT_ERR_INVALID_ARG;
    if (channels < 1 || channels > kMaxC) return NRT_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d)
        if (win[d] < 1 || win[d] > kMaxWin) return NRT_ERR_UNSUPPORTED;
    long long V = (long long)shape[0] * shape[1];                                // (stepwise: no product leaves 64 bits)
    if (V >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    V *= shape[2];
    if (V >= (1LL << 31) || V * batch >= (1LL << 31) || V * batch * channels >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    g.B = batch; g.X = shape[0]; g.Y = shape[1]; g.Z = shape[2]; g.C = channels;
    g.wx = win[0]; g.wy = win[1]; g.wz = win[2];
    g.px = (g.wx - 1) / 2; g.py = (g.wy - 1) / 2; g.pz = (g.wz - 1) / 2;
    g.HY = kTY + g.wy - 1; g.HZ = kTZ + g.wz - 1;
    g.nxc = (g.X + kXChunk - 1) / kXChunk;
    g.nty = (g.Y + kTY - 1) / kTY;
    g.ntz = (g.Z + kTZ - 1) / kTZ;
    g.n = (float)(g.wx * g.wy * g.wz * g.C);
    g.eps = eps;
    g.V = V;
    if ((long long)g.B * g.nxc * g.nty * g.ntz > 0x7fffffffLL) return NRT_ERR_UNSUPPORTED;
    return NRT_OK;
}
inline long long ncc_blocks(const NccGeom &g) { return (long long)g.B * g.nxc * g.nty * g.ntz; }
inline size_t ncc_part_bytes(const NccGeom &g) { return (size_t)ncc_blocks(g) * 2 * sizeof(float); }
inline size_t ncc_coef_bytes(const NccGeom &g) { return (size_t)g.B * (size_t)g.V * kFields * sizeof(float); }
inline size_t ncc_lds_bytes(const NccGeom &g) {
    return ((size_t)kFields * g.HY * g.HZ + (size_t)kFields * g.HY * kTZ + (size_t)kFields * g.wx * kThreads) * sizeof(float);
}

template <int MODE>
int ncc_launch(const float *I, const float *J, const NccGeom &g, const NccIO &io, hipStream_t st) {
    const size_t lds = ncc_lds_bytes(g);                                         // at most 111 KB (15 x 15 x 15)
    const dim3 grid((unsigned)ncc_blocks(g));
    if (g.C == 1 || MODE == kComb) {                                             // (kComb loads five fields per point, whatever C is)
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void *)ncc_box<MODE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return NRT_ERR_LAUNCH;
        hipLaunchKernelGGL((ncc_box<MODE, true>), grid, dim3(kThreads), lds, st, I, J, g, io);
    } else if constexpr (MODE != kComb) {
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void *)ncc_box<MODE, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return NRT_ERR_LAUNCH;
        hipLaunchKernelGGL((ncc_box<MODE, false>), grid, dim3(kThreads), lds, st, I, J, g, io);
    }
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

inline int grad_geom(int batch, const int *shape, int nd, int channels, int penalty, float loss_mult, GradGeom &g) {
    if (!shape || batch < 1 || channels < 1 || nd < 1 || nd > 3 || (penalty != 1 && penalty != 2)) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < 3; ++d)
        if (shape[d] < 1 || (d < 3 - nd && shape[d] != 1)) return NRT_ERR_INVALID_ARG;
    const long long rows = (long long)shape[0] * shape[1];
    const long long L = (long long)shape[2] * channels;
    if (rows >= (1LL << 31) || L >= (1LL << 31) || rows * L >= (1LL << 31) || rows * L * batch >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    g.B = batch; g.X = shape[0]; g.Y = shape[1]; g.Z = shape[2]; g.C = channels; g.nd = nd; g.l2 = penalty == 2;
    g.L = (int)L;
    g.rows = rows;
    g.cnt[0] = (long long)(g.X - 1) * g.Y * g.L;
    g.cnt[1] = (long long)g.X * (g.Y - 1) * g.L;
    g.cnt[2] = (long long)g.X * g.Y * (g.Z - 1) * g.C;
    g.mult = loss_mult;
    return NRT_OK;
}
// the partition, which depends on the width of the accesses
inline void grad_plan(GradGeom &g, int w) {
    const int groups = g.L / w;
    int lanes = 1;
    while (lanes < kThreads && lanes < groups) lanes <<= 1;
    g.lanes_c = lanes;
    const long long nrl = kThreads / lanes;
    const long long nb = std::max(1LL, std::min((g.rows + nrl - 1) / nrl, (long long)kGradBlocks));
    g.rows_per_block = (int)((g.rows + nb - 1) / nb);
    g.nb = (int)((g.rows + g.rows_per_block - 1) / g.rows_per_block);
}
inline size_t grad_part_bytes(int batch) { return (size_t)batch * kGradBlocks * 3 * 2 * sizeof(float); }

}  // namespace

// What nrt_ncc_f32 and nrt_ncc_bwd_f32 of this geometry need at most; 0 for a geometry the calls refuse.
extern "C" size_t nrt_ncc_workspace_bytes(int batch, const int *shape, int channels, const int *win) {
    NccGeom g;
    if (ncc_geom(batch, shape, channels, win, 1e-5f, g) != NRT_OK) return 0;
    return std::max(ncc_part_bytes(g), ncc_coef_bytes(g));
}

extern "C" int nrt_ncc_f32(const float *I, const float *J, int batch, const int *shape, int channels, const int *win, float eps,
                           float *sums, float *cc, float *loss, void *workspace, size_t workspace_bytes, void *stream) {
    if (!I || !J || (!sums && !cc && !loss)) return NRT_ERR_INVALID_ARG;
    NccGeom g;
    const int rc = ncc_geom(batch, shape, channels, win, eps, g);
    if (rc != NRT_OK) return rc;
    if (loss && (!workspace || workspace_bytes < ncc_part_bytes(g))) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    NccIO io = {};
    io.sums = sums;
    io.cc = cc;
    io.part = loss ? (float *)workspace : nullptr;
    const int lrc = ncc_launch<kFwd>(I, J, g, io, st);
    if (lrc != NRT_OK || !loss) return lrc;
    hipLaunchKernelGGL(ncc_finish, dim3((unsigned)g.B), dim3(kThreads), 0, st, (const float *)io.part, g.nxc * g.nty * g.ntz, g.V, loss);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_ncc_bwd_f32(const float *I, const float *J, const float *gcc, const float *gloss, int batch, const int *shape,
                               int channels, const int *win, float eps, float *gI, float *gJ, void *workspace, size_t workspace_bytes,
                               void *stream) {
    if (!I || !J || (!gcc && !gloss) || (!gI && !gJ)) return NRT_ERR_INVALID_ARG;
    NccGeom g;
    int rc = ncc_geom(batch, shape, channels, win, eps, g);
    if (rc != NRT_OK) return rc;
    if (!workspace || workspace_bytes < ncc_coef_bytes(g)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    NccIO io = {};
    io.gcc = gcc;
    io.gloss = gloss;
    io.coef = (float *)workspace;
    rc = ncc_launch<kCoef>(I, J, g, io, st);
    if (rc != NRT_OK) return rc;
    // the transpose of the forward window: the zeros that followed now lead
    g.px = g.wx - 1 - g.px; g.py = g.wy - 1 - g.py; g.pz = g.wz - 1 - g.pz;
    io.gI = gI;
    io.gJ = gJ;
    return ncc_launch<kComb>(I, J, g, io, st);
}

extern "C" int nrt_grad_loss_f32(const float *y, int batch, const int *shape, int nd, int channels, int penalty, float loss_mult,
                                 float *loss, void *workspace, size_t workspace_bytes, void *stream) {
    if (!y || !loss) return NRT_ERR_INVALID_ARG;
    GradGeom g;
    const int rc = grad_geom(batch, shape, nd, channels, penalty, loss_mult, g);
    if (rc != NRT_OK) return rc;
    if (!workspace || workspace_bytes < grad_part_bytes(batch)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    float *part = (float *)workspace;
    const bool vec = g.C % 4 == 0 && aligned16(y);
    grad_plan(g, vec ? 4 : 1);
    const dim3 grid((unsigned)((long long)g.B * g.nb));
    if (vec) hipLaunchKernelGGL(grad_fwd<4>, grid, dim3(kThreads), 0, st, y, part, g);
    else hipLaunchKernelGGL(grad_fwd<1>, grid, dim3(kThreads), 0, st, y, part, g);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_finish, dim3((unsigned)g.B), dim3(kThreads), 0, st, (const float *)part, loss, g);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_grad_loss_bwd_f32(const float *y, const float *gloss, int batch, const int *shape, int nd, int channels, int penalty,
                                     float loss_mult, float *gy, void *stream) {
    if (!y || !gloss || !gy) return NRT_ERR_INVALID_ARG;
    GradGeom g;
    const int rc = grad_geom(batch, shape, nd, channels, penalty, loss_mult, g);
    if (rc != NRT_OK) return rc;
    const bool vec = g.C % 4 == 0 && aligned16(y) && aligned16(gy);
    grad_plan(g, vec ? 4 : 1);
    const dim3 grid((unsigned)((long long)g.B * g.nb));
    if (vec) hipLaunchKernelGGL(grad_bwd<4>, grid, dim3(kThreads), 0, nrt_stream(stream), y, gloss, gy, g);
    else hipLaunchKernelGGL(grad_bwd<1>, grid, dim3(kThreads), 0, nrt_stream(stream), y, gloss, gy, g);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
