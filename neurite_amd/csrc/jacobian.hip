// The Jacobian determinant of a displacement field (vxm.py.utils.jacobian_determinant, restated: voxelmorph is not in the reference
// tree), the statistics a validation loop takes from it, the folding penalty mean(max(0, -det)), and the gradient with
// respect to the field.  float32, channels-last disp [B, *S, nd], nd = len(S) in {2, 3}, 'ij' coordinates.
//
// The stencil is np.gradient's.  Along spatial axis a of extent n, at index i: lo = max(i - 1, 0), hi = min(i + 1, n - 1),
//     G[a][c] = (disp[hi][c] - disp[lo][c]) * s,   s = 1/2 where lo and hi are both neighbours (interior), 1 at i = 0 and i = n - 1
// (one subtraction and an exact scaling), J[a][c] = G[a][c] + (a == c) (the grid's own derivative is exactly the identity), and
//     3-D  det = J0[0] (J1[1] J2[2] - J1[2] J2[1]) - J0[1] (J1[0] J2[2] - J1[2] J2[0]) + J0[2] (J1[0] J2[1] - J1[1] J2[0])
//     2-D  det = J0[0] J1[1] - J1[0] J0[1]
// one rounding per operation, in the order written (the library is built with -ffp-contract=off).
//
// Structure.  Both directions are plain gathers with one thread per voxel: a voxel is 12 (8) bytes and the 6 (4) neighbours of the
// forward all lie within one plane of it, so everything after the first touch of a line is served by the caches.  A block owns a
// contiguous run of voxels of ONE batch entry; logical blocks are renumbered so that consecutive runs stay on one XCD (one L2), which
// keeps the planes above and below a run in the cache that asks for them.  No LDS tile: see DESIGN 4.6i for why the ring of planes
// that csrc/vxmloss.hip uses for its box sums was not taken.
//   jacdet_fwd     writes det and / or leaves one row of partials per block: the count of det <= 0, min, max and the float64 sums of
//                  det, det^2 and max(0, -det) over the block's run (threads add in float64; lanes by xor shuffles, waves in wave order).
//   jacdet_finish  one block per batch entry adds the rows in block order in float64: the stats row, and loss = float32(sum / V).
//   jacdet_bwd     gdisp[q][c] = sum_a sum_p coef_a(p, q) w[p] cof[p][a][c].  The p that reach q along axis a are always two: q - e_a
//                  (+) or, at i = 0, q itself (-); and q + e_a (-) or, at i = n - 1, q itself (+); coef = s(p).  cof[p][a] is the
//                  cross product of the two other rows of J at p (2-D: the rotated other row), rebuilt from disp.  w[p] = gdet[p], or the
//                  indicator [det[p] < 0] (det as the forward computes it, bit for bit) whose sum is scaled by -gloss[b] / V in float64
//                  at the end: the indicator sums are short sums of cofactors, exact on integer fields.
// No atomics, no host synchronisation, no memset; every sum has a fixed partition and order given the shapes: run-to-run bit-identical.
// Partials travel as the two 32-bit halves of a float64, so the workspace needs 4-byte alignment only.
#include "wave_ops.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kRunVoxels = 2048;                     // voxels of a block's run, at least (8 per thread)
constexpr int kMaxRuns = 2048;                       // runs per batch entry, at most
constexpr int kPartWords = 9;                        // count, min, max, and three float64 as (hi, lo) words

struct JacGeom {
    int B, nd;
    int n[3];                                        // the nd extents, outermost first
    int V;                                           // voxels of a batch entry
    int nb, per;                                     // runs per batch entry, voxels per run
};

__device__ __forceinline__ void store_f64(unsigned *p, double s) {
    p[0] = (unsigned)__double2hiint(s);
    p[1] = (unsigned)__double2loint(s);
}
__device__ __forceinline__ double load_f64(const unsigned *p) { return __hiloint2double((int)p[0], (int)p[1]); }

// the coordinates of voxel v of a batch entry and the voxel strides of the axes
template <int ND> struct JacPos { int i[ND]; };
template <int ND> __device__ __forceinline__ JacPos<ND> jac_pos(int v, const JacGeom &g) {
    JacPos<ND> p;
#pragma unroll
    for (int a = ND - 1; a > 0; --a) {
        const int q = v / g.n[a];
        p.i[a] = v - q * g.n[a];
        v = q;
    }
    p.i[0] = v;
    return p;
}
template <int ND> __device__ __forceinline__ int jac_stride(int a, const JacGeom &g) {
    int s = 1;
#pragma unroll
    for (int k = ND - 1; k > a; --k) s *= g.n[k];
    return s;
}

// row a of J at voxel v (index i along axis a, extent n >= 2, voxel stride st); f is the batch entry
template <int ND>
__device__ __forceinline__ void jac_row(const float *__restrict__ f, int v, int a, int i, int n, int st, float (&J)[ND]) {
    const bool has_lo = i > 0, has_hi = i + 1 < n;
    const float s = has_lo && has_hi ? 0.5f : 1.0f;
    const float *ph = f + (long long)(has_hi ? v + st : v) * ND, *pl = f + (long long)(has_lo ? v - st : v) * ND;
#pragma unroll
    for (int c = 0; c < ND; ++c) J[c] = nrt_mul(nrt_sub(ph[c], pl[c]), s);
#pragma unroll
    for (int c = 0; c < ND; ++c)
        if (c == a) J[c] = nrt_add(J[c], 1.0f);
}

__device__ __forceinline__ float jac_det(const float (&J)[3][3]) {
    const float m0 = nrt_sub(nrt_mul(J[1][1], J[2][2]), nrt_mul(J[1][2], J[2][1]));
    const float m1 = nrt_sub(nrt_mul(J[1][0], J[2][2]), nrt_mul(J[1][2], J[2][0]));
    const float m2 = nrt_sub(nrt_mul(J[1][0], J[2][1]), nrt_mul(J[1][1], J[2][0]));
    return nrt_add(nrt_sub(nrt_mul(J[0][0], m0), nrt_mul(J[0][1], m1)), nrt_mul(J[0][2], m2));
}
__device__ __forceinline__ float jac_det(const float (&J)[2][2]) { return nrt_sub(nrt_mul(J[0][0], J[1][1]), nrt_mul(J[1][0], J[0][1])); }

// d det / d J[a][.]: the cross product of the two rows that follow a cyclically (3-D), the other row turned by a quarter (2-D)
template <int A> __device__ __forceinline__ void jac_cof(const float (&J)[3][3], float (&c)[3]) {
    constexpr int r = (A + 1) % 3, s = (A + 2) % 3;
    c[0] = nrt_sub(nrt_mul(J[r][1], J[s][2]), nrt_mul(J[r][2], J[s][1]));
    c[1] = nrt_sub(nrt_mul(J[r][2], J[s][0]), nrt_mul(J[r][0], J[s][2]));
    c[2] = nrt_sub(nrt_mul(J[r][0], J[s][1]), nrt_mul(J[r][1], J[s][0]));
}
template <int A> __device__ __forceinline__ void jac_cof(const float (&J)[2][2], float (&c)[2]) {
    if (A == 0) { c[0] = J[1][1]; c[1] = -J[1][0]; }
    else { c[0] = -J[0][1]; c[1] = J[0][0]; }
}

// the run of logical block `lb`: batch entry, first voxel, one past the last
__device__ __forceinline__ void jac_run(unsigned lb, const JacGeom &g, int &b, int &beg, int &end) {
    b = (int)(lb / (unsigned)g.nb);
    beg = (int)(lb % (unsigned)g.nb) * g.per;        // (nb - 1) * per < V
    end = (int)min((unsigned)g.V, (unsigned)beg + (unsigned)g.per);              // (V <= 2^30: nd >= 2 elements per voxel)
}

// grid = nrt_xcd_grid(B * nb); part [B * nb][kPartWords]
template <int ND>
__global__ void __launch_bounds__(kThreads)
jacdet_fwd(const float *__restrict__ disp, JacGeom g, float *__restrict__ det, unsigned *__restrict__ part) {
    __shared__ double red[kWaves];
    __shared__ float redf[kWaves];
    const unsigned lb = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (lb >= (unsigned)g.B * (unsigned)g.nb) return;
    int b, beg, end;
    jac_run(lb, g, b, beg, end);
    const float *f = disp + (long long)b * g.V * ND;
    int st[ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) st[a] = jac_stride<ND>(a, g);
    int cnt = 0;
    float mn = INFINITY, mx = -INFINITY;
    double s = 0.0, ss = 0.0, ls = 0.0;
    for (int v = beg + (int)threadIdx.x; v < end; v += kThreads) {
        const JacPos<ND> p = jac_pos<ND>(v, g);
        float J[ND][ND];
#pragma unroll
        for (int a = 0; a < ND; ++a) jac_row<ND>(f, v, a, p.i[a], g.n[a], st[a], J[a]);
        const float d = jac_det(J);
        if (det) det[(long long)b * g.V + v] = d;
        cnt += d <= 0.0f ? 1 : 0;
        mn = fminf(mn, d);
        mx = fmaxf(mx, d);
        s += (double)d;
        ss += (double)d * (double)d;
        ls += (double)fmaxf(0.0f, -d);
    }
    if (!part) return;
    const double c = nrt_block_sum<kWaves>((double)cnt, red);                                // (an integer below 2^31: exact)
    const float lo = nrt_block_reduce<kWaves>(mn, redf, nrt_op_min()), hi = nrt_block_reduce<kWaves>(mx, redf, nrt_op_max());
    const double ts = nrt_block_sum<kWaves>(s, red), tss = nrt_block_sum<kWaves>(ss, red), tls = nrt_block_sum<kWaves>(ls, red);
    if (threadIdx.x == 0) {
        unsigned *row = part + (size_t)lb * kPartWords;
        row[0] = (unsigned)(int)c;
        row[1] = __float_as_uint(lo);
        row[2] = __float_as_uint(hi);
        store_f64(row + 3, ts);
        store_f64(row + 5, tss);
        store_f64(row + 7, tls);
    }
}

// grid = B.  stats [B][5] of 8 bytes: the count as int64, then min, max, sum det, sum det^2 as float64; loss [B]
__global__ void __launch_bounds__(kThreads)
jacdet_finish(const unsigned *__restrict__ part, JacGeom g, void *__restrict__ stats, float *__restrict__ loss) {
    __shared__ double red[kWaves];
    __shared__ float redf[kWaves];
    const unsigned *p = part + (size_t)blockIdx.x * g.nb * kPartWords;
    double c = 0.0, s = 0.0, ss = 0.0, ls = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = threadIdx.x; k < g.nb; k += kThreads) {
        const unsigned *row = p + (size_t)k * kPartWords;
        c += (double)(int)row[0];
        mn = fminf(mn, __uint_as_float(row[1]));
        mx = fmaxf(mx, __uint_as_float(row[2]));
        s += load_f64(row + 3);
        ss += load_f64(row + 5);
        ls += load_f64(row + 7);
    }
    const double tc = nrt_block_sum<kWaves>(c, red);
    const float lo = nrt_block_reduce<kWaves>(mn, redf, nrt_op_min()), hi = nrt_block_reduce<kWaves>(mx, redf, nrt_op_max());
    const double ts = nrt_block_sum<kWaves>(s, red), tss = nrt_block_sum<kWaves>(ss, red), tls = nrt_block_sum<kWaves>(ls, red);
    if (threadIdx.x != 0) return;
    if (stats) {
        long long *ci = (long long *)stats + 5LL * blockIdx.x;
        double *cd = (double *)stats + 5LL * blockIdx.x;
        ci[0] = (long long)tc;
        cd[1] = (double)lo;
        cd[2] = (double)hi;
        cd[3] = ts;
        cd[4] = tss;
    }
    if (loss) loss[blockIdx.x] = (float)(tls / (double)g.V);
}

// what voxel p (q moved by `dv` voxels along axis A, index ip there) sends to q: sign * s(p) * w[p] * cof[p][A][.]
template <int ND, int A>
__device__ __forceinline__ void jac_send(const float *__restrict__ f, const float *__restrict__ gd, bool want_loss, const JacGeom &g,
                                         const int (&st)[ND], const JacPos<ND> &q, int vq, int ip, float sign, float (&acc)[ND],
                                         float (&accl)[ND]) {
    const int vp = vq + (ip - q.i[A]) * st[A];
    const float coef = (ip > 0 && ip + 1 < g.n[A]) ? 0.5f * sign : sign;
    float J[ND][ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) {
        if (a != A || want_loss) jac_row<ND>(f, vp, a, a == A ? ip : q.i[a], g.n[a], st[a], J[a]);
        else {
#pragma unroll
            for (int c = 0; c < ND; ++c) J[a][c] = 0.0f;                         // (row A is not part of its own cofactors)
        }
    }
    float cof[ND];
    jac_cof<A>(J, cof);
    if (gd) {
        const float w = gd[vp] * coef;
#pragma unroll
        for (int c = 0; c < ND; ++c) acc[c] += w * cof[c];
    }
    if (want_loss && jac_det(J) < 0.0f) {
#pragma unroll
        for (int c = 0; c < ND; ++c) accl[c] += coef * cof[c];
    }
}

template <int ND, int A>
__device__ __forceinline__ void jac_gather_axis(const float *__restrict__ f, const float *__restrict__ gd, bool want_loss,
                                                const JacGeom &g, const int (&st)[ND], const JacPos<ND> &q, int vq, float (&acc)[ND],
                                                float (&accl)[ND]) {
    const int i = q.i[A], n = g.n[A];
    // q is the `hi` of q - e_A (and of itself at the far end), the `lo` of q + e_A (and of itself at the near end)
    if (i > 0) jac_send<ND, A>(f, gd, want_loss, g, st, q, vq, i - 1, 1.0f, acc, accl);
    else jac_send<ND, A>(f, gd, want_loss, g, st, q, vq, i, -1.0f, acc, accl);
    if (i + 1 < n) jac_send<ND, A>(f, gd, want_loss, g, st, q, vq, i + 1, -1.0f, acc, accl);
    else jac_send<ND, A>(f, gd, want_loss, g, st, q, vq, i, 1.0f, acc, accl);
}

// grid = nrt_xcd_grid(B * nb)
template <int ND>
__global__ void __launch_bounds__(kThreads)
jacdet_bwd(const float *__restrict__ disp, const float *__restrict__ gdet, const float *__restrict__ gloss, JacGeom g,
           float *__restrict__ gdisp) {
    const unsigned lb = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (lb >= (unsigned)g.B * (unsigned)g.nb) return;
    int b, beg, end;
    jac_run(lb, g, b, beg, end);
    const float *f = disp + (long long)b * g.V * ND;
    const float *gd = gdet ? gdet + (long long)b * g.V : nullptr;
    float *out = gdisp + (long long)b * g.V * ND;
    const bool want_loss = gloss != nullptr;
    const double lscale = want_loss ? -(double)gloss[b] / (double)g.V : 0.0;
    int st[ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) st[a] = jac_stride<ND>(a, g);
    for (int v = beg + (int)threadIdx.x; v < end; v += kThreads) {
        const JacPos<ND> q = jac_pos<ND>(v, g);
        float acc[ND], accl[ND];
#pragma unroll
        for (int c = 0; c < ND; ++c) acc[c] = accl[c] = 0.0f;
        jac_gather_axis<ND, 0>(f, gd, want_loss, g, st, q, v, acc, accl);
        jac_gather_axis<ND, 1>(f, gd, want_loss, g, st, q, v, acc, accl);
        if constexpr (ND == 3) jac_gather_axis<ND, 2>(f, gd, want_loss, g, st, q, v, acc, accl);
#pragma unroll
        for (int c = 0; c < ND; ++c) {
            float r = acc[c];
            if (want_loss) {
                const float l = (float)((double)accl[c] * lscale);
                r = gd ? r + l : l;
            }
            out[(long long)v * ND + c] = r;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int jac_geom(int batch, const int *shape, int nd, JacGeom &g) {
    if (!shape || batch < 1) return NRT_ERR_INVALID_ARG;
    if (nd != 2 && nd != 3) return NRT_ERR_UNSUPPORTED;
    long long V = 1;
    for (int a = 0; a < nd; ++a) {
        if (shape[a] < 2) return NRT_ERR_INVALID_ARG;                            // (np.gradient refuses an extent below 2)
        V *= shape[a];                                                           // (stepwise: no product leaves 64 bits)
        if (V >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    }
    if (batch > 65535 || V * batch >= (1LL << 31) || V * batch * nd >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    g.B = batch;
    g.nd = nd;
    for (int a = 0; a < 3; ++a) g.n[a] = a < nd ? shape[a] : 1;
    g.V = (int)V;
    const long long nb = std::max(1LL, std::min((V + kRunVoxels - 1) / kRunVoxels, (long long)kMaxRuns));
    g.per = (int)((V + nb - 1) / nb);
    g.nb = (int)((V + g.per - 1) / g.per);
    return NRT_OK;
}
inline size_t jac_part_bytes(const JacGeom &g) { return (size_t)g.B * g.nb * kPartWords * sizeof(unsigned); }

}  // namespace

// What nrt_jacdet_f32 of this geometry needs for `stats` or `loss`; 0 for a geometry the calls refuse.
extern "C" size_t nrt_jacdet_workspace_bytes(int batch, const int *shape, int nd) {
    JacGeom g;
    if (jac_geom(batch, shape, nd, g) != NRT_OK) return 0;
    return jac_part_bytes(g);
}

extern "C" int nrt_jacdet_f32(const float *disp, int batch, const int *shape, int nd, float *det, void *stats, float *loss,
                              void *workspace, size_t workspace_bytes, void *stream) {
    if (!disp || (!det && !stats && !loss)) return NRT_ERR_INVALID_ARG;
    if (((uintptr_t)stats & 7) != 0) return NRT_ERR_INVALID_ARG;
    JacGeom g;
    const int rc = jac_geom(batch, shape, nd, g);
    if (rc != NRT_OK) return rc;
    const bool reduce = stats || loss;
    if (reduce && (!workspace || workspace_bytes < jac_part_bytes(g))) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    unsigned *part = reduce ? (unsigned *)workspace : nullptr;
    const dim3 grid(nrt_xcd_grid((unsigned)(g.B * g.nb)));
    if (nd == 3) hipLaunchKernelGGL(jacdet_fwd<3>, grid, dim3(kThreads), 0, st, disp, g, det, part);
    else hipLaunchKernelGGL(jacdet_fwd<2>, grid, dim3(kThreads), 0, st, disp, g, det, part);
    NRT_CHECK_LAUNCH();
    if (!reduce) return NRT_OK;
    hipLaunchKernelGGL(jacdet_finish, dim3((unsigned)g.B), dim3(kThreads), 0, st, (const unsigned *)part, g, stats, loss);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_jacdet_bwd_f32(const float *disp, const float *gdet, const float *gloss, int batch, const int *shape, int nd,
                                  float *gdisp, void *stream) {
    if (!disp || (!gdet && !gloss) || !gdisp) return NRT_ERR_INVALID_ARG;
    JacGeom g;
    const int rc = jac_geom(batch, shape, nd, g);
    if (rc != NRT_OK) return rc;
    const dim3 grid(nrt_xcd_grid((unsigned)(g.B * g.nb)));
    if (nd == 3) hipLaunchKernelGGL(jacdet_bwd<3>, grid, dim3(kThreads), 0, nrt_stream(stream), disp, gdet, gloss, g, gdisp);
    else hipLaunchKernelGGL(jacdet_bwd<2>, grid, dim3(kThreads), 0, nrt_stream(stream), disp, gdet, gloss, g, gdisp);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
