// bfloat16 inference forms of the Conv3D stack (models.py, bf16 path) for gfx950 (MI355X).
//
// Numerics (Keras mixed_bfloat16 compute with bf16 variables): tensors are stored as bf16, every kernel computes in float32 from
// the stored values and rounds its result to bf16 ONCE, round-to-nearest-even (the hardware v_cvt_pk_bf16_f32).
//
// conv3d_bf16 -- implicit GEMM on v_mfma_f32_16x16x32_bf16 (exact bf16 products, float32 accumulation), computed as
//   D = W^T . X^T so that the output voxels sit on the MFMA column (lane & 15) and a lane owns 4 consecutive output channels of
//   one voxel: the epilogue stores 8 bytes per lane and the four 16-lane groups assemble whole channel rows.
//   Block = 4 waves = a 4(x) x 4(y) x 16(z) output tile (the tile and halo scheme of conv3d_mfma, conv.hip); wave w owns the
//   x-slab w, acc[mt][nt] = y-row mt of 16 z-voxels x 16 output channels of block nt.
//   K order (nrt_conv3d_pack_weights_bf16), two forms:
//     Cin >= 8: [8-channel group g][tap, padded to a multiple of 4][8 channels].  A k-step is 4 taps of one group; a lane's B
//               fragment is 8 consecutive channels of one tap at one voxel = one 16-byte LDS read.  The halo tile of CG groups
//               (CG = 4, 2 or 1: 32, 16 or 8 channels, the largest whose LDS fits) is staged per chunk; the packing does not
//               depend on CG.
//     Cin < 8:  dense k = tap * Cin + c, zero-padded to a multiple of 32 (the single-channel first layer: K = 27, ONE k-step);
//               a lane gathers its 8 values with scalar LDS reads through a per-block offset table.
//   Any kernel size and dilation, SAME or VALID, stride 1; nearest up-sampling + concatenate of a second source in the loader.
//   Epilogue in float32: + bias, ELU as exp(x) - 1 on the hardware exponential (as conv.hip) or ReLU, then one rounding to bf16.
// conv1x1_bf16 -- the likelihood 1x1x1 convolution with the channel softmax optionally fused, float32 arithmetic.
// maxpool3d_bf16, upsample_concat_bf16 -- exact; add_act_affine_bf16, softmax_lastdim_bf16 -- float32, one rounding.
// No atomics: every output is written by exactly one lane, so two runs give the same bits.

#include "nrt_common.h"
#include "activations.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef uint16_t bf16_t;                       // storage of one bfloat16

__device__ __forceinline__ float bf2f(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }     // RNE (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack2(float lo, float hi) { return (unsigned)f2bf(lo) | ((unsigned)f2bf(hi) << 16); }
__device__ __forceinline__ float lo_f(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_f(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ void unpack8(u32x4 v, float *f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = lo_f(v[k]); f[2 * k + 1] = hi_f(v[k]); }
}
__device__ __forceinline__ u32x4 pack8(const float *f) {
    return (u32x4){pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])};
}

struct ConvB {
    const bf16_t *src0;      // [B, X, Y, Z, c0]
    const bf16_t *src1;      // [B, X/ux, Y/uy, Z/uz, c1] or null
    const float *bias;       // [Cout] or null
    bf16_t *out;             // [B, OX, OY, OZ, Cout]
    int X, Y, Z, OX, OY, OZ;
    int c0, c1, Cin, Cout;
    int ux, uy, uz, X1, Y1, Z1;
    int kx, ky, kz, ntap, ntap4, dil;
    int px, py, pz;          // padding before
    int act;
    int dense;               // Cin < 8: dense K order
    int vec;                 // 8-channel groups are 16-byte aligned in both sources (c0, c1 multiples of 8, aligned bases)
    int CG;                  // channel groups of 8 per staged chunk (Cin >= 8)
    int nks;                 // k-steps in all
};

constexpr int BT_X = 4, BT_Y = 4, BT_Z = 16;

// one input channel at (x, y, z) of the concatenated (skip, up-sampled lo) tensor; the caller has checked the bounds
__device__ __forceinline__ bf16_t load_ch(const ConvB &a, const bf16_t *s0, const bf16_t *s1, int x, int y, int z, int c) {
    if (c < a.c0) return s0[(((long long)x * a.Y + y) * a.Z + z) * a.c0 + c];
    return s1[(((long long)(x / a.ux) * a.Y1 + (y / a.uy)) * a.Z1 + (z / a.uz)) * a.c1 + (c - a.c0)];
}

template <int NT>
__global__ __launch_bounds__(256) void conv3d_bf16(ConvB a, const u32x4 *__restrict__ wpacked, unsigned nblk, unsigned nby,
                                                   unsigned nbz) {
    extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
    const unsigned lb = nrt_xcd_block(blockIdx.x, gridDim.x);
    if (lb >= nblk) return;
    const int b = blockIdx.y;
    const int bz = lb % nbz, by = (lb / nbz) % nby, bx = lb / (nbz * nby);
    const int x0 = bx * BT_X, y0 = by * BT_Y, z0 = bz * BT_Z;
    const int HX = BT_X + (a.kx - 1) * a.dil, HY = BT_Y + (a.ky - 1) * a.dil, HZ = BT_Z + (a.kz - 1) * a.dil;
    const int nrows = HX * HY * HZ;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int ntt = (a.Cout + 15) >> 4, nt0 = blockIdx.z * NT;
    const int RS = a.dense ? 8 : 8 * a.CG + 8;                     // bf16 per staged row (16 bytes of padding)
    int *tab = (int *)(lds + (size_t)nrows * RS);                  // tap (Cin >= 8) or k (Cin < 8) -> LDS offset

    const bf16_t *s0 = a.src0 + (long long)b * a.X * a.Y * a.Z * a.c0;
    const bf16_t *s1 = a.src1 ? a.src1 + (long long)b * a.X1 * a.Y1 * a.Z1 * a.c1 : nullptr;

    // offset tables, written once per block
    if (a.dense) {
        const int K = a.ntap * a.Cin;
        for (int k = threadIdx.x; k < a.nks * 32; k += 256) {
            int v = -1;
            if (k < K) {
                const int t = k / a.Cin, c = k - t * a.Cin;
                const int dz = t % a.kz, dy = (t / a.kz) % a.ky, dx = t / (a.kz * a.ky);
                v = ((dx * a.dil * HY + dy * a.dil) * HZ + dz * a.dil) * RS + c;
            }
            tab[k] = v;
        }
    } else {
        for (int t = threadIdx.x; t < a.ntap4; t += 256) {
            int v = -1;
            if (t < a.ntap) {
                const int dz = t % a.kz, dy = (t / a.kz) % a.ky, dx = t / (a.kz * a.ky);
                v = ((dx * a.dil * HY + dy * a.dil) * HZ + dz * a.dil) * RS;
            }
            tab[t] = v;
        }
    }

    f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    const int base = ((w * HY) * HZ + li) * RS;                   // this lane's voxel (mt = 0) in the halo tile
    const int ng = (a.Cin + 7) >> 3, nq = a.ntap4 >> 2;
    const int nchunk = a.dense ? 1 : (ng + a.CG - 1) / a.CG;
    const u32x4 zero4 = (u32x4){0u, 0u, 0u, 0u};

    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();                                           // previous chunk consumed (and, first time, tables written)
        // ---- stage the halo tile of this chunk ----------------------------------------------------------
        const int G = a.dense ? 1 : a.CG;
        for (int it = threadIdx.x; it < nrows * G; it += 256) {
            const int r = it / G, gl = it - r * G;
            const int rz = r % HZ, ry = (r / HZ) % HY, rx = r / (HZ * HY);
            const int x = x0 - a.px + rx, y = y0 - a.py + ry, z = z0 - a.pz + rz;
            const int c = a.dense ? 0 : 8 * (ch * a.CG + gl);
            u32x4 v = zero4;
            if (x >= 0 && x < a.X && y >= 0 && y < a.Y && z >= 0 && z < a.Z && c < a.Cin) {
                if (a.vec) {
                    const bf16_t *p = c < a.c0 ? s0 + (((long long)x * a.Y + y) * a.Z + z) * a.c0 + c
                                               : s1 + (((long long)(x / a.ux) * a.Y1 + (y / a.uy)) * a.Z1 + (z / a.uz)) * a.c1 + (c - a.c0);
                    v = *(const u32x4 *)p;
                } else {
                    unsigned short e[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) e[j] = (c + j < a.Cin) ? load_ch(a, s0, s1, x, y, z, c + j) : (unsigned short)0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
                }
            }
            *(u32x4 *)&lds[r * RS + 8 * gl] = v;
        }
        __syncthreads();
        // ---- k-steps of this chunk --------------------------------------------------------------------
        auto step = [&](int s, const u32x4 (&xf)[4]) {
            u32x4 wf[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                wf[nt] = (nt0 + nt < ntt) ? wpacked[((long long)s * ntt + nt0 + nt) * 64 + lane] : zero4;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[nt]),
                                                                          __builtin_bit_cast(bf16x8, xf[mt]), acc[mt][nt], 0, 0, 0);
        };
        if (a.dense) {
            for (int s = 0; s < a.nks; ++s) {
                int off[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) off[j] = tab[32 * s + 8 * kq + j];
                u32x4 xf[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const bf16_t *p = lds + base + mt * HZ * RS;
                    unsigned short e[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) e[j] = off[j] >= 0 ? p[off[j]] : (unsigned short)0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) xf[mt][j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
                }
                step(s, xf);
            }
        } else {
            const int gend = min(ng - ch * a.CG, a.CG);
            for (int gl = 0; gl < gend; ++gl) {
                const int s0k = (ch * a.CG + gl) * nq;
                for (int q = 0; q < nq; ++q) {
                    const int off = tab[4 * q + kq];                  // pad taps (>= ntap) read zeros
                    u32x4 xf[4];
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        xf[mt] = off >= 0 ? *(const u32x4 *)(lds + base + mt * HZ * RS + off + 8 * gl) : zero4;
                    step(s0k + q, xf);
                }
            }
        }
    }
    // ---- epilogue: D[row = channel 4 kq + i][col = voxel li] -----------------------------------------------
    const int x = x0 + w, z = z0 + li;
    if (x >= a.OX || z >= a.OZ) return;
    bf16_t *ob = a.out + (long long)b * a.OX * a.OY * a.OZ * a.Cout;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int y = y0 + mt;
        if (y >= a.OY) continue;
        bf16_t *orow = ob + (((long long)x * a.OY + y) * a.OZ + z) * a.Cout;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = (nt0 + nt) * 16 + 4 * kq;
            if (co >= a.Cout) continue;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float bv = (a.bias && co + i < a.Cout) ? a.bias[co + i] : 0.0f;
                v[i] = nrt_activate_fused(acc[mt][nt][i] + bv, a.act);
            }
            if ((a.Cout & 3) == 0) {
                *(u32x2 *)(orow + co) = (u32x2){pack2(v[0], v[1]), pack2(v[2], v[3])};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (co + i < a.Cout) orow[co + i] = f2bf(v[i]);
            }
        }
    }
}

// Keras-layout weights [taps, Cin, Cout] (float32 or bf16) -> [k-step][nt][lane][8] bf16, the A operand of 16x16x32:
// lane l holds A[row = output channel 16 nt + (l & 15)][k = 8 (l >> 4) + j]
template <typename T>
__global__ void conv3d_pack_bf16(const T *__restrict__ w, int ntap, int ntap4, int Cin, int Cout, int nks, int ntt, int dense,
                                 bf16_t *__restrict__ packed) {
    const long long total = (long long)nks * ntt * 64 * 8;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int j = e & 7, lane = (e >> 3) & 63;
        long long r = e >> 9;
        const int nt = (int)(r % ntt), s = (int)(r / ntt);
        const int co = nt * 16 + (lane & 15);
        int t, c;
        if (dense) {
            const int k = 32 * s + 8 * (lane >> 4) + j;
            t = k / Cin; c = k - t * Cin;
        } else {
            const int nq = ntap4 >> 2, g = s / nq;
            t = 4 * (s - g * nq) + (lane >> 4); c = 8 * g + j;
        }
        bf16_t v = 0;
        if (t < ntap && c < Cin && co < Cout) {
            const T x = w[((long long)t * Cin + c) * Cout + co];
            if constexpr (sizeof(T) == 4) v = f2bf(x);
            else v = x;
        }
        packed[e] = v;
    }
}

void conv_geometry(const int *ksize, int cin, int cout, int &ntap, int &ntap4, int &nks, int &ntt, int &dense) {
    ntap = ksize[0] * ksize[1] * ksize[2];
    ntap4 = (ntap + 3) & ~3;
    dense = cin < 8;
    nks = dense ? (ntap * cin + 31) / 32 : ((cin + 7) / 8) * (ntap4 / 4);
    ntt = (cout + 15) / 16;
}

constexpr size_t LDS_MAX = 160 * 1024;

size_t conv_lds_bytes(const ConvB &a, int CG) {
    const size_t rows = (size_t)(BT_X + (a.kx - 1) * a.dil) * (BT_Y + (a.ky - 1) * a.dil) * (BT_Z + (a.kz - 1) * a.dil);
    const size_t RS = a.dense ? 8 : 8 * CG + 8;
    const size_t tab = a.dense ? (size_t)a.nks * 32 : (size_t)a.ntap4;
    return rows * RS * sizeof(bf16_t) + tab * sizeof(int);
}

template <int NT>
int launch_conv_bf16(const ConvB &a, const u32x4 *w, int batch, hipStream_t st, int nsplit) {
    const unsigned nbx = (a.OX + BT_X - 1) / BT_X, nby = (a.OY + BT_Y - 1) / BT_Y, nbz = (a.OZ + BT_Z - 1) / BT_Z;
    const unsigned nblk = nbx * nby * nbz;
    const size_t shm = conv_lds_bytes(a, a.CG);
    if (shm > 64 * 1024 &&
        hipFuncSetAttribute((const void *)conv3d_bf16<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
        return NRT_ERR_LAUNCH;
    hipLaunchKernelGGL((conv3d_bf16<NT>), dim3(nrt_xcd_grid(nblk), batch, nsplit), dim3(256), shm, st, a, w, nblk, nby, nbz);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// 1x1x1 convolution (+ channel softmax): one voxel per thread, the [cin, cout] weights as float32 in LDS (exact copies of bf16)
// ---------------------------------------------------------------------------------------------------------------
template <int CO_MAX>
__global__ __launch_bounds__(256) void conv1x1_bf16(const bf16_t *__restrict__ x, const bf16_t *__restrict__ w,
                                                    const float *__restrict__ bias, bf16_t *__restrict__ y, long long nvox, int cin,
                                                    int cout, int softmax, int act, int vec) {
    extern __shared__ float wl[];                                  // [cin][cout] then bias [cout]
    for (int i = threadIdx.x; i < cin * cout; i += 256) wl[i] = bf2f(w[i]);
    for (int i = threadIdx.x; i < cout; i += 256) wl[cin * cout + i] = bias ? bias[i] : 0.0f;
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nvox; q += (long long)gridDim.x * 256) {
        float acc[CO_MAX];
#pragma unroll
        for (int o = 0; o < CO_MAX; ++o) acc[o] = o < cout ? wl[cin * cout + o] : 0.0f;
        const bf16_t *xr = x + q * cin;
        auto fma_in = [&](float xv, int c) {
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o)
                if (o < cout) acc[o] = __fmaf_rn(xv, wl[c * cout + o], acc[o]);     // the bf16 x bf16 product is exact in float32
        };
        if (vec) {
            for (int c = 0; c < cin; c += 8) {
                float f[8];
                unpack8(*(const u32x4 *)(xr + c), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) fma_in(f[j], c + j);
            }
        } else {
            for (int c = 0; c < cin; ++c) fma_in(bf2f(xr[c]), c);
        }
        if (softmax) {
            float m = -INFINITY;
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o) if (o < cout) m = fmaxf(m, acc[o]);
            float s = 0.0f;
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o)
                if (o < cout) { acc[o] = __builtin_amdgcn_exp2f((acc[o] - m) * 1.44269504088896341f); s += acc[o]; }
            const float inv = 1.0f / s;
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o) acc[o] *= inv;
        } else {
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o) acc[o] = nrt_activate_fused(acc[o], act);
        }
        bf16_t *yr = y + q * cout;
        if (vec && (cout & 7) == 0) {
#pragma unroll
            for (int o = 0; o < CO_MAX; o += 8)
                if (o < cout) *(u32x4 *)(yr + o) = pack8(acc + o);
        } else {
#pragma unroll
            for (int o = 0; o < CO_MAX; ++o) if (o < cout) yr[o] = f2bf(acc[o]);
        }
    }
}

// softmax over the last axis: one row per thread, float32, one rounding; 16-byte loads / stores when V8
template <bool V8>
__global__ __launch_bounds__(256) void softmax_lastdim_bf16(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, long long n, int C) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
        const bf16_t *xr = x + q * C;
        bf16_t *yr = y + q * C;
        float m = -INFINITY, s = 0.0f;
        if (V8) {
            for (int c = 0; c < C; c += 8) {
                float f[8]; unpack8(*(const u32x4 *)(xr + c), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) m = fmaxf(m, f[j]);
            }
            for (int c = 0; c < C; c += 8) {
                float f[8]; unpack8(*(const u32x4 *)(xr + c), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += expf(f[j] - m);
            }
            const float inv = 1.0f / s;
            for (int c = 0; c < C; c += 8) {
                float f[8]; unpack8(*(const u32x4 *)(xr + c), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = expf(f[j] - m) * inv;
                *(u32x4 *)(yr + c) = pack8(f);
            }
        } else {
            for (int c = 0; c < C; ++c) m = fmaxf(m, bf2f(xr[c]));
            for (int c = 0; c < C; ++c) s += expf(bf2f(xr[c]) - m);
            const float inv = 1.0f / s;
            for (int c = 0; c < C; ++c) yr[c] = f2bf(expf(bf2f(xr[c]) - m) * inv);
        }
    }
}

// MaxPooling3D, stride = pool size, SAME (partial windows) or VALID; V = 8: one thread per (voxel, 8 channels)
template <int V>
__global__ __launch_bounds__(256) void maxpool3d_bf16(const bf16_t *__restrict__ x, bf16_t *__restrict__ y, int X, int Y, int Z, int C,
                                                      int OX, int OY, int OZ, int px, int py, int pz) {
    const int b = blockIdx.y;
    const bf16_t *xb = x + (long long)b * X * Y * Z * C;
    bf16_t *yb = y + (long long)b * OX * OY * OZ * C;
    const int CV = C / V;
    const long long total = (long long)OX * OY * OZ * CV;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % CV) * V;
        const long long q = e / CV;
        const int oz = q % OZ, oy = (q / OZ) % OY, ox = q / ((long long)OZ * OY);
        float m[V];
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = -INFINITY;
        for (int dx = 0; dx < px; ++dx) {
            const int xx = ox * px + dx; if (xx >= X) break;
            for (int dy = 0; dy < py; ++dy) {
                const int yy = oy * py + dy; if (yy >= Y) break;
                for (int dz = 0; dz < pz; ++dz) {
                    const int zz = oz * pz + dz; if (zz >= Z) break;
                    const bf16_t *p = xb + (((long long)xx * Y + yy) * Z + zz) * C + c;
                    if (V == 8) {
                        float f[8]; unpack8(*(const u32x4 *)p, f);
#pragma unroll
                        for (int j = 0; j < V; ++j) m[j] = fmaxf(m[j], f[j]);
                    } else {
                        m[0] = fmaxf(m[0], bf2f(p[0]));
                    }
                }
            }
        }
        if (V == 8) *(u32x4 *)(yb + q * C + c) = pack8(m);        // a maximum of bf16 values: exact
        else yb[q * C + c] = f2bf(m[0]);
    }
}

// UpSampling3D (nearest repeat) of `lo` + concatenate([skip, up]): a copy of bits; V = 8: 16-byte groups
template <int V>
__global__ __launch_bounds__(256) void upsample_concat_bf16(const bf16_t *__restrict__ skip, int c0, const bf16_t *__restrict__ lo, int c1,
                                                            bf16_t *__restrict__ y, int X, int Y, int Z, int ux, int uy, int uz) {
    const int b = blockIdx.y;
    const int C = c0 + c1, CV = C / V, X1 = X / ux, Y1 = Y / uy, Z1 = Z / uz;
    const bf16_t *sb = skip ? skip + (long long)b * X * Y * Z * c0 : nullptr;
    const bf16_t *lb = lo + (long long)b * X1 * Y1 * Z1 * c1;
    bf16_t *yb = y + (long long)b * X * Y * Z * C;
    const long long total = (long long)X * Y * Z * CV;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % CV) * V;
        const long long q = e / CV;
        const int z = q % Z, yy = (q / Z) % Y, x = q / ((long long)Z * Y);
        const bf16_t *p = (c < c0) ? sb + q * c0 + c : lb + (((long long)(x / ux) * Y1 + (yy / uy)) * Z1 + (z / uz)) * c1 + (c - c0);
        if (V == 8) *(u32x4 *)(yb + q * C + c) = *(const u32x4 *)p;
        else yb[q * C + c] = p[0];
    }
}

// y = act(a + b) [* scale + shift], or act(a) * b with ACT_MUL_B; float32 from the bf16 operands, one rounding.  V = 8: 16-byte groups
template <int V>
__global__ __launch_bounds__(256) void add_act_affine_bf16(const bf16_t *__restrict__ a, const bf16_t *__restrict__ bsrc,
                                                           const float *__restrict__ scale, const float *__restrict__ shift,
                                                           bf16_t *__restrict__ y, long long n, int C, int act) {
    const bool mul = (act & ACT_MUL_B) != 0;
    const long long nv = n / V;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nv; e += (long long)gridDim.x * blockDim.x) {
        float v[V], bv[V];
        if (V == 8) {
            unpack8(*(const u32x4 *)(a + e * 8), v);
            if (bsrc) unpack8(*(const u32x4 *)(bsrc + e * 8), bv);
        } else {
            v[0] = bf2f(a[e]);
            if (bsrc) bv[0] = bf2f(bsrc[e]);
        }
        const int c = (int)((e * V) % C);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float u = v[j];
            if (mul) u = nrt_activate(u, act & 0xff) * bv[j];
            else {
                if (bsrc) u += bv[j];
                u = nrt_activate(u, act);
            }
            if (scale) u = u * scale[c + j] + shift[c + j];
            v[j] = u;
        }
        if (V == 8) *(u32x4 *)(y + e * 8) = pack8(v);
        else y[e] = f2bf(v[0]);
    }
}

inline unsigned grid_for(long long items, unsigned cap) {
    long long b = (items + 255) / 256;
    if (b < 1) b = 1;
    return (unsigned)(b < cap ? b : cap);
}
inline bool al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" size_t nrt_conv3d_packed_weight_bytes_bf16(const int *ksize, int cin, int cout) {
    if (!ksize || cin < 1 || cout < 1 || ksize[0] < 1 || ksize[1] < 1 || ksize[2] < 1) return 0;
    int ntap, ntap4, nks, ntt, dense;
    conv_geometry(ksize, cin, cout, ntap, ntap4, nks, ntt, dense);
    return (size_t)nks * ntt * 64 * 8 * sizeof(bf16_t);
}

extern "C" int nrt_conv3d_pack_weights_bf16(const void *weights, int dtype, const int *ksize, int cin, int cout, void *packed,
                                            void *stream) {
    if (!weights || !packed || !ksize || cin < 1 || cout < 1) return NRT_ERR_INVALID_ARG;
    if (ksize[0] < 1 || ksize[1] < 1 || ksize[2] < 1) return NRT_ERR_INVALID_ARG;
    if (dtype != NRT_DT_F32 && dtype != NRT_DT_BF16) return NRT_ERR_UNSUPPORTED;
    int ntap, ntap4, nks, ntt, dense;
    conv_geometry(ksize, cin, cout, ntap, ntap4, nks, ntt, dense);
    const long long total = (long long)nks * ntt * 64 * 8;
    const unsigned blocks = grid_for(total, 4096);
    hipStream_t st = nrt_stream(stream);
    if (dtype == NRT_DT_F32)
        hipLaunchKernelGGL(conv3d_pack_bf16<float>, dim3(blocks), dim3(256), 0, st, (const float *)weights, ntap, ntap4, cin, cout, nks,
                           ntt, dense, (bf16_t *)packed);
    else
        hipLaunchKernelGGL(conv3d_pack_bf16<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t *)weights, ntap, ntap4, cin, cout,
                           nks, ntt, dense, (bf16_t *)packed);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_conv3d_bf16(const void *src0, int c0, const void *src1, int c1, const int *up, const void *packed_weights,
                               const float *bias, void *out, int batch, const int *shape, const int *ksize, int cout, int dilation,
                               int padding_same, int activation, void *stream) {
    if (!src0 || !out || !shape || !ksize || !packed_weights) return NRT_ERR_INVALID_ARG;
    if (c0 < 1 || c1 < 0 || cout < 1 || dilation < 1 || batch < 1 || batch > 65535) return NRT_ERR_INVALID_ARG;
    if (c1 > 0 && (!src1 || !up)) return NRT_ERR_INVALID_ARG;
    if (activation < ACT_NONE || activation > ACT_LAST_FUSED) return NRT_ERR_INVALID_ARG;
    ConvB a;
    a.src0 = (const bf16_t *)src0; a.src1 = c1 > 0 ? (const bf16_t *)src1 : nullptr; a.bias = bias; a.out = (bf16_t *)out;
    a.X = shape[0]; a.Y = shape[1]; a.Z = shape[2];
    if (a.X < 1 || a.Y < 1 || a.Z < 1) return NRT_ERR_INVALID_ARG;
    a.c0 = c0; a.c1 = c1; a.Cin = c0 + c1; a.Cout = cout;
    a.ux = c1 > 0 ? up[0] : 1; a.uy = c1 > 0 ? up[1] : 1; a.uz = c1 > 0 ? up[2] : 1;
    if (a.ux < 1 || a.uy < 1 || a.uz < 1) return NRT_ERR_INVALID_ARG;
    if (c1 > 0 && (a.X % a.ux || a.Y % a.uy || a.Z % a.uz)) return NRT_ERR_INVALID_ARG;
    a.X1 = a.X / a.ux; a.Y1 = a.Y / a.uy; a.Z1 = a.Z / a.uz;
    a.kx = ksize[0]; a.ky = ksize[1]; a.kz = ksize[2]; a.dil = dilation;
    if (a.kx < 1 || a.ky < 1 || a.kz < 1) return NRT_ERR_INVALID_ARG;
    if (padding_same) {
        a.px = ((a.kx - 1) * dilation) / 2; a.py = ((a.ky - 1) * dilation) / 2; a.pz = ((a.kz - 1) * dilation) / 2;
        a.OX = a.X; a.OY = a.Y; a.OZ = a.Z;
    } else {
        a.px = a.py = a.pz = 0;
        a.OX = a.X - (a.kx - 1) * dilation; a.OY = a.Y - (a.ky - 1) * dilation; a.OZ = a.Z - (a.kz - 1) * dilation;
        if (a.OX < 1 || a.OY < 1 || a.OZ < 1) return NRT_ERR_INVALID_ARG;
    }
    a.act = activation;
    int ntt;
    conv_geometry(ksize, a.Cin, cout, a.ntap, a.ntap4, a.nks, ntt, a.dense);
    a.vec = !a.dense && c0 % 8 == 0 && c1 % 8 == 0 && al16(src0) && (c1 == 0 || al16(src1));
    if (((uintptr_t)out) & 7) return NRT_ERR_INVALID_ARG;
    a.CG = 0;
    for (int cg = 4; cg >= 1 && !a.CG; cg >>= 1)
        if (conv_lds_bytes(a, cg) <= LDS_MAX) a.CG = cg;
    if (!a.CG) return NRT_ERR_UNSUPPORTED;                        // a halo tile of 8 channels does not fit the LDS (dilation too large)
    if (a.dense) a.CG = 1;
    hipStream_t st = nrt_stream(stream);
    // all N-tiles in one block, split over blockIdx.z when Cout > 64 or when the grid has fewer than two tiles per CU
    const long long tiles = (long long)batch * ((a.OX + BT_X - 1) / BT_X) * ((a.OY + BT_Y - 1) / BT_Y) * ((a.OZ + BT_Z - 1) / BT_Z);
    int NT = ntt < 4 ? ntt : 4;
    if (tiles < 2ll * nrt_num_cus() && ntt > 1 && ntt <= 4) NT = 1;
    const int nsplit = (ntt + NT - 1) / NT;
    switch (NT) {
        case 1: return launch_conv_bf16<1>(a, (const u32x4 *)packed_weights, batch, st, nsplit);
        case 2: return launch_conv_bf16<2>(a, (const u32x4 *)packed_weights, batch, st, nsplit);
        case 3: return launch_conv_bf16<3>(a, (const u32x4 *)packed_weights, batch, st, nsplit);
        default: return launch_conv_bf16<4>(a, (const u32x4 *)packed_weights, batch, st, nsplit);
    }
}

extern "C" int nrt_conv1x1_softmax_bf16(const void *x, const void *weights, const float *bias, void *y, long long nvox, int cin, int cout,
                                        int softmax, int activation, void *stream) {
    if (!x || !weights || !y || nvox < 0 || cin < 1 || cout < 1) return NRT_ERR_INVALID_ARG;
    if (activation < ACT_NONE || activation > ACT_LAST_FUSED) return NRT_ERR_INVALID_ARG;
    if (cout > 64 || (size_t)(cin + 1) * cout * sizeof(float) > 64 * 1024) return NRT_ERR_UNSUPPORTED;
    if (nvox == 0) return NRT_OK;
    const int vec = cin % 8 == 0 && al16(x) && al16(y);
    const size_t shm = (size_t)(cin + 1) * cout * sizeof(float);
    const unsigned blocks = grid_for(nvox, 256 * 16);
    hipStream_t st = nrt_stream(stream);
    const bf16_t *xp = (const bf16_t *)x, *wp = (const bf16_t *)weights;
    bf16_t *yp = (bf16_t *)y;
    if (cout <= 16) hipLaunchKernelGGL(conv1x1_bf16<16>, dim3(blocks), dim3(256), shm, st, xp, wp, bias, yp, nvox, cin, cout, softmax, activation, vec);
    else if (cout <= 32) hipLaunchKernelGGL(conv1x1_bf16<32>, dim3(blocks), dim3(256), shm, st, xp, wp, bias, yp, nvox, cin, cout, softmax, activation, vec);
    else hipLaunchKernelGGL(conv1x1_bf16<64>, dim3(blocks), dim3(256), shm, st, xp, wp, bias, yp, nvox, cin, cout, softmax, activation, vec);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_softmax_lastdim_bf16(const void *x, void *y, long long n, int channels, void *stream) {
    if (!x || !y || n < 0 || channels < 1) return NRT_ERR_INVALID_ARG;
    if (n == 0) return NRT_OK;
    const unsigned blocks = grid_for(n, 256 * 16);
    if (channels % 8 == 0 && al16(x) && al16(y))
        hipLaunchKernelGGL(softmax_lastdim_bf16<true>, dim3(blocks), dim3(256), 0, nrt_stream(stream), (const bf16_t *)x, (bf16_t *)y, n, channels);
    else
        hipLaunchKernelGGL(softmax_lastdim_bf16<false>, dim3(blocks), dim3(256), 0, nrt_stream(stream), (const bf16_t *)x, (bf16_t *)y, n, channels);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_maxpool3d_bf16(const void *x, void *y, int batch, const int *shape, int channels, const int *pool, int padding_same,
                                  void *stream) {
    if (!x || !y || !shape || !pool || batch < 1 || batch > 65535 || channels < 1) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < 3; ++d) if (pool[d] < 1 || shape[d] < 1) return NRT_ERR_INVALID_ARG;
    int o[3];
    for (int d = 0; d < 3; ++d) o[d] = padding_same ? (shape[d] + pool[d] - 1) / pool[d] : shape[d] / pool[d];
    const long long total = (long long)o[0] * o[1] * o[2] * channels;
    if (total == 0) return NRT_OK;
    const bool v8 = channels % 8 == 0 && al16(x) && al16(y);
    const unsigned blocks = grid_for(v8 ? total / 8 : total, 256 * 32);
    if (v8)
        hipLaunchKernelGGL(maxpool3d_bf16<8>, dim3(blocks, batch), dim3(256), 0, nrt_stream(stream), (const bf16_t *)x, (bf16_t *)y,
                           shape[0], shape[1], shape[2], channels, o[0], o[1], o[2], pool[0], pool[1], pool[2]);
    else
        hipLaunchKernelGGL(maxpool3d_bf16<1>, dim3(blocks, batch), dim3(256), 0, nrt_stream(stream), (const bf16_t *)x, (bf16_t *)y,
                           shape[0], shape[1], shape[2], channels, o[0], o[1], o[2], pool[0], pool[1], pool[2]);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_upsample_concat_bf16(const void *skip, int c0, const void *lo, int c1, void *y, int batch, const int *shape,
                                        const int *up, void *stream) {
    if (!lo || !y || !shape || !up || batch < 1 || batch > 65535 || c0 < 0 || c1 < 1) return NRT_ERR_INVALID_ARG;
    if (c0 > 0 && !skip) return NRT_ERR_INVALID_ARG;
    for (int d = 0; d < 3; ++d) if (up[d] < 1 || shape[d] < 1 || shape[d] % up[d]) return NRT_ERR_INVALID_ARG;
    const long long total = (long long)shape[0] * shape[1] * shape[2] * (c0 + c1);
    const bool v8 = c0 % 8 == 0 && c1 % 8 == 0 && (c0 == 0 || al16(skip)) && al16(lo) && al16(y);
    const unsigned blocks = grid_for(v8 ? total / 8 : total, 256 * 32);
    const bf16_t *sp = c0 > 0 ? (const bf16_t *)skip : nullptr;
    if (v8)
        hipLaunchKernelGGL(upsample_concat_bf16<8>, dim3(blocks, batch), dim3(256), 0, nrt_stream(stream), sp, c0, (const bf16_t *)lo, c1,
                           (bf16_t *)y, shape[0], shape[1], shape[2], up[0], up[1], up[2]);
    else
        hipLaunchKernelGGL(upsample_concat_bf16<1>, dim3(blocks, batch), dim3(256), 0, nrt_stream(stream), sp, c0, (const bf16_t *)lo, c1,
                           (bf16_t *)y, shape[0], shape[1], shape[2], up[0], up[1], up[2]);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_add_act_affine_bf16(const void *a, const void *b, const float *scale, const float *shift, void *y, long long n,
                                       int channels, int activation, void *stream) {
    if (!a || !y || n < 0 || channels < 1) return NRT_ERR_INVALID_ARG;
    if ((scale == nullptr) != (shift == nullptr)) return NRT_ERR_INVALID_ARG;
    if ((activation & 0xff) > ACT_LAST || (activation & ~(0xff | ACT_MUL_B)) || activation < 0) return NRT_ERR_INVALID_ARG;
    if ((activation & ACT_MUL_B) && !b) return NRT_ERR_INVALID_ARG;
    if (n == 0) return NRT_OK;
    const bool v8 = n % 8 == 0 && (!scale || channels % 8 == 0) && al16(a) && (!b || al16(b)) && al16(y);
    const unsigned blocks = grid_for(v8 ? n / 8 : n, 256 * 32);
    if (v8)
        hipLaunchKernelGGL(add_act_affine_bf16<8>, dim3(blocks), dim3(256), 0, nrt_stream(stream), (const bf16_t *)a, (const bf16_t *)b,
                           scale, shift, (bf16_t *)y, n, channels, activation);
    else
        hipLaunchKernelGGL(add_act_affine_bf16<1>, dim3(blocks), dim3(256), 0, nrt_stream(stream), (const bf16_t *)a, (const bf16_t *)b,
                           scale, shift, (bf16_t *)y, n, channels, activation);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
