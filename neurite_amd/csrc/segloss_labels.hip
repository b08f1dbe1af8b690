// Segmentation training loss on an integer LABEL MAP as y_true: soft Dice (neurite/tf/metrics.py:415-482) and the label-weighted
// categorical cross-entropy (metrics.py:619-650) of  one_hot(labels, L)  and  y_pred [B, ..., L] float32, without the one-hot map.
//
//   forward   nrt_seg_loss_labels_f32      one id (4 bytes) and one row of y_pred per voxel: 4 L + 4 bytes instead of the 8 L of segloss.hip
//   backward  nrt_seg_loss_labels_bwd_f32  d(sum_bl gD[b,l] dice[b,l] + gC cce_sum) / d y_pred, optionally through y_pred = softmax(z):
//                                          8 L + 4 bytes per voxel instead of 12 L
//
// The arithmetic is that of seg_loss_vec / seg_loss_bwd_vec with t[l] = (id == l): the same expressions in the same order inside a
// voxel (a term whose factor t is 0 is left out where leaving it out cannot change a bit: x - 0 * log q with q clipped to a finite
// range).  An id outside [0, L) is an all-zero row (tf.one_hot); an id is only ever COMPARED with a label, never used as an index.
// Lane groups: Gr = ceil(L / 4) lanes own the label quads of a voxel, in groups of G = next power of two >= Gr lanes (the lanes past Gr of a
// padded group load nothing, dice.hip: dice_soft_vec).  Two arms of the same kernels:
//   VEC      L % 4 == 0 and 16-byte aligned rows: one float4 per lane
//   generic  every other L in [1, 256] (1, 5, 33 ...) or unaligned rows: up to four scalar loads per lane, labels >= L of the last quad
//            masked.  Correct and measured, not tuned.
// WANT (Dice, CCE or both) is a template argument: a single loss does not pay for the other.  No atomics; block partials are added in a
// fixed order (dice_reduce.h, seg_lab_cce_finalize): run-to-run bit-identical.  64-bit element offsets.
#include "dice_reduce.h"

namespace {

constexpr float SEGL_KERAS_EPS = 1e-7f;
constexpr int SEGL_MAX_LABELS = 256;
constexpr int SEGL_BWD_BLOCK = 256;

// what a lane of a lane group owns: the labels l0 ... l0 + 3 that are < L (none in the padding lanes of the group)
struct SeglLane {
    int lg, l0;
    bool real, valid[4];
};

template <int G>
__device__ __forceinline__ SeglLane segl_lane(int L, int Gr) {
    SeglLane s;
    s.lg = threadIdx.x % G;
    s.real = s.lg < Gr;
    s.l0 = s.real ? 4 * s.lg : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s.valid[k] = s.real && s.l0 + k < L;
    return s;
}

// this lane's quad of the row of voxel v (zeros for what it does not own); rows is the batch entry's [nvox, L]
template <bool VEC, bool NT>
__device__ __forceinline__ nrt_f4 segl_load(const float *__restrict__ rows, long long v, int L, int Gr, const SeglLane &s) {
    nrt_f4 p = {0, 0, 0, 0};
    if (VEC) {
        const nrt_f4 *q = (const nrt_f4 *)rows + v * Gr + (s.l0 >> 2);
        const nrt_f4 r = NT ? __builtin_nontemporal_load(q) : *q;
        if (s.real) p = r;
    } else {
        const float *r = rows + v * L + s.l0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s.valid[k]) p[k] = r[k];
    }
    return p;
}

// which of the lane's four labels the id is: 0 ... 3, or 4 for none (an id outside [0, L) matches nothing; unsigned: any id is safe to subtract from)
__device__ __forceinline__ unsigned segl_match(int id, int L, const SeglLane &s) {
    return (s.real && (unsigned)id < (unsigned)L) ? (unsigned)id - 4u * (unsigned)s.lg : 4u;
}

// wave partials -> block partials (fpart [3 L], mpart [4], cpart [1] of this block); red is [waves][3 L + 5]
template <bool DICE, bool CCE>
__device__ __forceinline__ void segl_block_out(float *red, int L, float *__restrict__ fpart, float *__restrict__ mpart,
                                               float *__restrict__ cpart) {
    constexpr int NW = DICE_BLOCK / NRT_WAVE;
    const int row = 3 * L + 5;
    __syncthreads();
    const long long pbase = ((long long)blockIdx.y * gridDim.x + blockIdx.x);
    if (DICE) {
        for (int i = threadIdx.x; i < 3 * L; i += DICE_BLOCK) {
            float s = red[i];
#pragma unroll
            for (int w2 = 1; w2 < NW; ++w2) s += red[w2 * row + i];
            fpart[pbase * 3 * L + i] = s;
        }
        if (threadIdx.x < 4) {
            float m = red[3 * L + threadIdx.x];
            for (int w2 = 1; w2 < NW; ++w2)
                m = (threadIdx.x & 1) ? fmaxf(m, red[w2 * row + 3 * L + threadIdx.x]) : fminf(m, red[w2 * row + 3 * L + threadIdx.x]);
            mpart[pbase * 4 + threadIdx.x] = m;
        }
    }
    if (CCE && threadIdx.x == 4) {
        float s = red[3 * L + 4];
        for (int w2 = 1; w2 < NW; ++w2) s += red[w2 * row + 3 * L + 4];
        cpart[pbase] = s;
    }
}

template <int G, bool VEC, int WANT>
__global__ __launch_bounds__(DICE_BLOCK) void seg_lab_fwd(const int *__restrict__ lab, const float *__restrict__ yp,
                                                          const float *__restrict__ lw, long long nvox, int L, int Gr, float smooth,
                                                          float *__restrict__ fpart, float *__restrict__ mpart,
                                                          float *__restrict__ cpart) {
    constexpr int NG = DICE_BLOCK / G;
    constexpr bool DICE = (WANT & NRT_SEG_WANT_DICE) != 0, CCE = (WANT & NRT_SEG_WANT_CCE) != 0;
    const int b = blockIdx.y;
    const int *ib = lab + (long long)b * nvox;
    const float *rows = yp + (long long)b * nvox * L;
    const SeglLane s = segl_lane<G>(L, Gr);
    const long long g = threadIdx.x / G;
    float wq[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (CCE && lw) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s.valid[k]) wq[k] = lw[s.l0 + k];
    }
    const float keep = 1.0f - smooth, add = smooth / (float)L;

    nrt_f4 stp = {0, 0, 0, 0}, stt = {0, 0, 0, 0}, spp = {0, 0, 0, 0};
    float mnp = INFINITY, mxp = -INFINITY, cce = 0.0f;
    long long vbeg, vend;
    nrt_block_range(nvox, NG, vbeg, vend);
#pragma unroll 4
    for (long long v = vbeg + g; v < vend; v += NG) {
        const int id = ib[v];
        const nrt_f4 p = segl_load<VEC, true>(rows, v, L, Gr, s);
        const unsigned kk = segl_match(id, L, s);
        if (DICE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool hit = kk == (unsigned)k;
                stp[k] += hit ? p[k] : 0.0f;
                stt[k] += hit ? 1.0f : 0.0f;
                spp[k] += p[k] * p[k];
                if (s.valid[k]) { mnp = fminf(mnp, p[k]); mxp = fmaxf(mxp, p[k]); }
            }
        }
        if (CCE) {
            const float sp = nrt_wave_sum<G>((p[0] + p[1]) + (p[2] + p[3]));
            float l = 0.0f;
            if (smooth != 0.0f) {                                 // every label carries weight: seg_loss_vec as it stands
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float q = p[k] / sp;
                    q = fminf(fmaxf(q, SEGL_KERAS_EPS), 1.0f - SEGL_KERAS_EPS);
                    float tt = wq[k] * (kk == (unsigned)k ? 1.0f : 0.0f);
                    tt = tt * keep + add;
                    const float term = tt * logf(q);
                    if (s.valid[k]) l -= term;
                }
            } else if (kk < 4u) {                                 // one non-zero term per voxel, in the lane that owns the id
                const float pk = kk == 0u ? p[0] : kk == 1u ? p[1] : kk == 2u ? p[2] : p[3];
                const float wk = kk == 0u ? wq[0] : kk == 1u ? wq[1] : kk == 2u ? wq[2] : wq[3];
                float q = pk / sp;
                q = fminf(fmaxf(q, SEGL_KERAS_EPS), 1.0f - SEGL_KERAS_EPS);
                l -= (wk * 1.0f) * logf(q);
            }
            cce += l;
        }
    }
    __shared__ float red[(DICE_BLOCK / NRT_WAVE) * (3 * 4 * G + 5)];     // L <= 4 Gr <= 4 G
    const int lane = threadIdx.x & (NRT_WAVE - 1), wv = threadIdx.x / NRT_WAVE;
    float *r = red + wv * (3 * L + 5);
    if (DICE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            stp[k] = nrt_wave_sum_from(stp[k], G);
            stt[k] = nrt_wave_sum_from(stt[k], G);
            spp[k] = nrt_wave_sum_from(spp[k], G);
        }
        if (lane < Gr) {                                          // (lane < G: lg == lane, s.valid is this lane's)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (s.valid[k]) {
                    r[0 * L + 4 * lane + k] = stp[k];
                    r[1 * L + 4 * lane + k] = stt[k];
                    r[2 * L + 4 * lane + k] = spp[k];
                }
            }
        }
    }
    // (nrt_wave_min / nrt_wave_max / nrt_wave_sum by hand: one loop, each chain only in the instances that need it)
    for (int off = 1; off < NRT_WAVE; off <<= 1) {
        if (DICE) { mnp = fminf(mnp, __shfl_xor(mnp, off, NRT_WAVE)); mxp = fmaxf(mxp, __shfl_xor(mxp, off, NRT_WAVE)); }
        if (CCE) cce += __shfl_xor(cce, off, NRT_WAVE);
    }
    if (lane == 0) {
        r[3 * L + 0] = 0.0f; r[3 * L + 1] = 1.0f;                  // the bounds of a one-hot row stand in for min t, max t
        r[3 * L + 2] = mnp; r[3 * L + 3] = mxp; r[3 * L + 4] = cce;
    }
    segl_block_out<DICE, CCE>(red, L, fpart, mpart, cpart);
}

// block partials of the CCE -> one float, fixed order, float64 accumulation (segloss.hip: seg_cce_finalize)
__global__ __launch_bounds__(256) void seg_lab_cce_finalize(const float *__restrict__ part, int n, float *__restrict__ out) {
    __shared__ double sl[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) a += (double)part[k];
    sl[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += sl[i];
        out[0] = (float)s;
    }
}

// SM: the gradient is taken through y_pred = softmax(z) and written as dz
template <int G, bool VEC, bool SM, int WANT>
__global__ __launch_bounds__(SEGL_BWD_BLOCK) void seg_lab_bwd(const int *__restrict__ lab, const float *__restrict__ yp,
                                                              const float *__restrict__ lw, const float *__restrict__ sums,
                                                              const float *__restrict__ gdice, const float *__restrict__ gcce,
                                                              long long nvox, int L, int Gr, float smooth, float eps,
                                                              float *__restrict__ out) {
    constexpr int NG = SEGL_BWD_BLOCK / G;
    constexpr bool DICE = (WANT & NRT_SEG_WANT_DICE) != 0, CCE = (WANT & NRT_SEG_WANT_CCE) != 0;
    const int b = blockIdx.y;
    const int *ib = lab + (long long)b * nvox;
    const float *rows = yp + (long long)b * nvox * L;
    float *orows = out + (long long)b * nvox * L;
    const SeglLane s = segl_lane<G>(L, Gr);
    const long long g = threadIdx.x / G;
    float ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0}, wq[4] = {1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                 // backward.hip: dice_soft_bwd_vec
        if (!s.valid[k]) continue;
        const int l = s.l0 + k;
        if (DICE) {
            const float *s3 = sums + (long long)b * 3 * L;
            const float num = 2.0f * s3[l] + eps, den = s3[L + l] + s3[2 * L + l] + eps;
            const float gd = gdice[(long long)b * L + l];
            if (den != 0.0f) { ca[k] = 2.0f * gd / den; cb[k] = -2.0f * gd * num / (den * den); }
        }
        if (CCE && lw) wq[k] = lw[l];
    }
    float gc = 0.0f;
    if (CCE) gc = gcce[0];
    const float keep = 1.0f - smooth, add = smooth / (float)L;
    long long vbeg, vend;
    nrt_block_range(nvox, NG, vbeg, vend);
#pragma unroll 2
    for (long long v = vbeg + g; v < vend; v += NG) {
        const int id = ib[v];
        const nrt_f4 p = segl_load<VEC, false>(rows, v, L, Gr, s);
        const unsigned kk = segl_match(id, L, s);
        nrt_f4 d = {0, 0, 0, 0};
        if (DICE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = ca[k] * (kk == (unsigned)k ? 1.0f : 0.0f) + cb[k] * p[k];
        }
        if (CCE) {                                                // backward.hip: wcce_bwd_vec, probabilities
            const float sp = nrt_wave_sum<G>((p[0] + p[1]) + (p[2] + p[3]));
            float tt[4], q[4], rq = 0.0f;
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tt[k] = wq[k] * (kk == (unsigned)k ? 1.0f : 0.0f);
                if (smooth != 0.0f) tt[k] = tt[k] * keep + add;
                q[k] = p[k] / sp;
                in[k] = s.valid[k] && q[k] >= SEGL_KERAS_EPS && q[k] <= 1.0f - SEGL_KERAS_EPS;
                rq += in[k] ? tt[k] : 0.0f;
            }
            rq = nrt_wave_sum<G>(rq);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float c = -gc * ((in[k] ? tt[k] / q[k] : 0.0f) - rq) / sp;
                d[k] = DICE ? d[k] + c : c;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!s.valid[k]) d[k] = 0.0f;
        if (SM) {                                                 // conv_bwd.hip: softmax_bwd_vec
            const float dot = nrt_wave_sum<G>((d[0] * p[0] + d[1] * p[1]) + (d[2] * p[2] + d[3] * p[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = p[k] * (d[k] - dot);
        }
        // read again by the head's wgrad / dgrad: normal stores
        if (VEC) {
            if (s.real) ((nrt_f4 *)orows)[v * Gr + s.lg] = d;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (s.valid[k]) orows[v * L + s.l0 + k] = d[k];
        }
    }
}

bool segl_labels_ok(int L) { return L >= 1 && L <= SEGL_MAX_LABELS; }
int segl_pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

struct SeglFwdArgs {
    const int *lab; const float *yp, *lw; long long nvox; int L, Gr; float smooth; float *fpart, *mpart, *cpart;
};

template <int G, bool VEC, int WANT>
void segl_fwd_launch(dim3 grid, hipStream_t st, const SeglFwdArgs &a) {
    hipLaunchKernelGGL((seg_lab_fwd<G, VEC, WANT>), grid, dim3(DICE_BLOCK), 0, st, a.lab, a.yp, a.lw, a.nvox, a.L, a.Gr, a.smooth, a.fpart,
                       a.mpart, a.cpart);
}

template <int G>
void segl_fwd_dispatch(bool vec, int want, dim3 grid, hipStream_t st, const SeglFwdArgs &a) {
    constexpr int D = NRT_SEG_WANT_DICE, C = NRT_SEG_WANT_CCE;
    if (vec) {
        if (want == D) segl_fwd_launch<G, true, D>(grid, st, a);
        else if (want == C) segl_fwd_launch<G, true, C>(grid, st, a);
        else segl_fwd_launch<G, true, D | C>(grid, st, a);
    } else {
        if (want == D) segl_fwd_launch<G, false, D>(grid, st, a);
        else if (want == C) segl_fwd_launch<G, false, C>(grid, st, a);
        else segl_fwd_launch<G, false, D | C>(grid, st, a);
    }
}

struct SeglBwdArgs {
    const int *lab; const float *yp, *lw, *sums, *gd, *gc; long long nvox; int L, Gr; float smooth, eps; float *out;
};

template <int G, bool VEC, bool SM, int WANT>
void segl_bwd_launch(dim3 grid, hipStream_t st, const SeglBwdArgs &a) {
    hipLaunchKernelGGL((seg_lab_bwd<G, VEC, SM, WANT>), grid, dim3(SEGL_BWD_BLOCK), 0, st, a.lab, a.yp, a.lw, a.sums, a.gd, a.gc, a.nvox, a.L,
                       a.Gr, a.smooth, a.eps, a.out);
}

template <int G, bool VEC, bool SM>
void segl_bwd_want(int want, dim3 grid, hipStream_t st, const SeglBwdArgs &a) {
    constexpr int D = NRT_SEG_WANT_DICE, C = NRT_SEG_WANT_CCE;
    if (want == D) segl_bwd_launch<G, VEC, SM, D>(grid, st, a);
    else if (want == C) segl_bwd_launch<G, VEC, SM, C>(grid, st, a);
    else segl_bwd_launch<G, VEC, SM, D | C>(grid, st, a);
}

template <int G>
void segl_bwd_dispatch(bool vec, bool sm, int want, dim3 grid, hipStream_t st, const SeglBwdArgs &a) {
    if (vec) {
        if (sm) segl_bwd_want<G, true, true>(want, grid, st, a);
        else segl_bwd_want<G, true, false>(want, grid, st, a);
    } else {
        if (sm) segl_bwd_want<G, false, true>(want, grid, st, a);
        else segl_bwd_want<G, false, false>(want, grid, st, a);
    }
}

}  // namespace

extern "C" int nrt_seg_loss_labels_supported(int nlabels) { return segl_labels_ok(nlabels) ? 1 : 0; }

extern "C" size_t nrt_seg_loss_labels_workspace_bytes(long long nvox, int nlabels, int batch) {
    if (nvox < 1 || !segl_labels_ok(nlabels) || batch < 1 || batch > 65535) return 0;
    return dice_ws_bytes(nlabels, batch) + (size_t)batch * DICE_MAX_BLOCKS * sizeof(float) + 256;
}

extern "C" int nrt_seg_loss_labels_f32(const int32_t *labels, const float *y_pred, const float *label_weights, long long nvox, int nlabels,
                                       int batch, int want, float label_smoothing, float laplace_smoothing, float *sums, float *dice,
                                       float *minmax, float *cce_sum, void *workspace, size_t workspace_bytes, void *stream) {
    const bool wd = (want & NRT_SEG_WANT_DICE) != 0, wc = (want & NRT_SEG_WANT_CCE) != 0;
    if (!labels || !y_pred || want < 1 || want > (NRT_SEG_WANT_DICE | NRT_SEG_WANT_CCE)) return NRT_ERR_INVALID_ARG;
    if ((wd && (!sums || !dice)) || (wc && !cce_sum) || (!wd && minmax)) return NRT_ERR_INVALID_ARG;
    if (nvox < 1 || batch < 1 || !segl_labels_ok(nlabels)) return NRT_ERR_INVALID_ARG;
    if (batch > 65535) return NRT_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < nrt_seg_loss_labels_workspace_bytes(nvox, nlabels, batch)) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    DiceWs w = dice_ws_carve(workspace, nlabels, batch);
    float *cpart = (float *)(((uintptr_t)workspace + dice_ws_bytes(nlabels, batch) + 15) & ~(uintptr_t)15);
    const bool vec = nlabels % 4 == 0 && ((uintptr_t)y_pred & 15) == 0;
    const int Gr = (nlabels + 3) / 4, G = segl_pow2_at_least(Gr);
    const unsigned nblk = dice_num_blocks(nvox, (DICE_BLOCK / G) * 4);
    const dim3 grid(nblk, batch);
    const SeglFwdArgs a = {labels, y_pred, label_weights, nvox, nlabels, Gr, label_smoothing, w.fpart, w.mpart, cpart};
    switch (G) {
        case 1: segl_fwd_dispatch<1>(vec, want, grid, st, a); break;
        case 2: segl_fwd_dispatch<2>(vec, want, grid, st, a); break;
        case 4: segl_fwd_dispatch<4>(vec, want, grid, st, a); break;
        case 8: segl_fwd_dispatch<8>(vec, want, grid, st, a); break;
        case 16: segl_fwd_dispatch<16>(vec, want, grid, st, a); break;
        case 32: segl_fwd_dispatch<32>(vec, want, grid, st, a); break;
        default: segl_fwd_dispatch<64>(vec, want, grid, st, a); break;
    }
    NRT_CHECK_LAUNCH();
    if (wc) {
        hipLaunchKernelGGL(seg_lab_cce_finalize, dim3(1), dim3(256), 0, st, (const float *)cpart, (int)(nblk * (unsigned)batch), cce_sum);
        NRT_CHECK_LAUNCH();
    }
    if (wd) return dice_finalize_soft(w, nblk, 1, batch, nlabels, laplace_smoothing, sums, dice, minmax, st);
    return NRT_OK;
}

extern "C" int nrt_seg_loss_labels_bwd_f32(const int32_t *labels, const float *y_pred, const float *label_weights, const float *sums,
                                           const float *grad_dice, const float *grad_cce, long long nvox, int nlabels, int batch,
                                           float label_smoothing, float laplace_smoothing, int through_softmax, float *grad, void *stream) {
    if (!labels || !y_pred || !grad || (!grad_dice && !grad_cce) || (grad_dice && !sums)) return NRT_ERR_INVALID_ARG;
    if (nvox < 1 || batch < 1 || !segl_labels_ok(nlabels)) return NRT_ERR_INVALID_ARG;
    if (batch > 65535) return NRT_ERR_UNSUPPORTED;
    hipStream_t st = nrt_stream(stream);
    const int want = (grad_dice ? NRT_SEG_WANT_DICE : 0) | (grad_cce ? NRT_SEG_WANT_CCE : 0);
    const bool vec = nlabels % 4 == 0 && (((uintptr_t)y_pred | (uintptr_t)grad) & 15) == 0;
    const int Gr = (nlabels + 3) / 4, G = segl_pow2_at_least(Gr);
    const dim3 grid(dice_num_blocks(nvox, (SEGL_BWD_BLOCK / G) * 4), batch);
    const SeglBwdArgs a = {labels, y_pred, label_weights, sums, grad_dice, grad_cce, nvox, nlabels, Gr, label_smoothing, laplace_smoothing, grad};
    const bool sm = through_softmax != 0;
    switch (G) {
        case 1: segl_bwd_dispatch<1>(vec, sm, want, grid, st, a); break;
        case 2: segl_bwd_dispatch<2>(vec, sm, want, grid, st, a); break;
        case 4: segl_bwd_dispatch<4>(vec, sm, want, grid, st, a); break;
        case 8: segl_bwd_dispatch<8>(vec, sm, want, grid, st, a); break;
        case 16: segl_bwd_dispatch<16>(vec, sm, want, grid, st, a); break;
        case 32: segl_bwd_dispatch<32>(vec, sm, want, grid, st, a); break;
        default: segl_bwd_dispatch<64>(vec, sm, want, grid, st, a); break;
    }
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
