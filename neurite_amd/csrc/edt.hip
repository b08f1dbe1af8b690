// Exact Euclidean distance transforms and the surface-distance reductions built on them.  What they replace: a copy of
// every volume to the host, scipy.ndimage.distance_transform_edt there (what VoxelMorph's dist_trf / signed_dist_trf call; restated,
// voxelmorph is not in the reference tree), and a copy back.
//
// out is [B, *S, L] float32 (L = 1 for a binary volume), D = len(S) in {2, 3}, every extent at most 1024.  The squared transform is
// separable: one pass per spatial axis, on out in place, viewed as [outer, n, inner] (inner holds the later axes and the L channels):
//     pass a:   f[i] = min_j ( g[j] + (s_a (i - j))^2 )            g the line before the pass, s_a the voxel size along the axis
// For the first pass g[j] is 0 at a feature voxel and +inf elsewhere, evaluated from the source on the fly (no mask tensor exists):
//     a uint8 volume: nonzero;   an int32 id map and a label list: ids == labels[l] (one-vs-rest, l the channel) or, with ANY_OF, ids in
//     the list (one channel);    SURFACE: voxels of the set with a face neighbour (2 D of them) outside it, the outside of the volume
//     counting as outside the set;   INVERT: the complement of all that.
// A line without a feature stays +inf through every pass (inf + x = inf), so no sentinel needs replacing at the end.
//
// Arithmetic: t(d) = fl(fl(s d) fl(s d)), candidate = fl(g[j] + t(|i - j|)), float32, no fused multiply-add.  The search runs outward
// from i, four distances at a time, and stops at the first group whose nearest d has t(d) >= best: t is monotone in d and g >= 0, so
// nothing farther can be smaller; the result is the plain minimum over the line.  The first pass needs no search: with g in {0, +inf}
// the minimum is t(distance to the nearest feature voxel of the line), found by one walk up and one walk down the line.  At unit
// spacing every value is an integer below sum (n_a - 1)^2 < 2^24: exact, in any order.
// The last pass takes the correctly rounded root (unless SQUARED) and, for SIGNED, combines two transforms: `first` holds the squared
// transform of the set (0 exactly on the set), this one is the complement's:  out = first > 0 ? root(first) : -root(this).
//
// One kernel, two arms, chosen by the line image n * inner:
//   contiguous  n * inner <= 16384 floats: a block takes `to` consecutive outer entries, a contiguous range of out that is copied to LDS
//               as it lies (to = max(1, 4096 / (n * inner))); lanes run along the range.  This covers the innermost axis of a
//               one-channel call (inner = 1: a block holds whole lines side by side and a wave works on a run of lines).
//   tiled       otherwise: a block takes the n lines of `ti` neighbouring inner positions of one outer entry (ti = 64 for n <= 256, 32 up
//               to 512, 16 up to 1024: at most 64 KiB), lanes along inner.
// Either way a block reads its lines completely into LDS before it writes any of them, and no two blocks share a line: safe in place.
// No atomics, no host synchronisation, no allocation: bit-identical run to run, and the calls capture into a graph.
//
// surface_stats: for every (batch entry, label) the surface voxels of label map t are walked and the squared distance d2 read there
// (the transform from the other map's surfaces) is reduced to count, max of d2 and the float64 sum of root(d2): per-block
// partials over fixed runs of voxels, added in block order by a second launch.  Optionally bin (int) d2 of a uint32 histogram is
// incremented (integer atomics commute: the bins are bit-identical run to run as well).
#include "nrt_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;                       // surface statistics
constexpr int kEdtThreads = 1024;                   // a transform pass: 16 waves share one LDS image
constexpr int kFar = 1 << 20;                       // farther than any extent
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kLdsFloats = 16384;                    // the largest LDS image of a block: 64 KiB
constexpr int kChunkFloats = 4096;                   // contiguous arm: outer entries are gathered up to this many floats per block
constexpr int kMaxExtent = 1024, kMaxLabels = 256;
constexpr int kRunVoxels = 2048, kMaxRuns = 256;     // surface_stats: voxels of a block's run at least, runs per (entry, label) at most
constexpr int kPartWords = 4;                        // count, max, and the float64 sum as (hi, lo) words

struct EdtGeom {
    int B, nd;
    int n[3];                                        // the nd extents, outermost first; 1 behind them
    int V, L;                                        // voxels of a batch entry; channels of out
};

struct EdtSrc {
    const unsigned char *mask;                       // [B, V], or
    const int *ids;                                  // [B, V] with
    const int *labels;                               // [nlabels]
    int nlabels, surface, invert, any_of;
};

__device__ __forceinline__ bool edt_in_set(const EdtSrc &s, int id, int l) {
    if (!s.any_of) return id == s.labels[l];
    bool in = false;
    for (int k = 0; k < s.nlabels; ++k) in |= id == s.labels[k];
    return in;
}

// whether voxel v (in the set) of the entry at `ids` has a face neighbour outside the set, or lies at the border of the volume
__device__ __forceinline__ bool edt_on_surface(const EdtSrc &s, const EdtGeom &g, const int *__restrict__ ids, unsigned v, int l) {
    unsigned r = v;
    int i[3], st[3];
    int stride = 1;
#pragma unroll
    for (int a = 2; a >= 0; --a) {
        const unsigned q = r / (unsigned)g.n[a];
        i[a] = (int)(r - q * (unsigned)g.n[a]);
        r = q;
        st[a] = stride;
        stride *= g.n[a];
    }
    bool edge = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a >= g.nd) continue;                     // (the padding extents are no axes: they have no outside)
        if (i[a] == 0 || !edt_in_set(s, ids[v - (unsigned)st[a]], l)) edge = true;
        if (i[a] == g.n[a] - 1 || !edt_in_set(s, ids[v + (unsigned)st[a]], l)) edge = true;
    }
    return edge;
}

// g of the first pass at element ge of out [B, V, L]: 0 at a feature voxel, +inf elsewhere
__device__ __forceinline__ float edt_seed(const EdtSrc &s, const EdtGeom &g, unsigned ge) {
    const unsigned bv = ge / (unsigned)g.L;
    const int l = (int)(ge - bv * (unsigned)g.L);
    bool f;
    if (s.mask) f = s.mask[bv] != 0;
    else {
        f = edt_in_set(s, s.ids[bv], l);
        if (f && s.surface) {
            const unsigned b = bv / (unsigned)g.V;
            f = edt_on_surface(s, g, s.ids + (size_t)b * g.V, bv - b * (unsigned)g.V, l);
        }
    }
    return (f != (s.invert != 0)) ? 0.0f : INFINITY;
}

struct EdtPass {
    int n;                                           // extent of the axis
    unsigned inner, outer;
    int ti;                                          // 0: the contiguous arm; else the tile width of the tiled arm
    unsigned to, tiles;                              // outer entries per block (contiguous); tiles per outer entry (tiled)
    float s;                                         // voxel size along the axis
    int first, last, squared;
};

__device__ __forceinline__ float edt_term(float s, int d) {
    const float sd = nrt_mul(s, (float)d);
    return nrt_mul(sd, sd);
}

// dynamic LDS: the block's image, (entries of the block) * n * inner floats or n * ti floats
__global__ void __launch_bounds__(kEdtThreads)
edt_pass(EdtSrc src, const float *__restrict__ first, float *__restrict__ out, EdtGeom g, EdtPass p) {
    extern __shared__ float lds[];
    const unsigned line = (unsigned)p.n * p.inner;
    unsigned base, cnt, stride, w = 0;
    if (p.ti == 0) {
        const unsigned o0 = blockIdx.x * p.to;
        base = o0 * line;
        cnt = min(p.to, p.outer - o0) * line;
        stride = p.inner;
    } else {
        const unsigned o = blockIdx.x / p.tiles, c0 = (blockIdx.x - o * p.tiles) * (unsigned)p.ti;
        base = o * line + c0;
        cnt = (unsigned)p.n * (unsigned)p.ti;
        stride = (unsigned)p.ti;
        w = min((unsigned)p.ti, p.inner - c0);
    }
    for (unsigned idx = threadIdx.x; idx < cnt; idx += kEdtThreads) {
        unsigned ge = base + idx;
        if (p.ti != 0) {
            const unsigned j = idx / stride, c = idx - j * stride;
            if (c >= w) continue;
            ge = base + j * p.inner + c;
        }
        lds[idx] = p.first ? edt_seed(src, g, ge) : out[ge];
    }
    __syncthreads();
    if (p.first) {
        // g is 0 or +inf: the minimum is the term of the nearest feature voxel of the line.  One thread per line walks it up, leaving the
        // distance to the last feature below, and down again with the next feature above: 2 n steps instead of a search per element.
        const unsigned cols = p.ti == 0 ? cnt / (unsigned)p.n : w;
        for (unsigned k = threadIdx.x; k < cols; k += kEdtThreads) {
            const unsigned idx0 = p.ti == 0 ? (k / p.inner) * line + k % p.inner : k;
            int last = -kFar;
            for (int j = 0; j < p.n; ++j) {
                const unsigned idx = idx0 + (unsigned)j * stride;
                last = lds[idx] == 0.0f ? j : last;
                lds[idx] = (float)(j - last);                            // (below 2^21: exact)
            }
            int next = kFar;
            for (int j = p.n - 1; j >= 0; --j) {
                const unsigned idx = idx0 + (unsigned)j * stride;
                const int below = (int)lds[idx];
                next = below == 0 ? j : next;
                const int d = min(below, next - j);
                lds[idx] = d < p.n ? edt_term(p.s, d) : INFINITY;
            }
        }
        __syncthreads();
    }
    for (unsigned idx = threadIdx.x; idx < cnt; idx += kEdtThreads) {
        unsigned ge = base + idx;
        int i;
        if (p.ti != 0) {
            const unsigned j = idx / stride, c = idx - j * stride;
            if (c >= w) continue;
            ge = base + j * p.inner + c;
            i = (int)j;
        } else {
            i = (int)((idx % line) / p.inner);
        }
        float best = lds[idx];
        if (!p.first) {
            // outward from i, four distances at a time (their eight reads are independent of each other); a group is entered only
            // while the term of its first distance is below the best so far, and whatever else it looks at is a candidate like any other
            const int dmax = max(i, p.n - 1 - i);
            for (int d0 = 1; d0 <= dmax; d0 += 4) {
                if (!(edt_term(p.s, d0) < best)) break;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int d = d0 + u;
                    const float t = edt_term(p.s, d);
                    const float lo = d <= i ? lds[idx - (unsigned)d * stride] : INFINITY;
                    const float hi = i + d < p.n ? lds[idx + (unsigned)d * stride] : INFINITY;
                    best = fminf(best, fminf(nrt_add(lo, t), nrt_add(hi, t)));
                }
            }
        }
        if (p.last) {
            float r = p.squared ? best : sqrtf(best);
            if (first) {
                const float f = first[ge];
                r = f > 0.0f ? (p.squared ? f : sqrtf(f)) : -r;
            }
            best = r;
        }
        out[ge] = best;
    }
}

__device__ __forceinline__ void store_f64(unsigned *p, double s) {
    p[0] = (unsigned)__double2hiint(s);
    p[1] = (unsigned)__double2loint(s);
}
__device__ __forceinline__ double load_f64(const unsigned *p) { return __hiloint2double((int)p[0], (int)p[1]); }

// grid = B * L * nb; part [B * L * nb][kPartWords]; hist [B * L][nbins] or NULL
__global__ void __launch_bounds__(kThreads)
surface_stats(const int *__restrict__ t, const int *__restrict__ labels, const float *__restrict__ d2, EdtGeom g, int nb, int per,
              unsigned *__restrict__ part, unsigned *__restrict__ hist, unsigned nbins) {
    __shared__ double red[kWaves];
    __shared__ float redf[kWaves];
    __shared__ int redi[kWaves];
    const unsigned bl = blockIdx.x / (unsigned)nb, k = blockIdx.x - bl * (unsigned)nb;
    const unsigned b = bl / (unsigned)g.L;
    const int l = (int)(bl - b * (unsigned)g.L);
    EdtSrc s;
    s.mask = nullptr;
    s.ids = t;
    s.labels = labels;
    s.nlabels = g.L;
    s.surface = 1;
    s.invert = 0;
    s.any_of = 0;
    const int lab = labels[l];
    const int *tb = t + (size_t)b * g.V;
    const float *db = d2 + (size_t)b * g.V * g.L + l;
    const unsigned beg = k * (unsigned)per, end = min((unsigned)g.V, beg + (unsigned)per);
    int cnt = 0;
    float mx = -INFINITY;
    double sum = 0.0;
    for (unsigned v = beg + threadIdx.x; v < end; v += kThreads) {
        if (tb[v] != lab || !edt_on_surface(s, g, tb, v, l)) continue;
        const float x2 = db[(size_t)v * g.L];
        const float d = sqrtf(x2);
        ++cnt;
        mx = fmaxf(mx, x2);
        sum += (double)d;
        if (hist && x2 >= 0.0f && x2 < (float)nbins) atomicAdd(hist + (size_t)bl * nbins + (unsigned)x2, 1u);
    }
    // lanes by xor shuffles, waves in wave order: a fixed order
    // (nrt_wave_sum / nrt_wave_max by hand, three chains in one loop: apart, the instruction count moves by 1.6 %)
    for (int off = 1; off < NRT_WAVE; off <<= 1) {
        cnt += __shfl_xor(cnt, off, NRT_WAVE);
        mx = fmaxf(mx, __shfl_xor(mx, off, NRT_WAVE));
        sum += __shfl_xor(sum, off, NRT_WAVE);
    }
    if ((threadIdx.x & (NRT_WAVE - 1)) == 0) {
        redi[threadIdx.x / NRT_WAVE] = cnt;
        redf[threadIdx.x / NRT_WAVE] = mx;
        red[threadIdx.x / NRT_WAVE] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < kWaves; ++wv) {
        cnt += redi[wv];
        mx = fmaxf(mx, redf[wv]);
        sum += red[wv];
    }
    unsigned *row = part + (size_t)blockIdx.x * kPartWords;
    row[0] = (unsigned)cnt;
    row[1] = __float_as_uint(mx);
    store_f64(row + 2, sum);
}

// one thread per (entry, label) adds its rows in block order.  stats [B * L][3] of 8 bytes: count (int64), max d2, sum of roots (float64)
__global__ void __launch_bounds__(kThreads)
surface_stats_finish(const unsigned *__restrict__ part, unsigned nbl, int nb, void *__restrict__ stats) {
    const unsigned bl = blockIdx.x * kThreads + threadIdx.x;
    if (bl >= nbl) return;
    const unsigned *row = part + (size_t)bl * nb * kPartWords;
    long long cnt = 0;
    float mx = -INFINITY;
    double sum = 0.0;
    for (int k = 0; k < nb; ++k, row += kPartWords) {
        cnt += (long long)row[0];
        mx = fmaxf(mx, __uint_as_float(row[1]));
        sum += load_f64(row + 2);
    }
    ((long long *)stats)[3 * (size_t)bl] = cnt;
    ((double *)stats)[3 * (size_t)bl + 1] = (double)mx;
    ((double *)stats)[3 * (size_t)bl + 2] = sum;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int edt_geom(int batch, const int *shape, int nd, int channels, EdtGeom &g) {
    if (!shape || batch < 1) return NRT_ERR_INVALID_ARG;
    if (nd != 2 && nd != 3) return NRT_ERR_UNSUPPORTED;
    for (int a = 0; a < nd; ++a)
        if (shape[a] < 1) return NRT_ERR_INVALID_ARG;
    if (channels < 1 || channels > kMaxLabels || batch > 65535) return NRT_ERR_UNSUPPORTED;
    long long V = 1;
    for (int a = 0; a < nd; ++a) {
        if (shape[a] > kMaxExtent) return NRT_ERR_UNSUPPORTED;
        V *= shape[a];                                                           // (at most 2^30)
    }
    if (V * batch * channels >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;         // (at most 2^30 * 65535 * 256 < 2^63)
    g.B = batch;
    g.nd = nd;
    for (int a = 0; a < 3; ++a) g.n[a] = a < nd ? shape[a] : 1;
    g.V = (int)V;
    g.L = channels;
    return NRT_OK;
}

inline int edt_run(const EdtSrc &src, const float *first, float *out, const EdtGeom &g, const float *s, int squared, hipStream_t st) {
    for (int a = 0; a < g.nd; ++a) {
        EdtPass p;
        p.n = g.n[a];
        long long outer = g.B, inner = g.L;
        for (int k = 0; k < a; ++k) outer *= g.n[k];
        for (int k = a + 1; k < g.nd; ++k) inner *= g.n[k];
        p.outer = (unsigned)outer;
        p.inner = (unsigned)inner;
        p.s = s[a];
        p.first = a == 0;
        p.last = a == g.nd - 1;
        p.squared = squared;
        const long long line = (long long)p.n * inner;
        unsigned grid;
        size_t lds;
        if (line <= kLdsFloats) {
            p.ti = 0;
            p.to = (unsigned)std::min<long long>(outer, std::max<long long>(1, kChunkFloats / line));
            p.tiles = 0;
            grid = (p.outer + p.to - 1) / p.to;
            lds = (size_t)p.to * (size_t)line * sizeof(float);
        } else {
            p.ti = p.n <= 256 ? 64 : p.n <= 512 ? 32 : 16;
            p.to = 0;
            p.tiles = (p.inner + (unsigned)p.ti - 1) / (unsigned)p.ti;
            grid = p.outer * p.tiles;                                            // (below the element count)
            lds = (size_t)p.n * p.ti * sizeof(float);
        }
        hipLaunchKernelGGL(edt_pass, dim3(grid), dim3(kEdtThreads), lds, st, src, p.last ? first : (const float *)nullptr, out, g, p);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}

inline void stats_runs(const EdtGeom &g, int &nb, int &per) {
    const long long V = g.V;
    const long long want = std::max(1LL, std::min((V + kRunVoxels - 1) / kRunVoxels, (long long)kMaxRuns));
    per = (int)((V + want - 1) / want);
    nb = (int)((V + per - 1) / per);
}

}  // namespace

// What a SIGNED nrt_edt_f32 of this geometry needs (one float volume of the output's size); 0 for a geometry the call refuses.
extern "C" size_t nrt_edt_workspace_bytes(int batch, const int *shape, int nd, int channels) {
    EdtGeom g;
    if (edt_geom(batch, shape, nd, channels, g) != NRT_OK) return 0;
    return (size_t)g.B * g.V * g.L * sizeof(float);
}

extern "C" int nrt_edt_f32(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int *shape, int nd,
                           const float *sampling, int flags, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!out || (mask != nullptr) == (ids != nullptr)) return NRT_ERR_INVALID_ARG;
    if (flags & ~(NRT_EDT_SURFACE | NRT_EDT_INVERT | NRT_EDT_SIGNED | NRT_EDT_SQUARED | NRT_EDT_ANY_OF)) return NRT_ERR_INVALID_ARG;
    const bool signed_ = flags & NRT_EDT_SIGNED, any_of = flags & NRT_EDT_ANY_OF, surface = flags & NRT_EDT_SURFACE;
    if (mask && (labels || nlabels != 1 || surface || any_of)) return NRT_ERR_INVALID_ARG;
    if (ids && !labels) return NRT_ERR_INVALID_ARG;
    if (surface && signed_) return NRT_ERR_INVALID_ARG;
    if (nlabels < 1 || nlabels > kMaxLabels) return NRT_ERR_UNSUPPORTED;
    EdtGeom g;
    const int rc = edt_geom(batch, shape, nd, any_of ? 1 : nlabels, g);
    if (rc != NRT_OK) return rc;
    float s[3] = {1.0f, 1.0f, 1.0f};
    for (int a = 0; sampling && a < nd; ++a) {
        if (!(sampling[a] > 0.0f) || !std::isfinite(sampling[a])) return NRT_ERR_INVALID_ARG;
        s[a] = sampling[a];
    }
    if (signed_ && (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < (size_t)g.B * g.V * g.L * sizeof(float)))
        return NRT_ERR_WORKSPACE;
    EdtSrc src;
    src.mask = (const unsigned char *)mask;
    src.ids = ids;
    src.labels = labels;
    src.nlabels = nlabels;
    src.surface = surface;
    src.invert = (flags & NRT_EDT_INVERT) != 0;
    src.any_of = any_of;
    hipStream_t st = nrt_stream(stream);
    const int squared = (flags & NRT_EDT_SQUARED) != 0;
    if (!signed_) return edt_run(src, nullptr, out, g, s, squared, st);
    // the set's own transform stays squared in the workspace; the complement's last pass combines the two
    const int rc1 = edt_run(src, nullptr, (float *)workspace, g, s, 1, st);
    if (rc1 != NRT_OK) return rc1;
    src.invert = !src.invert;
    return edt_run(src, (const float *)workspace, out, g, s, squared, st);
}

// What nrt_surface_stats_f32 of this geometry needs; 0 for a geometry the call refuses.
extern "C" size_t nrt_surface_stats_workspace_bytes(int batch, const int *shape, int nd, int nlabels) {
    EdtGeom g;
    if (edt_geom(batch, shape, nd, nlabels, g) != NRT_OK) return 0;
    int nb, per;
    stats_runs(g, nb, per);
    return (size_t)g.B * g.L * nb * kPartWords * sizeof(unsigned);
}

extern "C" int nrt_surface_stats_f32(const int *t, const int *labels, int nlabels, const float *d2, int batch, const int *shape, int nd,
                                     void *stats, unsigned *hist, long long nbins, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    if (!t || !labels || !d2 || !stats || ((uintptr_t)stats & 7) != 0) return NRT_ERR_INVALID_ARG;
    if (hist && nbins < 1) return NRT_ERR_INVALID_ARG;
    EdtGeom g;
    const int rc = edt_geom(batch, shape, nd, nlabels, g);
    if (rc != NRT_OK) return rc;
    if (hist && (nbins > (1LL << 24) || (long long)g.B * g.L * nbins >= (1LL << 31))) return NRT_ERR_UNSUPPORTED;
    int nb, per;
    stats_runs(g, nb, per);
    const size_t need = (size_t)g.B * g.L * nb * kPartWords * sizeof(unsigned);
    if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < need) return NRT_ERR_WORKSPACE;
    hipStream_t st = nrt_stream(stream);
    const unsigned nbl = (unsigned)(g.B * g.L);
    hipLaunchKernelGGL(surface_stats, dim3(nbl * (unsigned)nb), dim3(kThreads), 0, st, t, labels, d2, g, nb, per, (unsigned *)workspace,
                       hist, (unsigned)(hist ? nbins : 0));
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(surface_stats_finish, dim3((nbl + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                       (const unsigned *)workspace, nbl, nb, stats);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
