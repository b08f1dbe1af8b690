// Connected-component labelling of masks and label maps, and the mask clean-up built on it.  What it replaces: a copy of
// every volume to the host, scipy.ndimage.label / binary_fill_holes there, and a copy back.
//
// Input [B, *S], len(S) in {2, 3}: a uint8 mask (foreground = nonzero) or an int32 id map with a list of 1..256 label ids (ids outside
// the list are background).  Two neighbouring voxels (scipy's generate_binary_structure(nd, connectivity)) belong to one component when
// both are foreground and carry the same id.  Components of an entry are numbered 1, 2, ... in raster order of their first voxel:
// scipy.ndimage.label's numbering.  A 2-D volume is handled as [1, n0, n1].
//
// One union-find forest per batch entry on a global parent array (ccl_core.h), entry-local linear indices, -1 on the background:
//   init      parent[v] = the head of v's run of equal ids along the last axis (cut at the chunk seams); sizes zeroed
//   merge     every foreground voxel joins its backward neighbours (smaller linear index) with the same id, but for the unions that
//             the runs and the left neighbour's unions already imply (ccl_core.h: most of them)
//   flatten   parent[v] = root(v), and the representatives (parent[v] == v) of each 1024-voxel chunk are counted
//   scan      one block per entry turns the chunk counts into exclusive offsets and writes the entry's component count
//   number    representatives get 1 + offset + rank within the chunk, the background 0
//   spread    every other foreground voxel copies the number of its representative
// and for the statistics and the selection, after flatten:
//   sizes     size[rep] += run length (integer adds: runs of equal representatives summed per wave, the dominant one per block in LDS),
//             bit 31 = touches the border
//   reps      per (entry, label slot): the number of representatives and the 64-bit maximum of (size << 32 | ~rep)
//   select    a voxel is kept when its component passes every test the mode asks for
// Each phase is a launch of its own.  Within merge and flatten the parent words are shared between workgroups and touched by
// agent-scope atomics only; no workgroup waits for another (no flag, no spin, no ticket), and every loop ends by itself because a
// parent word only decreases (ccl_core.h).  Every other pass reads what an earlier launch finished.  The final parent array does not
// depend on the schedule (the root is the component's smallest index), the sums and maxima are integer, so the results are
// bit-identical run to run.  No host synchronisation, no allocation: the calls capture into a graph.
#include "wave_ops.h"

#include "ccl_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kChunk = 1024;                         // voxels of a block: kChunk / kThreads rounds of one voxel per thread
constexpr int kMaxLabels = 256;
constexpr int kSizeChunks = 8;                        // chunks of a block of ccl_sizes
constexpr int kMaxBatch = 65535;                     // keeps B * nchunks * kThreads below 2^32
constexpr unsigned kBorderBit = 0x80000000u;
constexpr int kAllModes = NRT_CCL_LARGEST | NRT_CCL_MIN_SIZE | NRT_CCL_BORDER_FREE | NRT_CCL_INVERT;

struct CclDevMem {
    static __device__ __forceinline__ int load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int fetch_min(int *p, int v) { return atomicMin(p, v); }
};

struct CclGeom {
    int B, nd;
    int n[3];                                        // extents, a 2-D volume padded in front with 1
    int V, L;                                        // voxels of an entry; label slots (1 for a mask)
    int nchunks;                                     // blocks per entry
};

struct CclSrc {
    const unsigned char *mask;                       // [B, V], or
    const int *ids;                                  // [B, V] with
    const int *labels;                               // [nlabels]
    int nlabels, invert;
};

// what two neighbours must share: the id, or for a mask whether the voxel is in the set
__device__ __forceinline__ int ccl_key(const CclSrc &s, unsigned e) {
    return s.mask ? (int)((s.mask[e] != 0) != (s.invert != 0)) : s.ids[e];
}

__device__ __forceinline__ void ccl_load_labels(const CclSrc &s, int *lab) {
    if (s.ids)
        for (int k = threadIdx.x; k < s.nlabels; k += kThreads) lab[k] = s.labels[k];
    __syncthreads();
}

// the slot of a key: 0 or -1 for a mask, the position in the label list or -1 for an id
__device__ __forceinline__ int ccl_slot(const CclSrc &s, const int *lab, int key) {
    if (s.mask) return key ? 0 : -1;
    int slot = -1;
    for (int k = 0; k < s.nlabels; ++k) slot = lab[k] == key ? k : slot;
    return slot;
}

// block b of the grid works on voxels [v0, v0 + kChunk) of entry `entry`
__device__ __forceinline__ void ccl_block(const CclGeom &g, unsigned &entry, unsigned &v0) {
    entry = blockIdx.x / (unsigned)g.nchunks;
    v0 = (blockIdx.x - entry * (unsigned)g.nchunks) * (unsigned)kChunk;
}

// inclusive maximum of x over the threads of the block up to this one; every thread of the block calls it
__device__ __forceinline__ int ccl_block_scan_max(int x, int *red) {
    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    x = nrt_wave_scan_incl(x, lane, nrt_op_max());
    __syncthreads();
    if (lane == NRT_WAVE - 1) red[wave] = x;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) x = max(x, red[w]);
    return x;
}

// parent[v] = the head of v's run (ccl_core.h) on the foreground, -1 elsewhere: the latest head at or in front of v, by a maximum scan
// over the block's voxels in raster order.  The block's first voxel is a head, so the scan never looks outside the chunk.
__global__ void __launch_bounds__(kThreads)
ccl_init(CclSrc src, CclGeom g, int *__restrict__ parent, unsigned *__restrict__ size) {
    __shared__ int lab[kMaxLabels];
    __shared__ int red[kWaves];
    ccl_load_labels(src, lab);
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    int carry = -1;
    for (unsigned r0 = v0; r0 < v0 + kChunk; r0 += kThreads) {                       // (uniform: every thread takes part in the scan)
        const unsigned v = r0 + threadIdx.x;
        const bool in = v < (unsigned)g.V;
        int key = 0, head = -1;
        if (in) {
            key = ccl_key(src, base + v);
            const int i2 = (int)(v % (unsigned)g.n[2]);
            if (ccl_is_run_head((int)v, i2, kChunk, v > 0 && ccl_key(src, base + v - 1) == key)) head = (int)v;
        }
        const int start = max(carry, ccl_block_scan_max(head, red));
        __syncthreads();
        if (threadIdx.x == kThreads - 1) red[0] = start;
        __syncthreads();
        carry = red[0];
        if (in) {
            parent[base + v] = ccl_slot(src, lab, key) >= 0 ? start : -1;
            size[base + v] = 0u;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
ccl_merge(CclSrc src, CclGeom g, int connectivity, int *parent) {
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    int *pe = parent + base;
    const auto key_of = [&](int u) { return ccl_key(src, base + (unsigned)u); };
    const auto join = [&](int a, int b) { ccl_union<CclDevMem>(pe, a, b); };
    for (unsigned v = v0 + threadIdx.x; v < v0 + kChunk && v < (unsigned)g.V; v += kThreads) {
        if (CclDevMem::load(pe + v) < 0) continue;
        ccl_for_each_union((int)v, g.n, connectivity, kChunk, key_of, join);
    }
}

// exclusive prefix of x over the threads of the block, and the block's total; every thread of the block calls it
__device__ __forceinline__ int ccl_block_scan(int x, int *red, int &total) {
    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    const int incl = nrt_wave_scan_incl(x, lane, nrt_op_sum());
    __syncthreads();
    if (lane == NRT_WAVE - 1) red[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? red[w] : 0;
        total += red[w];
    }
    return before + incl - x;
}

__global__ void __launch_bounds__(kThreads)
ccl_flatten(CclGeom g, int *parent, int *__restrict__ counts) {
    __shared__ int red[kWaves];
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    int *pe = parent + entry * (unsigned)g.V;
    int reps = 0;
    for (unsigned v = v0 + threadIdx.x; v < v0 + kChunk && v < (unsigned)g.V; v += kThreads) {
        if (CclDevMem::load(pe + v) < 0) continue;
        const int r = ccl_find_compress<CclDevMem>(pe, (int)v);
        reps += r == (int)v;
    }
    reps = nrt_block_sum<kWaves>(reps, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = reps;
}

// one block per entry: counts [B, nchunks] -> exclusive offsets in place, the total to count[entry]
__global__ void __launch_bounds__(kThreads)
ccl_scan(CclGeom g, int *__restrict__ counts, int *__restrict__ count) {
    __shared__ int red[kWaves];
    int *row = counts + (size_t)blockIdx.x * g.nchunks;
    int carry = 0;
    for (int k0 = 0; k0 < g.nchunks; k0 += kThreads) {
        const int k = k0 + (int)threadIdx.x;
        const int x = k < g.nchunks ? row[k] : 0;
        int total;
        const int before = ccl_block_scan(x, red, total);
        if (k < g.nchunks) row[k] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0 && count) count[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kThreads)
ccl_number(CclGeom g, const int *__restrict__ parent, const int *__restrict__ offsets, int *__restrict__ out) {
    __shared__ int red[kWaves];
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    int next = 1 + offsets[blockIdx.x];
    for (unsigned r0 = v0; r0 < v0 + kChunk; r0 += kThreads) {                       // (uniform: every thread takes part in the scan)
        const unsigned v = r0 + threadIdx.x;
        const bool in = v < (unsigned)g.V;
        const int p = in ? parent[base + v] : -1;
        const int rep = in && ccl_is_representative(parent + base, (int)v);
        int total;
        const int before = ccl_block_scan(rep, red, total);
        if (rep) out[base + v] = next + before;
        else if (p < 0 && in) out[base + v] = 0;
        next += total;
    }
}

__global__ void __launch_bounds__(kThreads)
ccl_spread(CclGeom g, const int *__restrict__ parent, int *out) {
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    for (unsigned v = v0 + threadIdx.x; v < v0 + kChunk && v < (unsigned)g.V; v += kThreads) {
        const int p = parent[base + v];
        if (p >= 0 && p != (int)v) out[base + v] = out[base + (unsigned)p];           // (a representative's word: written by ccl_number)
    }
}

// Runs of equal representatives along a wave are added up by shuffles first; then the most frequent representative of each chunk (the
// one with the longest such run) is added up in LDS, and carried from chunk to chunk while it stays the same: a block takes
// kSizeChunks chunks, so a component that fills the volume costs one global add per 8192 voxels, not one per wave.  Adds to ONE
// address serialise in the memory system (about 30 ns each, measured: 124 us for the 4000 block sums of a 160^3 volume).
__global__ void __launch_bounds__(kThreads)
ccl_sizes(CclGeom g, const int *__restrict__ parent, unsigned *__restrict__ size) {
    constexpr int kRounds = kChunk / kThreads;
    __shared__ unsigned long long hot;               // (longest run << 32) | its representative, of the chunk at hand
    __shared__ int cur;                              // the representative whose voxels hot_size holds, or -1
    __shared__ unsigned hot_size;
    const unsigned nsuper = ((unsigned)g.nchunks + kSizeChunks - 1) / kSizeChunks;
    const unsigned entry = blockIdx.x / nsuper, first = (blockIdx.x - entry * nsuper) * kSizeChunks;
    const unsigned base = entry * (unsigned)g.V;
    const int lane = threadIdx.x & (NRT_WAVE - 1);
    if (threadIdx.x == 0) {
        cur = -1;
        hot_size = 0u;
    }
    for (unsigned chunk = first; chunk < first + kSizeChunks && chunk < (unsigned)g.nchunks; ++chunk) {       // (uniform)
        const unsigned v0 = chunk * (unsigned)kChunk;
        if (threadIdx.x == 0) hot = 0ull;
        __syncthreads();
        int rep[kRounds];                            // the representative where this lane heads a run, else -1
        unsigned add[kRounds];                       // the run's voxels, bit 31: it touches the border
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {                                          // (uniform: every lane takes part in the shuffles)
            const unsigned v = v0 + (unsigned)k * kThreads + threadIdx.x;
            const int r = v < (unsigned)g.V ? parent[base + v] : -1;
            int cnt = r >= 0, border = 0;
            if (r >= 0) {
                const unsigned q = v / (unsigned)g.n[2];
                const int i2 = (int)(v - q * (unsigned)g.n[2]);
                const int i0 = (int)(q / (unsigned)g.n[1]);
                const int i1 = (int)(q - (unsigned)i0 * (unsigned)g.n[1]);
                border = i2 == 0 || i2 == g.n[2] - 1 || i1 == 0 || i1 == g.n[1] - 1 || (g.nd == 3 && (i0 == 0 || i0 == g.n[0] - 1));
            }
            const int prev = __shfl_up(r, 1, NRT_WAVE);
            const bool head = lane == 0 || prev != r;
            const unsigned long long heads = __ballot(head);
            const int run = __popcll(heads & ((2ull << lane) - 1ull));
            for (int off = 1; off < NRT_WAVE; off <<= 1) {
                const int oc = __shfl_down(cnt, off, NRT_WAVE), ob = __shfl_down(border, off, NRT_WAVE);
                const int orun = __shfl_down(run, off, NRT_WAVE);
                if (lane + off < NRT_WAVE && orun == run) {
                    cnt += oc;
                    border |= ob;
                }
            }
            rep[k] = head ? r : -1;
            add[k] = (unsigned)cnt | (border ? kBorderBit : 0u);
            if (rep[k] >= 0) atomicMax(&hot, ((unsigned long long)cnt << 32) | (unsigned)r);
        }
        __syncthreads();
        const int hot_rep = hot != 0ull ? (int)(unsigned)hot : -1;
        if (threadIdx.x == 0 && hot_rep >= 0 && hot_rep != cur) {                    // another component takes the LDS word: flush
            if (cur >= 0) {
                atomicAdd(size + base + (unsigned)cur, hot_size & ~kBorderBit);
                if (hot_size & kBorderBit) atomicOr(size + base + (unsigned)cur, kBorderBit);
            }
            cur = hot_rep;
            hot_size = 0u;
        }
        __syncthreads();
        const int held = cur;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            if (rep[k] < 0) continue;
            unsigned *word = rep[k] == held ? &hot_size : size + base + (unsigned)rep[k];
            atomicAdd(word, add[k] & ~kBorderBit);
            if (add[k] & kBorderBit) atomicOr(word, kBorderBit);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && cur >= 0) {
        atomicAdd(size + base + (unsigned)cur, hot_size & ~kBorderBit);
        if (hot_size & kBorderBit) atomicOr(size + base + (unsigned)cur, kBorderBit);
    }
}

__global__ void __launch_bounds__(kThreads)
ccl_reps(CclSrc src, CclGeom g, const int *__restrict__ parent, const unsigned *__restrict__ size, int *__restrict__ ncomp,
         unsigned long long *__restrict__ best) {
    __shared__ int lab[kMaxLabels];
    __shared__ int cnt[kMaxLabels];
    __shared__ unsigned long long top[kMaxLabels];
    for (int k = threadIdx.x; k < g.L; k += kThreads) {
        cnt[k] = 0;
        top[k] = 0ull;
    }
    ccl_load_labels(src, lab);
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    for (unsigned v = v0 + threadIdx.x; v < v0 + kChunk && v < (unsigned)g.V; v += kThreads) {
        if (parent[base + v] != (int)v) continue;
        const int slot = ccl_slot(src, lab, ccl_key(src, base + v));
        const unsigned long long packed = ((unsigned long long)(size[base + v] & ~kBorderBit) << 32) | (unsigned long long)(~v);
        atomicAdd(cnt + slot, 1);
        atomicMax(top + slot, packed);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < g.L; k += kThreads) {
        if (cnt[k] == 0) continue;
        atomicAdd(ncomp + entry * (unsigned)g.L + k, cnt[k]);
        atomicMax(best + entry * (unsigned)g.L + k, top[k]);
    }
}

__global__ void __launch_bounds__(kThreads)
ccl_table(int n, const int *__restrict__ ncomp, const unsigned long long *__restrict__ best, int *__restrict__ table) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    table[2 * i] = ncomp[i];
    table[2 * i + 1] = (int)(best[i] >> 32);
}

__global__ void __launch_bounds__(kThreads)
ccl_select(CclSrc src, CclGeom g, const int *__restrict__ parent, const unsigned *__restrict__ size,
           const unsigned long long *__restrict__ best, int mode, unsigned min_size, int fill, unsigned char *__restrict__ out_mask,
           int *__restrict__ out_ids) {
    __shared__ int lab[kMaxLabels];
    ccl_load_labels(src, lab);
    unsigned entry, v0;
    ccl_block(g, entry, v0);
    const unsigned base = entry * (unsigned)g.V;
    for (unsigned v = v0 + threadIdx.x; v < v0 + kChunk && v < (unsigned)g.V; v += kThreads) {
        const unsigned e = base + v;
        const int r = parent[e];
        const int key = ccl_key(src, e);
        bool keep = r >= 0;
        if (keep) {
            const unsigned w = size[base + (unsigned)r];
            if (mode & NRT_CCL_MIN_SIZE) keep = keep && (w & ~kBorderBit) >= min_size;
            if (mode & NRT_CCL_BORDER_FREE) keep = keep && (w & kBorderBit) == 0u;
            if (mode & NRT_CCL_LARGEST) {
                const int slot = ccl_slot(src, lab, key);
                keep = keep && ~(unsigned)best[entry * (unsigned)g.L + (unsigned)slot] == (unsigned)r;
            }
        }
        if (out_mask) out_mask[e] = (unsigned char)(r >= 0 ? keep : (src.invert != 0));
        else out_ids[e] = (r >= 0 && !keep) ? fill : key;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct CclPlan {
    CclGeom g;
    size_t words_parent, off_size, off_counts, off_ncomp, off_best, words;           // offsets in 4-byte words; off_best is even
};

// the checks every entry point shares, in the order the header promises
inline int ccl_check_source(const void *mask, const int *ids, const int *labels, int nlabels) {
    if ((mask != nullptr) == (ids != nullptr)) return NRT_ERR_INVALID_ARG;
    if (ids && !labels) return NRT_ERR_INVALID_ARG;
    if (mask && (labels || nlabels != 1)) return NRT_ERR_INVALID_ARG;
    return NRT_OK;
}

inline int ccl_plan(int nlabels, int batch, const int *shape, int nd, int connectivity, CclPlan &p) {
    if (!shape || batch < 1 || (nd != 2 && nd != 3)) return NRT_ERR_INVALID_ARG;
    for (int a = 0; a < nd; ++a)
        if (shape[a] < 1) return NRT_ERR_INVALID_ARG;
    if (connectivity < 1 || connectivity > nd || nlabels < 1 || nlabels > kMaxLabels) return NRT_ERR_INVALID_ARG;
    if (batch > kMaxBatch) return NRT_ERR_UNSUPPORTED;
    long long V = 1;
    for (int a = 0; a < nd; ++a) {
        V *= shape[a];                                                           // (below 2^31 * 2^31 at every step)
        if (V >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    }
    if (V * batch >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    CclGeom &g = p.g;
    g.B = batch;
    g.nd = nd;
    g.n[0] = nd == 3 ? shape[0] : 1;
    g.n[1] = shape[nd - 2];
    g.n[2] = shape[nd - 1];
    g.V = (int)V;
    g.L = nlabels;
    g.nchunks = (int)((V + kChunk - 1) / kChunk);
    const size_t N = (size_t)batch * (size_t)V, BL = (size_t)batch * nlabels;
    p.words_parent = N;
    p.off_size = N;
    p.off_counts = 2 * N;
    p.off_ncomp = p.off_counts + (size_t)batch * g.nchunks;
    p.off_best = (p.off_ncomp + BL + 1) & ~(size_t)1;
    p.words = p.off_best + 2 * BL;
    return NRT_OK;
}

inline bool ccl_workspace_ok(const CclPlan &p, const void *ws, size_t bytes) {
    return ws && ((uintptr_t)ws & 7) == 0 && bytes >= p.words * sizeof(int);
}

// init, merge, flatten: leaves the flattened forest in the workspace, the chunk counts behind it, and the small tables zeroed
inline int ccl_forest(const CclSrc &src, const CclPlan &p, int connectivity, void *ws, hipStream_t st) {
    int *w = (int *)ws;
    const dim3 grid((unsigned)p.g.B * (unsigned)p.g.nchunks), block(kThreads);
    if (nrt_zero_async(w + p.off_counts, (p.words - p.off_counts) * sizeof(int), st) != hipSuccess) return NRT_ERR_LAUNCH;
    hipLaunchKernelGGL(ccl_init, grid, block, 0, st, src, p.g, w, (unsigned *)(w + p.off_size));
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_merge, grid, block, 0, st, src, p.g, connectivity, w);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_flatten, grid, block, 0, st, p.g, w, w + p.off_counts);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

}  // namespace

// What nrt_ccl_label_i32 / nrt_ccl_select of this geometry need; 0 for a geometry the calls refuse.
extern "C" size_t nrt_ccl_workspace_bytes(int batch, const int *shape, int nd, int nlabels) {
    CclPlan p;
    if (ccl_plan(nlabels, batch, shape, nd, 1, p) != NRT_OK) return 0;
    return p.words * sizeof(int);
}

extern "C" int nrt_ccl_label_i32(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int *shape, int nd,
                                 int connectivity, int *components, int *count, void *workspace, size_t workspace_bytes, void *stream) {
    if (!components || !count) return NRT_ERR_INVALID_ARG;
    const int rs = ccl_check_source(mask, ids, labels, nlabels);
    if (rs != NRT_OK) return rs;
    CclPlan p;
    const int rc = ccl_plan(nlabels, batch, shape, nd, connectivity, p);
    if (rc != NRT_OK) return rc;
    if (!ccl_workspace_ok(p, workspace, workspace_bytes)) return NRT_ERR_WORKSPACE;
    const CclSrc src = {(const unsigned char *)mask, ids, labels, nlabels, 0};
    hipStream_t st = nrt_stream(stream);
    const int rf = ccl_forest(src, p, connectivity, workspace, st);
    if (rf != NRT_OK) return rf;
    int *w = (int *)workspace;
    const dim3 grid((unsigned)p.g.B * (unsigned)p.g.nchunks), block(kThreads);
    hipLaunchKernelGGL(ccl_scan, dim3((unsigned)p.g.B), block, 0, st, p.g, w + p.off_counts, count);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_number, grid, block, 0, st, p.g, (const int *)w, (const int *)(w + p.off_counts), components);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_spread, grid, block, 0, st, p.g, (const int *)w, components);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}

extern "C" int nrt_ccl_select(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int *shape, int nd,
                              int connectivity, int mode, int min_size, int fill, int *table, void *out, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (!table && !out) return NRT_ERR_INVALID_ARG;
    if ((mode & ~kAllModes) != 0 || min_size < 0 || ((mode & NRT_CCL_INVERT) && !mask)) return NRT_ERR_INVALID_ARG;
    const int rs = ccl_check_source(mask, ids, labels, nlabels);
    if (rs != NRT_OK) return rs;
    CclPlan p;
    const int rc = ccl_plan(nlabels, batch, shape, nd, connectivity, p);
    if (rc != NRT_OK) return rc;
    if (!ccl_workspace_ok(p, workspace, workspace_bytes)) return NRT_ERR_WORKSPACE;
    const CclSrc src = {(const unsigned char *)mask, ids, labels, nlabels, (mode & NRT_CCL_INVERT) != 0};
    hipStream_t st = nrt_stream(stream);
    const int rf = ccl_forest(src, p, connectivity, workspace, st);
    if (rf != NRT_OK) return rf;
    int *w = (int *)workspace;
    const unsigned *size = (const unsigned *)(w + p.off_size);
    int *ncomp = w + p.off_ncomp;
    unsigned long long *best = (unsigned long long *)(w + p.off_best);
    const dim3 grid((unsigned)p.g.B * (unsigned)p.g.nchunks), block(kThreads);
    const unsigned nsuper = ((unsigned)p.g.nchunks + kSizeChunks - 1) / kSizeChunks;
    hipLaunchKernelGGL(ccl_sizes, dim3((unsigned)p.g.B * nsuper), block, 0, st, p.g, (const int *)w, (unsigned *)(w + p.off_size));
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_reps, grid, block, 0, st, src, p.g, (const int *)w, size, ncomp, best);
    NRT_CHECK_LAUNCH();
    if (table) {
        const int n = p.g.B * p.g.L;
        hipLaunchKernelGGL(ccl_table, dim3((unsigned)(n + kThreads - 1) / kThreads), block, 0, st, n, (const int *)ncomp,
                           (const unsigned long long *)best, table);
        NRT_CHECK_LAUNCH();
    }
    if (out) {
        hipLaunchKernelGGL(ccl_select, grid, block, 0, st, src, p.g, (const int *)w, size, (const unsigned long long *)best, mode,
                           (unsigned)min_size, fill, mask ? (unsigned char *)out : (unsigned char *)nullptr,
                           mask ? (int *)nullptr : (int *)out);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}
