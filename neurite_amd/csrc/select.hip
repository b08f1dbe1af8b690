// Exact percentiles of every batch entry of a volume, and the percentile intensity normalisation built on them.  What
// they replace: torch.quantile (a sort of every volume and a sorted copy, no mask) or a round trip through the host.
//
// x [B, V] float32, bfloat16 or float16, an optional uint8 mask [B, V]; up to 8 fractions f per call.  The population of an entry is
// its selected and, with NRT_PCT_IGNORE_NAN, non-NaN elements, n of them; pos = (n - 1) f in float64, and the result is formed from the
// order statistics of ranks floor(pos) and ceil(pos) (include/neurite_amd.h).  An order statistic needs no sort: a radix select on the
// monotone key of the floats (select_core.h) finds it in three counting passes, 12 + 10 + 10 key bits from the top:
//   hist 0    every block counts the first digit of its share of an entry in 4096 LDS counters and adds the counters that are not zero
//             to the entry's global row
//   scan 0    one block per entry: the population from the row's total and its NaN bin, the ranks from it, and per rank the bin that
//             holds it and the rank that remains inside the bin; equal prefixes share a slot (at most 16 slots)
//   hist 1, 2 as hist 0 on the next digit, 1024 counters per slot, of the elements whose higher key bits equal a slot's prefix
//   scan 1, 2 as scan 0 on the slot rows; the last one turns the keys back into floats and writes the results
// A float stored in 16 bits has no third digit (select_core.h): two passes.  All counters are integers, added by vector atomics on
// unsigned words, so the results do not depend on the schedule: bit-identical run to run.  No workgroup waits for another, nothing
// goes to the host, nothing is allocated: the calls capture into a graph.
//
// Hot bins.  A brain volume is 70 % exact zeros and a constant image is legal: nearly every increment then goes to ONE counter, and
// adds of one wave to one LDS address are carried out one after the other.  sel_add therefore adds per wave: the lanes that hold the
// code of the first active lane are counted by a ballot and added once, twice over (the hot code is missed both times with
// probability 0.09 at 70 % zeros), and only what is left goes lane by lane.
#include "wave_ops.h"

#include "select_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NRT_WAVE;
constexpr int kMaxQ = 8;
constexpr int kMaxRanks = 2 * kMaxQ;
constexpr int kMaxBatch = 65535;                     // gridDim.y
constexpr unsigned kNone = 0xFFFFFFFFu;              // no counter: not selected, or no slot has the element's prefix
constexpr int kBlockElems = 8192;                    // the least share of a block
constexpr int kTargetBlocks = 1024;                  // about that many blocks in a launch

// the table of an entry in the workspace, in words
constexpr int kTabSlots = 0;                         // live slots
constexpr int kTabCount = 1;                         // the population n
constexpr int kTabNan = 2;                           // 1: the results are NaN (an empty population, or a NaN in it without IGNORE_NAN)
constexpr int kTabSlotPrefix = 4;                    // [16] the prefix of each slot
constexpr int kTabRankSlot = 20;                     // [16] the slot of each rank
constexpr int kTabRankRem = 36;                      // [16] the rank that remains inside the prefix
constexpr int kTabWords = 52;

struct SelGeom {
    unsigned V;                                      // elements of an entry
    unsigned per;                                    // elements of a block's share
    int vec;                                         // x and mask allow 4-element loads at element indices that are multiples of 4
    int nranks;                                      // 2 * nq
};

struct SelFractions {
    double f[kMaxQ];
};

// ---- loads ----------------------------------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ unsigned sel_bits(const void *x, unsigned g) {
    if (DT == NRT_DT_F32) return ((const unsigned *)x)[g];
    const unsigned short h = ((const unsigned short *)x)[g];
    if (DT == NRT_DT_BF16) return (unsigned)h << 16;
    return __float_as_uint((float)__builtin_bit_cast(_Float16, h));
}

template <int DT>
__device__ __forceinline__ void sel_bits4(const void *x, unsigned g, unsigned *b) {
    if (DT == NRT_DT_F32) {
        const nrt_i4 v = *(const nrt_i4 *)((const unsigned *)x + g);
        b[0] = (unsigned)v.x, b[1] = (unsigned)v.y, b[2] = (unsigned)v.z, b[3] = (unsigned)v.w;
        return;
    }
    typedef unsigned sel_u2 __attribute__((ext_vector_type(2)));
    const sel_u2 v = *(const sel_u2 *)((const unsigned short *)x + g);
    const unsigned short h[4] = {(unsigned short)(v.x & 0xFFFFu), (unsigned short)(v.x >> 16), (unsigned short)(v.y & 0xFFFFu),
                                 (unsigned short)(v.y >> 16)};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        b[k] = DT == NRT_DT_BF16 ? (unsigned)h[k] << 16 : __float_as_uint((float)__builtin_bit_cast(_Float16, h[k]));
}

// A block's share [beg, end) of an entry as global element ranges: [a0, a1) and [t0, t1) one element at a time, [a1, t0) in aligned fours
struct SelRange {
    unsigned a0, a1, t0, t1;
};

__device__ __forceinline__ SelRange sel_range(const SelGeom &g) {
    const unsigned beg = min(blockIdx.x * g.per, g.V), end = min(beg + g.per, g.V);          // (blockIdx.x * per < V + per < 2^32)
    const unsigned base = blockIdx.y * g.V;
    SelRange r;
    r.a0 = base + beg;
    r.t1 = base + end;
    r.a1 = g.vec ? min((r.a0 + 3u) & ~3u, r.t1) : r.t1;
    r.t0 = g.vec ? max(r.t1 & ~3u, r.a1) : r.t1;
    return r;
}

// ---- counting -------------------------------------------------------------------------------------------------------------------------
// counter[code] += 1 for every lane with a code; every lane of the wave calls it
__device__ __forceinline__ void sel_add(unsigned *counter, unsigned code, int lane) {
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const unsigned long long active = __ballot(code != kNone);
        if (active == 0ull) return;                                                  // (uniform)
        const int leader = __ffsll(active) - 1;
        const unsigned lead = __shfl(code, leader, NRT_WAVE);
        const unsigned long long same = __ballot(code == lead);
        if (lane == leader) atomicAdd(counter + lead, (unsigned)__popcll(same));
        if (code == lead) code = kNone;
    }
    if (code != kNone) atomicAdd(counter + code, 1u);
}

struct SelSlots {
    int n;
    unsigned prefix[kMaxRanks];
};

// the counter of a key: its digit in pass 0, later slot * 1024 + digit where a slot has the key's higher bits
template <int PASS>
__device__ __forceinline__ unsigned sel_code(unsigned bits, bool selected, const SelSlots &s) {
    const unsigned key = sel_key(bits);
    if (PASS == 0) return selected ? sel_digit(key, 0) : kNone;
    const unsigned above = sel_above(key, PASS);
    unsigned code = kNone;
#pragma unroll
    for (int k = 0; k < kMaxRanks; ++k)
        if (k < s.n && above == s.prefix[k]) code = (unsigned)k * kSelBins + sel_digit(key, PASS);
    return selected ? code : kNone;
}

// grid (blocks of an entry, B); dynamic LDS: 4096 words in pass 0, nranks * 1024 later
template <int DT, int PASS>
__global__ void __launch_bounds__(kThreads)
sel_hist(const void *__restrict__ x, const unsigned char *__restrict__ mask, SelGeom g, const unsigned *__restrict__ table,
         unsigned *__restrict__ rows) {
    extern __shared__ unsigned counter[];
    SelSlots s;
    s.n = 0;
    if (PASS > 0) {
        const unsigned *tab = table + (size_t)blockIdx.y * kTabWords;
        s.n = (int)tab[kTabSlots];
        if (s.n == 0) return;                                                        // (uniform: an empty population)
#pragma unroll
        for (int k = 0; k < kMaxRanks; ++k) s.prefix[k] = tab[kTabSlotPrefix + k];
    }
    const int ncounters = PASS == 0 ? kSelBins0 : s.n * kSelBins;
    for (int i = threadIdx.x; i < ncounters; i += kThreads) counter[i] = 0u;
    __syncthreads();
    const SelRange r = sel_range(g);
    const int lane = threadIdx.x & (NRT_WAVE - 1);
    const unsigned wave0 = (threadIdx.x / NRT_WAVE) * NRT_WAVE;
    // (the loops are uniform per wave: every lane takes part in the ballots of sel_add)
    for (unsigned q0 = r.a1 + 4u * wave0; q0 < r.t0; q0 += 4u * kThreads) {
        const unsigned q = q0 + 4u * (unsigned)lane;
        unsigned code[4] = {kNone, kNone, kNone, kNone};
        if (q < r.t0) {
            unsigned b[4];
            sel_bits4<DT>(x, q, b);
            const unsigned m = mask ? *(const unsigned *)(mask + q) : 0x01010101u;
#pragma unroll
            for (int k = 0; k < 4; ++k) code[k] = sel_code<PASS>(b[k], ((m >> (8 * k)) & 0xFFu) != 0u, s);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sel_add(counter, code[k], lane);
    }
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const unsigned from = part == 0 ? r.a0 : r.t0, to = part == 0 ? r.a1 : r.t1;
        for (unsigned e0 = from + wave0; e0 < to; e0 += kThreads) {
            const unsigned e = e0 + (unsigned)lane;
            unsigned code = kNone;
            if (e < to) code = sel_code<PASS>(sel_bits<DT>(x, e), mask ? mask[e] != 0 : true, s);
            sel_add(counter, code, lane);
        }
    }
    __syncthreads();
    unsigned *row = rows + (size_t)blockIdx.y * (PASS == 0 ? (size_t)kSelBins0 : (size_t)g.nranks * kSelBins);
    for (int i = threadIdx.x; i < ncounters; i += kThreads) {
        const unsigned c = counter[i];
        if (c != 0u) atomicAdd(row + i, c);
    }
}

// ---- ranks ----------------------------------------------------------------------------------------------------------------------------
// exclusive prefix of x over the threads of the block, and the block's total; every thread of the block calls it
__device__ __forceinline__ unsigned sel_block_scan(unsigned x, unsigned *red, unsigned &total) {
    const int lane = threadIdx.x & (NRT_WAVE - 1), wave = threadIdx.x / NRT_WAVE;
    const unsigned incl = nrt_wave_scan_incl(x, lane, nrt_op_sum());
    __syncthreads();
    if (lane == NRT_WAVE - 1) red[wave] = incl;
    __syncthreads();
    unsigned before = 0u;
    total = 0u;
    for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? red[w] : 0u;
        total += red[w];
    }
    return before + incl - x;
}

// sel_walk over a row of PER * kThreads counters by the whole block: the one thread whose PER counters hold the rank writes
// found[0] = bin, found[1] = the rank inside the bin.  Returns the row's total.  Every thread of the block calls it.
template <int PER>
__device__ __forceinline__ unsigned sel_block_walk(const unsigned *row, unsigned rank, unsigned *red, unsigned *found) {
    unsigned c[PER], sum = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        c[k] = row[threadIdx.x * PER + k];
        sum += c[k];
    }
    unsigned total;
    const unsigned before = sel_block_scan(sum, red, total);
    if (rank >= before && rank - before < sum) {
        unsigned bin = 0u, rem = 0u;
        sel_walk(c, PER, rank - before, &bin, &rem);
        found[0] = threadIdx.x * PER + bin;
        found[1] = rem;
    }
    __syncthreads();
    return total;
}

struct SelOut {
    float *out, *lower, *upper;                      // [B, nq]; lower and upper may be NULL
    int *count;                                      // [B] or NULL
};

// One block per entry.  PASS 0 forms the ranks; every pass extends each rank's prefix by the digit that holds it; the pass that is the
// call's last writes the results, the others share out the slots for the next hist launch and leave the slot rows zeroed.
template <int PASS>
__global__ void __launch_bounds__(kThreads)
sel_scan(SelGeom g, SelFractions fr, int method, int flags, int last, unsigned *__restrict__ table, unsigned *__restrict__ rows0,
         unsigned *__restrict__ rows, SelOut o) {
    __shared__ unsigned red[kWaves];
    __shared__ unsigned found[2];
    __shared__ unsigned prefix[kMaxRanks], rem[kMaxRanks], slot[kMaxRanks];
    __shared__ unsigned head[4];
    unsigned *tab = table + (size_t)blockIdx.x * kTabWords;
    unsigned *slot_rows = rows + (size_t)blockIdx.x * (size_t)g.nranks * kSelBins;
    const int nq = g.nranks / 2;
    if (PASS == 0) {
        const unsigned *row = rows0 + (size_t)blockIdx.x * kSelBins0;
        if (threadIdx.x < 2) found[threadIdx.x] = 0u;
        const unsigned total = sel_block_walk<kSelBins0 / kThreads>(row, kNone, red, found);      // (no rank: the total only)
        if (threadIdx.x == 0) {
            const unsigned nan = row[kSelNanBin];
            const unsigned n = (flags & NRT_PCT_IGNORE_NAN) ? total - nan : total;
            head[kTabCount] = n;
            head[kTabNan] = (n == 0u || (!(flags & NRT_PCT_IGNORE_NAN) && nan != 0u)) ? 1u : 0u;
            for (int j = 0; j < nq; ++j) {
                const double pos = (double)(n == 0u ? 0u : n - 1u) * fr.f[j];
                rem[2 * j] = (unsigned)floor(pos);
                rem[2 * j + 1] = (unsigned)ceil(pos);
                prefix[2 * j] = prefix[2 * j + 1] = 0u;
                slot[2 * j] = slot[2 * j + 1] = 0u;
            }
        }
    } else if (threadIdx.x >= NRT_WAVE) {
        if (threadIdx.x < NRT_WAVE + 4) head[threadIdx.x - NRT_WAVE] = tab[threadIdx.x - NRT_WAVE];
    } else if (threadIdx.x < (unsigned)g.nranks) {
        slot[threadIdx.x] = tab[kTabRankSlot + threadIdx.x];
        rem[threadIdx.x] = tab[kTabRankRem + threadIdx.x];
        prefix[threadIdx.x] = tab[kTabSlotPrefix + slot[threadIdx.x]];
    }
    __syncthreads();
    const unsigned n = head[kTabCount];
    if (n != 0u) {                                                                   // (uniform)
        for (int r = 0; r < g.nranks; ++r) {
            if (threadIdx.x < 2) found[threadIdx.x] = 0u;
            if (PASS == 0) sel_block_walk<kSelBins0 / kThreads>(rows0 + (size_t)blockIdx.x * kSelBins0, rem[r], red, found);
            else sel_block_walk<kSelBins / kThreads>(slot_rows + (size_t)slot[r] * kSelBins, rem[r], red, found);
            if (threadIdx.x == 0) {
                prefix[r] = sel_extend(prefix[r], PASS, found[0]);
                rem[r] = found[1];
            }
            __syncthreads();
        }
    }
    if (last) {
        if (threadIdx.x < (unsigned)nq) {
            const int j = threadIdx.x;
            const float nanf_ = __uint_as_float(0x7FC00000u);
            float a = nanf_, b = nanf_, v = nanf_;
            if (head[kTabNan] == 0u) {
                a = __uint_as_float(sel_unkey(sel_prefix_key(prefix[2 * j], PASS + 1)));
                b = __uint_as_float(sel_unkey(sel_prefix_key(prefix[2 * j + 1], PASS + 1)));
                const double pos = (double)(n - 1u) * fr.f[j];
                const double t = pos - floor(pos), a64 = (double)a, b64 = (double)b;
                if (method == NRT_PCT_LOWER) v = a;
                else if (method == NRT_PCT_HIGHER) v = b;
                else if (method == NRT_PCT_MIDPOINT) v = (float)((a64 + b64) / 2.0);
                else v = (float)(t < 0.5 ? a64 + (b64 - a64) * t : b64 - (b64 - a64) * (1.0 - t));
            }
            const size_t at = (size_t)blockIdx.x * nq + j;
            o.out[at] = v;
            if (o.lower) o.lower[at] = a;
            if (o.upper) o.upper[at] = b;
        }
        if (threadIdx.x == 0 && o.count) o.count[blockIdx.x] = (int)n;
        return;
    }
    // equal prefixes share a slot
    if (threadIdx.x == 0) {
        unsigned nslots = 0u;
        for (int r = 0; r < g.nranks; ++r) {
            unsigned s = nslots;
            for (unsigned k = 0; k < nslots; ++k)
                if (tab[kTabSlotPrefix + k] == prefix[r]) s = min(s, k);
            if (n == 0u) s = 0u;                                                     // (an empty population: no slot, but a valid index)
            else if (s == nslots) tab[kTabSlotPrefix + nslots++] = prefix[r];
            tab[kTabRankSlot + r] = s;
            tab[kTabRankRem + r] = n == 0u ? 0u : rem[r];
        }
        for (unsigned k = nslots; k < (unsigned)kMaxRanks; ++k) tab[kTabSlotPrefix + k] = kNone;
        tab[kTabSlots] = nslots;
        tab[kTabCount] = n;
        tab[kTabNan] = head[kTabNan];
    }
    if (PASS > 0)                                                                    // the rows serve the next pass
        for (int i = threadIdx.x; i < g.nranks * kSelBins; i += kThreads) slot_rows[i] = 0u;
}

// ---- rescale --------------------------------------------------------------------------------------------------------------------------
struct SelRescale {
    const float *lo, *hi;                            // entry b reads lo[b * stride], hi[b * stride]
    int stride, clip, map;
    float out_min, out_max;
};

__device__ __forceinline__ float sel_rescale(float x, float lo, float hi, const SelRescale &p) {
    float y = (x - lo) / (hi - lo);
    if (hi == lo) y = 0.0f;
    if (p.clip) y = y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y);                         // (a NaN stays)
    if (p.map) y = p.out_min + y * (p.out_max - p.out_min);
    if (lo != lo || hi != hi) y = __uint_as_float(0x7FC00000u);
    return y;
}

template <int DT>
__global__ void __launch_bounds__(kThreads)
sel_rescale_clip(const void *__restrict__ x, SelGeom g, SelRescale p, float *__restrict__ y) {
    const SelRange r = sel_range(g);
    const float lo = p.lo[(size_t)blockIdx.y * p.stride], hi = p.hi[(size_t)blockIdx.y * p.stride];
    for (unsigned q = r.a1 + 4u * threadIdx.x; q < r.t0; q += 4u * kThreads) {
        unsigned b[4];
        sel_bits4<DT>(x, q, b);
        nrt_f4 v;
        v.x = sel_rescale(__uint_as_float(b[0]), lo, hi, p);
        v.y = sel_rescale(__uint_as_float(b[1]), lo, hi, p);
        v.z = sel_rescale(__uint_as_float(b[2]), lo, hi, p);
        v.w = sel_rescale(__uint_as_float(b[3]), lo, hi, p);
        *(nrt_f4 *)(y + q) = v;
    }
    for (unsigned e = r.a0 + threadIdx.x; e < r.a1; e += kThreads) y[e] = sel_rescale(__uint_as_float(sel_bits<DT>(x, e)), lo, hi, p);
    for (unsigned e = r.t0 + threadIdx.x; e < r.t1; e += kThreads) y[e] = sel_rescale(__uint_as_float(sel_bits<DT>(x, e)), lo, hi, p);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct SelPlan {
    SelGeom g;
    unsigned blocks;                                 // of an entry
    size_t off_rows0, off_rows, words;               // in 4-byte words
};

inline bool sel_dtype_ok(int dtype) { return dtype == NRT_DT_F32 || dtype == NRT_DT_BF16 || dtype == NRT_DT_F16; }

// the geometry checks every entry point shares, in the order the header promises
inline int sel_plan(int batch, long long voxels, int nq, SelPlan &p) {
    if (batch < 1 || voxels < 1 || nq < 1 || nq > kMaxQ) return NRT_ERR_INVALID_ARG;
    if (batch > kMaxBatch || voxels >= (1LL << 31) || voxels * batch >= (1LL << 31)) return NRT_ERR_UNSUPPORTED;
    long long blocks = (voxels + kBlockElems - 1) / kBlockElems;
    const long long most = kTargetBlocks / batch > 1 ? kTargetBlocks / batch : 1;
    if (blocks > most) blocks = most;
    long long per = (voxels + blocks - 1) / blocks;
    per = (per + 3) & ~3LL;
    p.blocks = (unsigned)((voxels + per - 1) / per);
    p.g.V = (unsigned)voxels;
    p.g.per = (unsigned)per;
    p.g.vec = 0;
    p.g.nranks = 2 * nq;
    p.off_rows0 = ((size_t)batch * kTabWords + 3) & ~(size_t)3;
    p.off_rows = p.off_rows0 + (size_t)batch * kSelBins0;
    p.words = p.off_rows + (size_t)batch * (size_t)p.g.nranks * kSelBins;
    return NRT_OK;
}

inline int sel_vec_ok(const void *x, int dtype, const void *mask, const void *y) {
    const uintptr_t ax = dtype == NRT_DT_F32 ? 15 : 7;
    return ((uintptr_t)x & ax) == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)y & 15) == 0;
}

template <int DT, int PASS>
inline void sel_launch_hist(const void *x, const void *mask, const SelPlan &p, int batch, unsigned *w, hipStream_t st) {
    const size_t lds = (PASS == 0 ? (size_t)kSelBins0 : (size_t)p.g.nranks * kSelBins) * sizeof(unsigned);
    hipLaunchKernelGGL((sel_hist<DT, PASS>), dim3(p.blocks, (unsigned)batch), dim3(kThreads), lds, st, x, (const unsigned char *)mask, p.g,
                       (const unsigned *)w, w + (PASS == 0 ? p.off_rows0 : p.off_rows));
}

template <int DT>
inline int sel_run(const void *x, const void *mask, const SelPlan &p, int batch, const SelFractions &fr, int method, int flags,
                   const SelOut &o, unsigned *w, hipStream_t st) {
    constexpr int passes = DT == NRT_DT_F32 ? 3 : 2;
    if (nrt_zero_async(w + p.off_rows0, (p.words - p.off_rows0) * sizeof(unsigned), st) != hipSuccess) return NRT_ERR_LAUNCH;
    const dim3 one((unsigned)batch), block(kThreads);
    sel_launch_hist<DT, 0>(x, mask, p, batch, w, st);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_scan<0>, one, block, 0, st, p.g, fr, method, flags, 0, w, w + p.off_rows0, w + p.off_rows, o);
    NRT_CHECK_LAUNCH();
    sel_launch_hist<DT, 1>(x, mask, p, batch, w, st);
    NRT_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_scan<1>, one, block, 0, st, p.g, fr, method, flags, passes == 2, w, w + p.off_rows0, w + p.off_rows, o);
    NRT_CHECK_LAUNCH();
    if (passes == 3) {
        sel_launch_hist<DT, 2>(x, mask, p, batch, w, st);
        NRT_CHECK_LAUNCH();
        hipLaunchKernelGGL(sel_scan<2>, one, block, 0, st, p.g, fr, method, flags, 1, w, w + p.off_rows0, w + p.off_rows, o);
        NRT_CHECK_LAUNCH();
    }
    return NRT_OK;
}

}  // namespace

// What nrt_percentile of this geometry needs; 0 for a geometry the call refuses.
extern "C" size_t nrt_select_workspace_bytes(int batch, long long voxels, int nq) {
    SelPlan p;
    if (sel_plan(batch, voxels, nq, p) != NRT_OK) return 0;
    return p.words * sizeof(unsigned);
}

extern "C" int nrt_percentile(const void *x, int dtype, const void *mask, int batch, long long voxels, const double *positions, int nq,
                              int method, int flags, float *out, float *out_lower, float *out_upper, int *out_count, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (!x || !positions || !out) return NRT_ERR_INVALID_ARG;
    if (!sel_dtype_ok(dtype) || method < NRT_PCT_LINEAR || method > NRT_PCT_MIDPOINT || (flags & ~NRT_PCT_IGNORE_NAN) != 0)
        return NRT_ERR_INVALID_ARG;
    SelPlan p;
    if (batch < 1 || voxels < 1 || nq < 1 || nq > kMaxQ) return NRT_ERR_INVALID_ARG;
    SelFractions fr = {};
    for (int j = 0; j < nq; ++j) {
        if (!(positions[j] >= 0.0 && positions[j] <= 1.0)) return NRT_ERR_INVALID_ARG;      // (a NaN fails both)
        fr.f[j] = positions[j];
    }
    const int rc = sel_plan(batch, voxels, nq, p);
    if (rc != NRT_OK) return rc;
    if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < p.words * sizeof(unsigned)) return NRT_ERR_WORKSPACE;
    p.g.vec = sel_vec_ok(x, dtype, mask, nullptr);
    const SelOut o = {out, out_lower, out_upper, out_count};
    hipStream_t st = nrt_stream(stream);
    unsigned *w = (unsigned *)workspace;
    if (dtype == NRT_DT_F32) return sel_run<NRT_DT_F32>(x, mask, p, batch, fr, method, flags, o, w, st);
    if (dtype == NRT_DT_BF16) return sel_run<NRT_DT_BF16>(x, mask, p, batch, fr, method, flags, o, w, st);
    return sel_run<NRT_DT_F16>(x, mask, p, batch, fr, method, flags, o, w, st);
}

extern "C" int nrt_rescale_clip_f32(const void *x, int dtype, int batch, long long voxels, const float *lo, const float *hi, int stride,
                                    int clip, float out_min, float out_max, float *y, void *stream) {
    if (!x || !lo || !hi || !y || stride < 1) return NRT_ERR_INVALID_ARG;
    if (!sel_dtype_ok(dtype) || out_min != out_min || out_max != out_max) return NRT_ERR_INVALID_ARG;
    SelPlan p;
    const int rc = sel_plan(batch, voxels, 1, p);
    if (rc != NRT_OK) return rc;
    p.g.vec = sel_vec_ok(x, dtype, nullptr, y);
    const SelRescale r = {lo, hi, stride, clip != 0, !(out_min == 0.0f && out_max == 1.0f), out_min, out_max};
    const dim3 grid(p.blocks, (unsigned)batch), block(kThreads);
    hipStream_t st = nrt_stream(stream);
    if (dtype == NRT_DT_F32) hipLaunchKernelGGL(sel_rescale_clip<NRT_DT_F32>, grid, block, 0, st, x, p.g, r, y);
    else if (dtype == NRT_DT_BF16) hipLaunchKernelGGL(sel_rescale_clip<NRT_DT_BF16>, grid, block, 0, st, x, p.g, r, y);
    else hipLaunchKernelGGL(sel_rescale_clip<NRT_DT_F16>, grid, block, 0, st, x, p.g, r, y);
    NRT_CHECK_LAUNCH();
    return NRT_OK;
}
