// The integer core of the per-label statistics and the label confusion matrix (csrc/labelstats.hip), as plain C++ that the host
// compiles too: the id -> slot lookup, the voxel index -> coordinates split, the integer summary (coordinate sums, box) of the lanes of a
// wave that share a slot, formed from the ballot mask alone, the order in which a wave peels off its distinct slots, and the
// order-preserving key of a float.  tests/label_stats_core_main.cpp runs them serially under the sanitizers; the kernels call the very
// same functions.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS_HD __host__ __device__ __forceinline__
#else
#define LS_HD inline
#endif

constexpr int kLsMaxLabels = 256;
constexpr int kLsMaxChannels = 4;
constexpr int kLsWave = 64;
constexpr int kLsNone = -1;                          // the slot of an id that is in no slot

// ---- id -> slot ----------------------------------------------------------------------------------------------------------------------
// The place of labels[t] in the ascending order of the list (ties, which the interface rules out, by position: still a permutation).
LS_HD int ls_rank(const int *labels, int n, int t) {
    const int mine = labels[t];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (labels[j] < mine || (labels[j] == mine && j < t)) ? 1 : 0;
    return r;
}

// keys[n] ascending, slots[n] the slot of each key: the slot of id, or kLsNone.  No index is formed from id.
LS_HD int ls_find(const int *keys, const int *slots, int n, int id) {
    int lo = 0, hi = n;                              // the first key >= id lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && keys[lo] == id) ? slots[lo] : kLsNone;
}

// without a list: slot l is the id l
LS_HD int ls_direct(int id, int n) { return (unsigned)id < (unsigned)n ? id : kLsNone; }

// the counter of a voxel in the [n + 1, n + 1] confusion table: ids in no slot go to the last row / column
LS_HD unsigned ls_pair(int slot_a, int slot_b, int n) {
    const unsigned i = slot_a == kLsNone ? (unsigned)n : (unsigned)slot_a, j = slot_b == kLsNone ? (unsigned)n : (unsigned)slot_b;
    return i * (unsigned)(n + 1) + j;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// The kernels always see three axes: a 2-D shape gets a leading extent of 1, and axis a of the caller is axis a + (3 - nd) here.
struct LsShape {
    unsigned s[3];
};

LS_HD LsShape ls_shape(const int *shape, int nd) {
    LsShape g;
    g.s[0] = nd == 3 ? (unsigned)shape[0] : 1u;
    g.s[1] = (unsigned)shape[nd - 2];
    g.s[2] = (unsigned)shape[nd - 1];
    return g;
}

// voxel index v of an entry (C order) -> its three coordinates
LS_HD void ls_coords(unsigned v, const LsShape &g, unsigned *c) {
    const unsigned t = v / g.s[2];
    c[2] = v - t * g.s[2];
    c[0] = t / g.s[1];
    c[1] = t - c[0] * g.s[1];
}

// ---- the integer summary of the voxels of a wave that share a slot -------------------------------------------------------------------
struct LsSeg {
    unsigned long long cs[3];                        // coordinate sums (64 voxels of coordinates below 2^31: below 2^37)
    int lo[3], hi[3];                                // the box; empty: (INT_MAX, -1)
};

LS_HD LsSeg ls_seg_empty() {
    LsSeg s;
    for (int a = 0; a < 3; ++a) s.cs[a] = 0ull, s.lo[a] = 0x7FFFFFFF, s.hi[a] = -1;
    return s;
}

// the sum of the positions of the set bits of m
LS_HD unsigned ls_bit_index_sum(unsigned long long m) {
    return (unsigned)__builtin_popcountll(m & 0xAAAAAAAAAAAAAAAAull) + ((unsigned)__builtin_popcountll(m & 0xCCCCCCCCCCCCCCCCull) << 1) +
           ((unsigned)__builtin_popcountll(m & 0xF0F0F0F0F0F0F0F0ull) << 2) + ((unsigned)__builtin_popcountll(m & 0xFF00FF00FF00FF00ull) << 3) +
           ((unsigned)__builtin_popcountll(m & 0xFFFF0000FFFF0000ull) << 4) + ((unsigned)__builtin_popcountll(m & 0xFFFFFFFF00000000ull) << 5);
}

// A wave holds the 64 consecutive voxels v0 .. v0 + 63 of an entry, lane k the voxel v0 + k.  The summary of the voxels whose lane has
// its bit set in `lanes` (all of them inside the entry), from the mask alone: the wave is cut into the runs that lie in one row of the
// last axis, where the other coordinates are constant and the last one is the run's start plus the lane; no lane exchanges anything.
LS_HD LsSeg ls_seg_of_lanes(unsigned long long lanes, unsigned v0, const LsShape &g) {
    LsSeg s = ls_seg_empty();
    unsigned c[3];
    ls_coords(v0, g, c);
    unsigned lane = 0;
    while (lane < (unsigned)kLsWave && (lanes >> lane) != 0ull) {
        const unsigned left = g.s[2] - c[2], room = (unsigned)kLsWave - lane;
        const unsigned run = left < room ? left : room;                              // 1 .. 64 lanes in this row
        const unsigned long long m = (lanes >> lane) & (run == (unsigned)kLsWave ? ~0ull : (1ull << run) - 1ull);
        if (m != 0ull) {
            const unsigned n = (unsigned)__builtin_popcountll(m);
            const int first = __builtin_ctzll(m), last = 63 - __builtin_clzll(m);
            s.cs[0] += (unsigned long long)n * c[0];
            s.cs[1] += (unsigned long long)n * c[1];
            s.cs[2] += (unsigned long long)n * c[2] + ls_bit_index_sum(m);
            for (int a = 0; a < 2; ++a) {
                s.lo[a] = s.lo[a] < (int)c[a] ? s.lo[a] : (int)c[a];
                s.hi[a] = s.hi[a] > (int)c[a] ? s.hi[a] : (int)c[a];
            }
            s.lo[2] = s.lo[2] < (int)c[2] + first ? s.lo[2] : (int)c[2] + first;
            s.hi[2] = s.hi[2] > (int)c[2] + last ? s.hi[2] : (int)c[2] + last;
        }
        lane += run;
        c[2] = 0u;                                                                   // the next row
        if (++c[1] == g.s[1]) c[1] = 0u, ++c[0];
    }
    return s;
}

// ---- the segments of a wave ----------------------------------------------------------------------------------------------------------
// A wave holds one slot per lane; `pending` has a bit for every lane whose slot is still to be handled (lanes in no slot never are).
// The next segment is the slot of the lowest pending lane.  The kernels find the lanes of the segment by a ballot; ls_lanes_of is that
// ballot for the host.
LS_HD int ls_lowest(unsigned long long pending) { return __builtin_ctzll(pending); }            // (pending != 0)

LS_HD unsigned long long ls_lanes_of(const int *slot, int value) {
    unsigned long long m = 0ull;
    for (int k = 0; k < kLsWave; ++k)
        if (slot[k] == value) m |= 1ull << k;
    return m;
}

// ---- floats --------------------------------------------------------------------------------------------------------------------------
// An unsigned key in the order of the floats (-0.0 below +0.0), so that min and max of floats are integer atomics; never fed a NaN.
LS_HD unsigned ls_fkey(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
LS_HD unsigned ls_funkey(unsigned key) { return (key & 0x80000000u) ? key & 0x7FFFFFFFu : ~key; }
constexpr unsigned kLsKeyPosInf = 0xFF800000u;       // ls_fkey(+inf): where a min starts
constexpr unsigned kLsKeyNegInf = 0x007FFFFFu;       // ls_fkey(-inf): where a max starts
