// The word arithmetic of the binary morphology (csrc/morph.hip) and the index fold of the boundary modes of the grey and rank
// filters, as plain C++ that the host compiles too.  One voxel is one bit: bit j of word w of a row along the last axis is the voxel
// x = 64 w + j.  tests/morph_core_main.cpp runs the same functions serially under the sanitizers; the kernels call them as they are.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_HD __host__ __device__ __forceinline__
#else
#define MC_HD inline
#endif

constexpr int kMcWordBits = 64;
constexpr int kMcMaxWords = 16;                      // extents along the last axis up to 1024
constexpr uint32_t kMcStructureBits = (1u << 27) - 1u;

// ---- the structure -------------------------------------------------------------------------------------------------------------------
// Bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of a structure is its entry at the offset (dz, dy, dx); a 2-D structure lives in the
// plane dz = 0.  The three entries of a neighbour row (dz, dy), dx = -1, 0, +1 from the lowest bit:
MC_HD uint32_t mc_row_bits(uint32_t structure, int r) { return (structure >> (3 * r)) & 7u; }
// Dilation by a structure is the OR over the REFLECTED structure: the entry at o moves to -o, bit i to bit 26 - i.
MC_HD uint32_t mc_reflect(uint32_t structure) {
    uint32_t out = 0;
    for (int i = 0; i < 27; ++i) out |= ((structure >> i) & 1u) << (26 - i);
    return out;
}
MC_HD uint32_t mc_plane_mask() { return 0x1FFu << 9; }                // the entries with dz = 0

// ---- words ---------------------------------------------------------------------------------------------------------------------------
// the words of a row of n voxels
MC_HD int mc_words(int n) { return (n + kMcWordBits - 1) / kMcWordBits; }
// all ones or all zeros: a word wholly outside the volume
MC_HD uint64_t mc_fill(int border) { return border ? ~0ull : 0ull; }
// the bits of word w that are voxels of a row of n (never a shift by 64: a full word is answered before the shift is formed)
MC_HD uint64_t mc_tail_mask(int n, int w) {
    const int left = n - w * kMcWordBits;
    if (left >= kMcWordBits) return ~0ull;
    if (left <= 0) return 0ull;
    return (1ull << left) - 1ull;
}
// the bits past the end of the row take the border value
MC_HD uint64_t mc_border_fill(uint64_t word, uint64_t valid, int border) { return border ? (word | ~valid) : (word & valid); }
// bit j of the result is the voxel x - 1: the word moves up by one bit and takes the top bit of the word before it
MC_HD uint64_t mc_from_below(uint64_t word, uint64_t prev) { return (word << 1) | (prev >> 63); }
// bit j of the result is the voxel x + 1: the word moves down by one bit and takes the lowest bit of the word behind it
MC_HD uint64_t mc_from_above(uint64_t word, uint64_t next) { return (word >> 1) | (next << 63); }

// One step of one word.  rows[r] = {the word before, the word itself, the word behind} of the neighbour row r = (dz + 1) * 3 + (dy + 1),
// already holding the border value wherever they lie outside the volume; rows that the structure does not name are not read.
// OR of m[x + o] over the set entries o (any = 1: dilation, with the reflected structure) or their AND (any = 0: erosion).  An empty
// structure gives the neutral element, as scipy does.
MC_HD uint64_t mc_step_word(const uint64_t rows[9][3], uint32_t structure, int any) {
    uint64_t acc = any ? 0ull : ~0ull;
    for (int r = 0; r < 9; ++r) {
        const uint32_t bits = mc_row_bits(structure, r);
        if (!bits) continue;
        const uint64_t prev = rows[r][0], word = rows[r][1], next = rows[r][2];
        if (bits & 1u) acc = any ? (acc | mc_from_below(word, prev)) : (acc & mc_from_below(word, prev));
        if (bits & 2u) acc = any ? (acc | word) : (acc & word);
        if (bits & 4u) acc = any ? (acc | mc_from_above(word, next)) : (acc & mc_from_above(word, next));
    }
    return acc;
}

// ---- the boundary modes of the grey and rank filters ---------------------------------------------------------------------------------
constexpr int kMcReflect = 0, kMcMirror = 1, kMcNearest = 2, kMcConstant = 3;
constexpr int kMcOutside = -1;                       // the fold of an outside index under kMcConstant

// The index in [0, n) that sample p of an axis of n stands for, for any p (a window may be wider than the axis: the fold is the
// closed form of scipy's repeated one).  reflect: period 2 n, the edge repeated; mirror: period 2 n - 2, the edge not repeated.
MC_HD int mc_fold(int p, int n, int mode) {
    if (p >= 0 && p < n) return p;
    if (mode == kMcConstant) return kMcOutside;
    if (mode == kMcNearest) return p < 0 ? 0 : n - 1;
    if (mode == kMcMirror) {
        if (n == 1) return 0;
        const int period = 2 * n - 2;
        int q = p % period;
        if (q < 0) q += period;
        return q < n ? q : period - q;
    }
    const int period = 2 * n;
    int q = p % period;
    if (q < 0) q += period;
    return q < n ? q : period - 1 - q;
}
