// Cross-lane and block reductions shared by the kernels (wave64 only).  Each helper fixes the ORDER in which lanes and waves are
// combined: float sums round, so that order is part of a kernel's bits, and the bit-for-bit tests pin it.  The loop bounds are template
// parameters under #pragma unroll: so written a helper compiles to the instructions of the unrolled loop it stands for
// (tools/kernel_digest.py --tree on both commits shows where it does not; those sites stay written out and say so).
#pragma once

#include "nrt_common.h"

namespace {

struct nrt_op_sum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct nrt_op_max {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
};
struct nrt_op_min {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
};

// Butterfly over the lanes that differ in the bits FROM, 2 FROM, ... < TO, offsets ASCENDING, v = op(v, partner's v); every lane gets
// the result.  <NRT_WAVE, 1> is the whole wave, <G, 1> an aligned group of G lanes, <NRT_WAVE, G> the lanes that agree in lane % G.
template <int TO, int FROM, typename T, typename OP> __device__ __forceinline__ T nrt_wave_reduce(T v, OP op) {
#pragma unroll
    for (int off = FROM; off < TO; off <<= 1) v = op(v, __shfl_xor(v, off, NRT_WAVE));
    return v;
}
template <int TO = NRT_WAVE, int FROM = 1, typename T> __device__ __forceinline__ T nrt_wave_sum(T v) {
    return nrt_wave_reduce<TO, FROM>(v, nrt_op_sum());
}
template <int TO = NRT_WAVE, int FROM = 1, typename T> __device__ __forceinline__ T nrt_wave_max(T v) {
    return nrt_wave_reduce<TO, FROM>(v, nrt_op_max());
}
template <int TO = NRT_WAVE, int FROM = 1, typename T> __device__ __forceinline__ T nrt_wave_min(T v) {
    return nrt_wave_reduce<TO, FROM>(v, nrt_op_min());
}

// nrt_wave_sum<NRT_WAVE, FROM> with the first offset as an argument (a power of two), for the Dice, warp + Dice and joint-loss
// kernels: they were written against this form, which is unrolled after it is inlined, and the instruction streams that the
// benchmark pins come out different through the template form.
// New code uses the template form.
template <typename T> __device__ __forceinline__ T nrt_wave_sum_from(T v, int from) {
    for (int off = from; off < NRT_WAVE; off <<= 1) v += __shfl_xor(v, off, NRT_WAVE);
    return v;
}

// Sum over each aligned group of 8 lanes in three DPP steps, no LDS crossbar: lane ^ 1 (quad_perm [1,0,3,2]), lane ^ 2 (quad_perm
// [2,3,0,1]), then the mirrored half row (row_half_mirror); every lane of the group gets the sum.
__device__ __forceinline__ float nrt_dpp_sum8(float r) {
    r += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(r), 0xB1, 0xF, 0xF, true));
    r += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(r), 0x4E, 0xF, 0xF, true));
    r += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(r), 0x141, 0xF, 0xF, true));
    return r;
}
// The whole wave's sum on top of it: the mirrored row (row_mirror) makes it 16 lanes, xor 16 and xor 32 the wave.
__device__ __forceinline__ float nrt_dpp_wave_sum(float r) {
    r = nrt_dpp_sum8(r);
    r += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(r), 0x140, 0xF, 0xF, true));
    return nrt_wave_sum<NRT_WAVE, 16>(r);
}

// Inclusive scan over the wave by __shfl_up, offsets 1, 2, ..., 32: lane l ends with op over lanes 0..l.
template <typename T, typename OP> __device__ __forceinline__ T nrt_wave_scan_incl(T v, unsigned lane, OP op) {
#pragma unroll
    for (int off = 1; off < NRT_WAVE; off <<= 1) {
        const T y = __shfl_up(v, off, NRT_WAVE);
        if (lane >= (unsigned)off) v = op(v, y);
    }
    return v;
}

// The block's reduction of one value per thread: the wave butterfly (ascending), then lane 0 of each wave leaves its partial in
// red[wave] and every thread folds red[0], red[1], ... in wave order.  Every thread of the block calls it and gets the result; the
// leading barrier keeps a previous call's readers of `red` ahead of this call's writers.
template <int WAVES, typename T, typename OP> __device__ __forceinline__ T nrt_block_reduce(T v, T *red, OP op) {
    v = nrt_wave_reduce<NRT_WAVE, 1>(v, op);
    __syncthreads();
    if ((threadIdx.x & (NRT_WAVE - 1)) == 0) red[threadIdx.x / NRT_WAVE] = v;
    __syncthreads();
    T s = red[0];
    for (int w = 1; w < WAVES; ++w) s = op(s, red[w]);
    return s;
}
template <int WAVES, typename T> __device__ __forceinline__ T nrt_block_sum(T v, T *red) {
    return nrt_block_reduce<WAVES>(v, red, nrt_op_sum());
}

}  // namespace
