// Device pieces shared by the kernels that form a sampling location from an affine matrix in registers (affine_warp.hip,
// warp_argmax.hip): the argument block, the matrix load and the location with the roundings of the two-kernel path.
#pragma once

#include "interpn_core.h"

namespace {

struct AffWarpArgs {
    const float *vol;        // [batch][S][C]
    const float *matrix;     // [matrix_batch][D][D + 1]
    const float *gout;       // backward: [batch][O][C]
    float *out;              // forward:  [batch][O][C]
    float *rows;             // backward: [batch][gridDim.x][D (D + 1)] partial sums
    int S[NRT_MAXD], O[NRT_MAXD];
    float c[NRT_MAXD];       // centre offsets (0 without shift_center)
    int C, CG;               // channels; items per voxel (C / V for V channels per item, see item_width)
    unsigned nout, nitems;   // prod(O); nout * CG
    long long vol_bs, out_bs;
    int m_bs;                // matrix batch stride in floats (0: one transform for the batch)
    int has_fill;
    float fill;
};

template <int D>
__device__ __forceinline__ void load_matrix(const AffWarpArgs &a, int b, float (&M)[D][D + 1]) {
    const float *m = a.matrix + (long long)b * a.m_bs;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= D; ++j) M[i][j] = m[i * (D + 1) + j];
}

// centred coordinate p and sampling location of output voxel q: affine_shift<D> (vxm.hip) followed by load_loc<D, NRT_LOC_SHIFT>
template <int D>
__device__ __forceinline__ void affine_loc(const AffWarpArgs &a, const float (&M)[D][D + 1], unsigned q, float (&p)[D], float (&loc)[D]) {
    int qd[D];
    unsigned r = q;
#pragma unroll
    for (int d = D - 1; d > 0; --d) { qd[d] = (int)(r % (unsigned)a.O[d]); r /= (unsigned)a.O[d]; }
    qd[0] = (int)r;
#pragma unroll
    for (int d = 0; d < D; ++d) p[d] = nrt_sub((float)qd[d], a.c[d]);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = nrt_mul(M[i][0], p[0]);
#pragma unroll
        for (int j = 1; j < D; ++j) s = nrt_add(s, nrt_mul(M[i][j], p[j]));
        s = nrt_add(s, M[i][D]);                             // the homogeneous coordinate is 1
        loc[i] = nrt_add((float)qd[i], nrt_sub(s, p[i]));    // cast(mesh, float32) + shift
    }
}

template <int D>
__device__ __forceinline__ bool affine_oob(const AffWarpArgs &a, const float (&loc)[D]) {
    bool oob = false;                                        // the unclipped location, as out_of_bounds<D>
#pragma unroll
    for (int d = 0; d < D; ++d) oob = oob || (loc[d] < 0.0f) || (loc[d] > (float)(a.S[d] - 1));
    return oob;
}

}  // namespace
