// Device pieces shared by the kernels that warp integer LABEL MAPS (warp_labels.hip, warp_argmax.hip): the 8 gathered corner ids and
// the per-dimension weights of a sampling location, and the 8 corner weights fl(fl(wx wy) wz) in corner order 000 ... 111.
#pragma once

#include "interpn_core.h"

namespace {

constexpr int WL_BLOCK = 256;

// the 8 corner ids and the per-dimension weights at location p (every index lies inside the volume, whatever p holds: corner_1d)
__device__ __forceinline__ void wl_gather(const InterpArgs &a, const int *__restrict__ mov, const float (&p)[NRT_MAXD], int (&lab)[8],
                                          float (&w0)[3], float (&w1)[3]) {
    int i0[3], i1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) corner_1d(p[d], a.S[d], i0[d], i1[d], w0[d], w1[d]);
    // corner = 4 cx + 2 cy + cz; every index lies inside the volume.  The two z-neighbours of an (x, y) row are one 8-byte request, 4
    // requests per voxel instead of 8: the pair starts at zb = min(z0, S_z - 2), and z0, z1 are each zb or zb + 1 (z1 = z0 at the far
    // face).  Worth 3 - 4 % where the gathers are incoherent (rough field 1.05 -> 1.01 ms forward, 1.62 -> 1.57 with the backward at
    // 4 x 160^3 x 32), nothing on the smooth bench field, where the kernels are bound by VALU issue
    if (a.S[2] >= 2) {
        const int zb = min(i0[2], a.S[2] - 2);
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const int idx = (((c & 4) ? i1[0] : i0[0]) * a.S[1] + ((c & 2) ? i1[1] : i0[1])) * a.S[2] + zb;
            int pair[2];
            __builtin_memcpy(pair, mov + idx, sizeof(pair));     // (4-byte aligned; the compiler picks the request)
            lab[c] = i0[2] == zb ? pair[0] : pair[1];
            lab[c + 1] = i1[2] == zb ? pair[0] : pair[1];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int idx = (((c & 4) ? i1[0] : i0[0]) * a.S[1] + ((c & 2) ? i1[1] : i0[1])) * a.S[2] + ((c & 1) ? i1[2] : i0[2]);
            lab[c] = mov[idx];
        }
    }
}

// location, the 8 corner ids and the per-dimension weights of output voxel q
template <int MODE>
__device__ __forceinline__ void wl_corners(const InterpArgs &a, const float *locb, const int *__restrict__ mov, unsigned q, int (&lab)[8],
                                           float (&w0)[3], float (&w1)[3], float (&p)[NRT_MAXD], bool &oob) {
    int qd[NRT_MAXD];
    decode<3>(a, q, qd);
    load_loc<3, MODE>(a, locb, q, qd, p);
    oob = a.has_fill ? out_of_bounds<3>(a, p) : false;
    wl_gather(a, mov, p, lab, w0, w1);
}

__device__ __forceinline__ void wl_weights(const float (&w0)[3], const float (&w1)[3], float (&wt)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
        wt[c] = nrt_mul(nrt_mul((c & 4) ? w1[0] : w0[0], (c & 2) ? w1[1] : w0[1]), (c & 1) ? w1[2] : w0[2]);
}

}  // namespace
