// The union-find core of connected-component labelling (csrc/ccl.hip): neighbour enumeration, find, union and the
// representative test.  It compiles for the device and, as plain C++, for the host, where tests/ccl_core_main.cpp runs it serially
// under the address and undefined-behaviour sanitizers.
//
// parent[] holds, for a foreground voxel v of one batch entry, the linear index of another voxel of the same component with
// parent[v] <= v, and -1 on the background.  It starts as the head of v's run (below) and only ever DECREASES (every write is a minimum), so
//   * a chain v, parent[v], parent[parent[v]], ... strictly decreases until it reaches a root (parent[r] == r) and cannot cycle;
//   * the root of a finished component is its smallest linear index, whatever the order of the unions.
// M supplies the two memory operations on a parent word: on the device agent-scope atomics (a word another workgroup may write is
// never read by a plain load), on the host plain accesses.
#pragma once

#if defined(__HIPCC__)
#define CCL_HD __host__ __device__ __forceinline__
#else
#define CCL_HD inline
#endif

struct CclHostMem {
    static inline int load(const int *p) { return *p; }
    static inline int fetch_min(int *p, int v) {
        const int old = *p;
        if (v < old) *p = v;
        return old;
    }
};

constexpr int kCclBackward = 13;                     // the offsets of {-1, 0, 1}^3 in front of (0, 0, 0) in raster order

// Backward neighbour c (0 <= c < 13) of voxel (i0, i1, i2) in a volume of extents n[3] (a 2-D volume has n[0] = 1: its offsets along
// the padding axis fall outside).  The offset is o = (c / 9 - 1, c / 3 % 3 - 1, c % 3 - 1), lexicographically negative, so the
// neighbour's linear index is smaller.  Returns it, or -1 when sum |o| > connectivity or the neighbour lies outside the volume.
CCL_HD int ccl_backward_neighbour(int c, const int *n, int connectivity, int i0, int i1, int i2) {
    const int o0 = c / 9 - 1, o1 = (c / 3) % 3 - 1, o2 = c % 3 - 1;
    const int order = (o0 != 0) + (o1 != 0) + (o2 != 0);
    if (order > connectivity) return -1;
    const int j0 = i0 + o0, j1 = i1 + o1, j2 = i2 + o2;
    if (j0 < 0 || j1 < 0 || j2 < 0 || j0 >= n[0] || j1 >= n[1] || j2 >= n[2]) return -1;
    return (j0 * n[1] + j1) * n[2] + j2;
}

// Runs.  A run is a stretch of equal keys along the last axis inside one row and one chunk of `chunk` consecutive voxels (the share of
// a block).  The forest starts with every foreground voxel pointing at the head of its run: a valid forest (the head has the smallest
// index of the run and carries the same id), already flat inside a run, that makes most unions unnecessary:
//   * voxel v and its left neighbour v - 1 need a union only where a chunk seam cut their run (ccl_seam_union);
//   * the union of v with its backward neighbour w = v + o, o not (0, 0, -1), is IMPLIED when the left neighbour v - 1 carries v's key
//     and its own neighbour by the same offset, t = w - 1, exists and carries it too: v ~ v - 1 and t ~ w are run or seam links, and
//     v - 1 ~ t is v - 1's own union for offset o, made there or implied further left (the induction ends at the row's first voxel
//     or at a key that differs).  ccl_left_twin returns t, or -1 where v - 1 has no such neighbour.
CCL_HD bool ccl_is_run_head(int v, int i2, int chunk, bool same_key_as_left) { return i2 == 0 || v % chunk == 0 || !same_key_as_left; }
CCL_HD bool ccl_seam_union(int v, int i2, int chunk) { return i2 > 0 && v % chunk == 0; }
CCL_HD int ccl_left_twin(int c, const int *n, int i2, int w) {
    const int j2 = i2 - 1 + (c % 3 - 1);
    return (i2 > 0 && j2 >= 0 && j2 < n[2]) ? w - 1 : -1;
}
constexpr int kCclLeft = 12;                         // the backward neighbour (0, 0, -1)

// Calls join(v, w) for every union foreground voxel v has to make, by the rules above.  key(u) is the key of voxel u of the entry.
template <class Key, class Join>
CCL_HD void ccl_for_each_union(int v, const int *n, int connectivity, int chunk, const Key &key, const Join &join) {
    const int q = v / n[2];
    const int i2 = v - q * n[2], i0 = q / n[1], i1 = q - i0 * n[1];
    const int k = key(v);
    const bool left = i2 > 0 && key(v - 1) == k;
    if (left && ccl_seam_union(v, i2, chunk)) join(v, v - 1);
    for (int c = n[0] == 1 ? 9 : 0; c < kCclLeft; ++c) {                          // (nothing in front along an axis of one voxel)
        const int w = ccl_backward_neighbour(c, n, connectivity, i0, i1, i2);
        if (w < 0 || key(w) != k) continue;
        const int t = left ? ccl_left_twin(c, n, i2, w) : -1;
        if (t >= 0 && key(t) == k) continue;
        join(v, w);
    }
}

// The root of x's tree at some moment of the call.  Every step moves to a strictly smaller index (parent[x] < x unless x is a root),
// so the loop ends after at most x steps whatever other threads write meanwhile: their writes only lower parent words.
template <class M>
CCL_HD int ccl_find(int *parent, int x) {
    int p = M::load(parent + x);
    while (p != x) {
        x = p;
        p = M::load(parent + x);
    }
    return x;
}

// As ccl_find, and shortens x's own link to the root found (a minimum: it can only lower parent[x], to an ancestor of x).
template <class M>
CCL_HD int ccl_find_compress(int *parent, int x) {
    const int first = M::load(parent + x);
    int r = first;
    if (r != x) {
        r = ccl_find<M>(parent, first);
        if (r != first) M::fetch_min(parent + x, r);
    }
    return r;
}

// Joins the trees of a and b.  Each turn takes the two current roots, a > b, and lowers parent[a] to b.  If a still was a root, the
// trees are one.  If not, another thread had hung a below `old` < a in between: a now hangs below min(old, b), and what is left is to
// join old and b.  max(a, b) strictly decreases from turn to turn (old < a, and find never moves up) and is bounded below by 0, so
// the loop ends without waiting for anybody.
template <class M>
CCL_HD void ccl_union(int *parent, int a, int b) {
    if (M::load(parent + a) == M::load(parent + b)) return;                       // (one tree already: the root is not looked at)
    for (;;) {
        a = ccl_find_compress<M>(parent, a);
        b = ccl_find_compress<M>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = M::fetch_min(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// After flattening, parent[v] is the representative of v's component: its smallest linear index.  Component numbers count the
// representatives in raster order: number(v) = 1 + #{ r < parent[v] : parent[r] == r }.
CCL_HD bool ccl_is_representative(const int *parent, int v) { return parent[v] == v; }
