// Serial driver of neurite_amd/csrc/labelstats_core.h for tests/test_label_stats_core_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as a child process.  A slot that leaves its table, an id used as an index or a summary that loses
// a voxel shows here.
//
//   label_stats_core_main <cases.bin> <out.bin>
// cases.bin (int32): the number of cases, then per case  kind (0 statistics, 1 confusion)  nlabels  listed  batch  nd  shape[nd],
// the label list [nlabels] if listed, the id map [batch, *shape] and for a confusion case the second id map.
// out.bin (int64): statistics: counts [batch, nlabels], coord_sums [batch, nlabels, nd], bbox [batch, nlabels, 2, nd];
// confusion: counts [batch, nlabels + 1, nlabels + 1].  Everything is found as the kernels find it: the label list sorted by ls_rank,
// the slot of an id by ls_find / ls_direct, and per 64 voxels ("a wave") the distinct slots peeled off from the lowest pending lane,
// each summarised from the mask of its lanes by ls_seg_of_lanes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "labelstats_core.h"

static bool read_ints(std::FILE *f, int32_t *p, size_t n) { return n == 0 || std::fread(p, sizeof(int32_t), n, f) == n; }
static bool write_longs(std::FILE *f, const std::vector<int64_t> &v) {
    return v.empty() || std::fwrite(v.data(), sizeof(int64_t), v.size(), f) == v.size();
}

struct Lookup {
    bool listed;
    int n;
    std::vector<int> keys, slots;                    // exactly n each: an index past the list is an error the sanitizer sees
    int slot(int id) const { return listed ? ls_find(keys.data(), slots.data(), n, id) : ls_direct(id, n); }
};

static int run_case(std::FILE *in, std::FILE *out) {
    int32_t head[5];
    if (!read_ints(in, head, 5)) return 3;
    const int kind = head[0], nl = head[1], listed = head[2], batch = head[3], nd = head[4];
    if (kind < 0 || kind > 1 || nl < 1 || nl > kLsMaxLabels || batch < 1 || nd < 2 || nd > 3) return 3;
    int32_t shape[3];
    if (!read_ints(in, shape, (size_t)nd)) return 3;
    size_t voxels = 1;
    for (int a = 0; a < nd; ++a) voxels *= (size_t)shape[a];
    std::vector<int32_t> labels((size_t)(listed ? nl : 0)), a((size_t)batch * voxels), b(kind == 1 ? a.size() : 0);
    if (!read_ints(in, labels.data(), labels.size()) || !read_ints(in, a.data(), a.size()) || !read_ints(in, b.data(), b.size())) return 3;

    Lookup look = {listed != 0, nl, {}, {}};
    if (listed) {
        look.keys.assign((size_t)nl, 0);
        look.slots.assign((size_t)nl, 0);
        std::vector<char> seen((size_t)nl, 0);
        for (int t = 0; t < nl; ++t) {
            const int r = ls_rank(labels.data(), nl, t);
            if (r < 0 || r >= nl || seen[(size_t)r]) return 5;                      // (not a permutation)
            seen[(size_t)r] = 1;
            look.keys[(size_t)r] = labels[(size_t)t];
            look.slots[(size_t)r] = t;
        }
    }
    const LsShape g = ls_shape(shape, nd);
    const int ax0 = 3 - nd;

    if (kind == 1) {
        std::vector<int64_t> counts((size_t)batch * (size_t)(nl + 1) * (size_t)(nl + 1), 0);
        for (int e = 0; e < batch; ++e)
            for (size_t v = 0; v < voxels; ++v) {
                const size_t at = (size_t)e * voxels + v;
                const unsigned code = ls_pair(look.slot(a[at]), look.slot(b[at]), nl);
                counts.at((size_t)e * (size_t)(nl + 1) * (size_t)(nl + 1) + code) += 1;
            }
        return write_longs(out, counts) ? 0 : 4;
    }

    std::vector<int64_t> counts((size_t)batch * nl, 0), sums((size_t)batch * nl * nd, 0), bbox((size_t)batch * nl * 2 * nd, 0);
    for (int e = 0; e < batch; ++e) {
        for (int l = 0; l < nl; ++l)
            for (int k = 0; k < nd; ++k) {
                bbox[(((size_t)e * nl + l) * 2 + 0) * nd + k] = shape[k];
                bbox[(((size_t)e * nl + l) * 2 + 1) * nd + k] = -1;
            }
        for (size_t step = 0; step < voxels; step += kLsWave) {
            int slot[kLsWave];
            unsigned long long pending = 0ull;
            for (int k = 0; k < kLsWave; ++k) {
                const size_t v = step + (size_t)k;
                slot[k] = v < voxels ? look.slot(a[(size_t)e * voxels + v]) : kLsNone;
                if (slot[k] != kLsNone) pending |= 1ull << k;
            }
            while (pending != 0ull) {
                const int s = slot[ls_lowest(pending)];
                const unsigned long long lanes = ls_lanes_of(slot, s);
                if (s < 0 || s >= nl || (lanes & ~pending) != 0ull) return 5;
                const LsSeg seg = ls_seg_of_lanes(lanes, (unsigned)step, g);
                const size_t row = (size_t)e * nl + (size_t)s;
                counts.at(row) += __builtin_popcountll(lanes);
                for (int ax = ax0; ax < 3; ++ax) {
                    const size_t k = (size_t)(ax - ax0);
                    sums.at(row * nd + k) += (int64_t)seg.cs[ax];
                    int64_t &lo = bbox.at((row * 2 + 0) * nd + k), &hi = bbox.at((row * 2 + 1) * nd + k);
                    if (seg.lo[ax] < lo) lo = seg.lo[ax];
                    if (seg.hi[ax] > hi) hi = seg.hi[ax];
                }
                pending &= ~lanes;
            }
        }
    }
    return write_longs(out, counts) && write_longs(out, sums) && write_longs(out, bbox) ? 0 : 4;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t ncases = 0;
    int rc = read_ints(in, &ncases, 1) ? 0 : 3;
    for (int32_t k = 0; rc == 0 && k < ncases; ++k) rc = run_case(in, out);
    std::fclose(in);
    if (std::fclose(out) != 0 && rc == 0) rc = 4;
    return rc;
}
