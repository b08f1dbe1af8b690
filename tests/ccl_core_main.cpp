// Serial driver of neurite_amd/csrc/ccl_core.h for tests/test_ccl_core_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as a child process.  An out-of-bounds neighbour or a loop that does not end shows here.
//
//   ccl_core_main <cases.bin> <maps.bin>
// cases.bin (int32): the number of cases, then per case  n0 n1 n2 connectivity chunk  and n0 * n1 * n2 keys (0 = background; neighbours
// join when their keys are equal; chunk: the voxels of a block's share, where runs are cut).  maps.bin (int32): per case three
// component maps, from the unions of ccl_for_each_union applied in raster order and in two shuffled orders.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "ccl_core.h"

static bool read_ints(std::FILE *f, int *p, size_t n) { return std::fread(p, sizeof(int), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int ncases = 0;
    if (!read_ints(in, &ncases, 1)) return 3;
    for (int k = 0; k < ncases; ++k) {
        int head[5];
        if (!read_ints(in, head, 5)) return 3;
        const int n[3] = {head[0], head[1], head[2]}, connectivity = head[3], chunk = head[4];
        const int V = n[0] * n[1] * n[2];
        std::vector<int> key(V);
        if (!read_ints(in, key.data(), (size_t)V)) return 3;
        // the unions the merge kernel makes: the seam links, and every backward neighbour whose union is not implied
        std::vector<std::pair<int, int>> pairs;
        std::vector<int> start(V);
        const auto key_of = [&](int u) { return key[(size_t)u]; };
        const auto join = [&](int a, int b) { pairs.emplace_back(a, b); };
        for (int v = 0; v < V; ++v) {
            start[v] = ccl_is_run_head(v, v % n[2], chunk, v > 0 && key[v - 1] == key[v]) ? v : start[v - 1];
            if (key[v] != 0) ccl_for_each_union(v, n, connectivity, chunk, key_of, join);
        }
        for (int order = 0; order < 3; ++order) {
            if (order > 0) {                                                     // Fisher-Yates with a 64-bit LCG
                uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(order + 1) + (uint64_t)k;
                for (size_t i = pairs.size(); i > 1; --i) {
                    s = s * 6364136223846793005ull + 1442695040888963407ull;
                    std::swap(pairs[i - 1], pairs[(size_t)((s >> 33) % i)]);
                }
            }
            std::vector<int> parent(V), comp(V, 0);
            for (int v = 0; v < V; ++v) parent[v] = key[v] != 0 ? start[v] : -1;
            for (const auto &p : pairs) {
                if (order == 2) ccl_union<CclHostMem>(parent.data(), p.second, p.first);
                else ccl_union<CclHostMem>(parent.data(), p.first, p.second);
            }
            for (int v = 0; v < V; ++v)
                if (parent[v] >= 0) ccl_find_compress<CclHostMem>(parent.data(), v);
            int count = 0;
            for (int v = 0; v < V; ++v)                                          // a representative precedes the rest of its component
                if (parent[v] >= 0) comp[v] = ccl_is_representative(parent.data(), v) ? ++count : comp[parent[v]];
            if (std::fwrite(comp.data(), sizeof(int), (size_t)V, out) != (size_t)V) return 4;
        }
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
