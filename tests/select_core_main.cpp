// Serial driver of neurite_amd/csrc/select_core.h for tests/test_select_core_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as a child process.  An index outside a histogram row or a walk that runs off it shows here.
//
//   select_core_main select <cases.bin> <out.bin>
// cases.bin (uint32): the number of cases, then per case  n nranks passes,  nranks ranks (each < n) and the bits of n floats.
// out.bin (uint32): per case and rank the bits of the order statistic of that rank, found as the kernels find it: per pass a
// histogram of the digit of the elements whose higher key bits equal the prefix found so far, and sel_walk over it.
//
//   select_core_main keys <bits.bin> <out.bin>
// bits.bin (uint32): float bit patterns.  out.bin (uint32): per pattern its key and the bits the key turns back into.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "select_core.h"

static bool read_words(std::FILE *f, uint32_t *p, size_t n) { return std::fread(p, sizeof(uint32_t), n, f) == n; }
static bool write_words(std::FILE *f, const uint32_t *p, size_t n) { return std::fwrite(p, sizeof(uint32_t), n, f) == n; }

static int run_select(std::FILE *in, std::FILE *out) {
    uint32_t ncases = 0;
    if (!read_words(in, &ncases, 1)) return 3;
    for (uint32_t k = 0; k < ncases; ++k) {
        uint32_t head[3];
        if (!read_words(in, head, 3)) return 3;
        const uint32_t n = head[0], nranks = head[1];
        const int passes = (int)head[2];
        if (passes < 1 || passes > kSelPasses) return 3;
        std::vector<uint32_t> ranks(nranks), bits(n), result(nranks);
        if (!read_words(in, ranks.data(), nranks) || !read_words(in, bits.data(), n)) return 3;
        for (uint32_t r = 0; r < nranks; ++r) {
            uint32_t prefix = 0, rem = ranks[r];
            for (int pass = 0; pass < passes; ++pass) {
                std::vector<unsigned> row((size_t)sel_bins(pass), 0u);
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t key = sel_key(bits[i]);
                    if (pass == 0 || sel_above(key, pass) == prefix) ++row[sel_digit(key, pass)];
                }
                unsigned bin = 0, left = 0;
                if (!sel_walk(row.data(), sel_bins(pass), rem, &bin, &left)) return 5;      // (the rank is not in the row)
                prefix = sel_extend(prefix, pass, bin);
                rem = left;
            }
            result[r] = sel_unkey(sel_prefix_key(prefix, passes));
        }
        if (!write_words(out, result.data(), nranks)) return 4;
    }
    return 0;
}

static int run_keys(std::FILE *in, std::FILE *out) {
    uint32_t b;
    while (read_words(in, &b, 1)) {
        const uint32_t key = sel_key(b);
        const uint32_t pair[2] = {key, sel_unkey(key)};
        if (!write_words(out, pair, 2)) return 4;
        // the digits put the key together again
        uint32_t prefix = 0;
        for (int pass = 0; pass < kSelPasses; ++pass) {
            if (pass > 0 && sel_above(key, pass) != prefix) return 6;
            prefix = sel_extend(prefix, pass, sel_digit(key, pass));
        }
        if (prefix != key || sel_prefix_key(prefix, kSelPasses) != key) return 6;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int rc = 2;
    if (std::strcmp(argv[1], "select") == 0) rc = run_select(in, out);
    else if (std::strcmp(argv[1], "keys") == 0) rc = run_keys(in, out);
    std::fclose(in);
    if (std::fclose(out) != 0 && rc == 0) rc = 4;
    return rc;
}
