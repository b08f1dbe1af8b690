// Serial driver of neurite_amd/csrc/morph_core.h for tests/test_morph_core_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as a child process.  A shift by 64, a wrong tail mask or a word read past its row shows here.
//
//   morph_core_main <cases.bin> <out.bin>
// cases.bin (int32): the number of cases, then per case  structure (27 bits)  iterations  border  nstages  stage[2] (0 erosion, 1
// dilation)  batch  nd  shape[nd]  and the mask [batch, *shape] as 0 / 1 words.
// out.bin (uint8): per case the result [batch, *shape].
// Everything is formed as the kernel forms it: a row is packed 64 voxels at a time (the ballot), the bits past its end take the border
// value (mc_tail_mask, mc_border_fill), a row outside the volume is mc_fill, a step gathers the (up to) 9 neighbour-row triples of a word
// and calls mc_step_word, a dilation runs on mc_reflect of the structure.  The fold of the filters' boundary modes (mc_fold) is checked
// against its definition by repetition on the side.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "morph_core.h"

static bool read_ints(std::FILE *f, int32_t *p, size_t n) { return n == 0 || std::fread(p, sizeof(int32_t), n, f) == n; }

struct Volume {
    int Z, Y, X, W;
    std::vector<uint64_t> words;                     // exactly Z * Y * W: an index past a row is an error the sanitizer sees
    const uint64_t *row(int z, int y) const { return words.data() + ((size_t)z * Y + y) * W; }
};

static void step(const Volume &src, Volume &dst, uint32_t structure, int any, int border) {
    const uint64_t fill = mc_fill(border);
    for (int z = 0; z < src.Z; ++z)
        for (int y = 0; y < src.Y; ++y)
            for (int w = 0; w < src.W; ++w) {
                uint64_t nb[9][3];
                for (int r = 0; r < 9; ++r) {
                    nb[r][0] = nb[r][1] = nb[r][2] = fill;
                    if (!mc_row_bits(structure, r)) continue;
                    const int zz = z + r / 3 - 1, yy = y + r % 3 - 1;
                    if (zz < 0 || zz >= src.Z || yy < 0 || yy >= src.Y) continue;
                    const uint64_t *p = src.row(zz, yy);
                    nb[r][0] = w > 0 ? p[w - 1] : fill;
                    nb[r][1] = p[w];
                    nb[r][2] = w < src.W - 1 ? p[w + 1] : fill;
                }
                dst.words[((size_t)z * src.Y + y) * src.W + w] =
                    mc_border_fill(mc_step_word(nb, structure, any), mc_tail_mask(src.X, w), border);
            }
}

static int run_case(std::FILE *in, std::FILE *out) {
    int32_t head[8];
    if (!read_ints(in, head, 8)) return 3;
    const uint32_t structure = (uint32_t)head[0];
    const int iterations = head[1], border = head[2], nstages = head[3], batch = head[6], nd = head[7];
    if ((structure & ~kMcStructureBits) || iterations < 1 || border < 0 || border > 1 || nstages < 1 || nstages > 2 || batch < 1 || nd < 2 ||
        nd > 3)
        return 3;
    int32_t shape[3];
    if (!read_ints(in, shape, (size_t)nd)) return 3;
    Volume a;
    a.Z = nd == 3 ? shape[0] : 1;
    a.Y = shape[nd - 2];
    a.X = shape[nd - 1];
    if (a.Z < 1 || a.Y < 1 || a.X < 1 || a.X > kMcMaxWords * kMcWordBits) return 3;
    a.W = mc_words(a.X);
    const size_t voxels = (size_t)a.Z * a.Y * a.X;
    std::vector<int32_t> mask(voxels);
    std::vector<uint8_t> result(voxels);
    for (int e = 0; e < batch; ++e) {
        if (!read_ints(in, mask.data(), voxels)) return 3;
        a.words.assign((size_t)a.Z * a.Y * a.W, 0);
        for (int z = 0; z < a.Z; ++z)
            for (int y = 0; y < a.Y; ++y)
                for (int w = 0; w < a.W; ++w) {
                    uint64_t ballot = 0;
                    for (int lane = 0; lane < kMcWordBits; ++lane) {
                        const int x = w * kMcWordBits + lane;
                        if (x < a.X && mask[((size_t)z * a.Y + y) * a.X + x] != 0) ballot |= 1ull << lane;
                    }
                    a.words[((size_t)z * a.Y + y) * a.W + w] = mc_border_fill(ballot, mc_tail_mask(a.X, w), border);
                }
        Volume b = a;
        for (int s = 0; s < nstages; ++s) {
            const int any = head[4 + s];
            if (any < 0 || any > 1) return 3;
            const uint32_t st = any ? mc_reflect(structure) : structure;
            for (int i = 0; i < iterations; ++i) {
                step(a, b, st, any, border);
                a.words.swap(b.words);
            }
        }
        for (int z = 0; z < a.Z; ++z)
            for (int y = 0; y < a.Y; ++y)
                for (int x = 0; x < a.X; ++x)
                    result[((size_t)z * a.Y + y) * a.X + x] = (uint8_t)((a.row(z, y)[x / kMcWordBits] >> (x % kMcWordBits)) & 1ull);
        if (std::fwrite(result.data(), 1, voxels, out) != voxels) return 4;
    }
    return 0;
}

// the closed form of the fold against one reflection at a time
static int fold_by_repetition(int p, int n, int mode) {
    if (mode == kMcConstant) return (p < 0 || p >= n) ? kMcOutside : p;
    if (mode == kMcNearest) return p < 0 ? 0 : (p >= n ? n - 1 : p);
    if (mode == kMcMirror && n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = mode == kMcMirror ? -p : -p - 1;
        else p = mode == kMcMirror ? 2 * n - 2 - p : 2 * n - 1 - p;
    }
    return p;
}

static int check_fold() {
    for (int mode = kMcReflect; mode <= kMcConstant; ++mode)
        for (int n = 1; n <= 9; ++n)
            for (int p = -40; p <= 48; ++p)
                if (mc_fold(p, n, mode) != fold_by_repetition(p, n, mode)) {
                    std::fprintf(stderr, "mc_fold(%d, %d, %d) = %d, by repetition %d\n", p, n, mode, mc_fold(p, n, mode),
                                 fold_by_repetition(p, n, mode));
                    return 6;
                }
    // the words: no shift by 64 at either end of the range
    if (mc_tail_mask(64, 0) != ~0ull || mc_tail_mask(64, 1) != 0ull || mc_tail_mask(65, 1) != 1ull || mc_tail_mask(1, 0) != 1ull ||
        mc_tail_mask(130, 2) != 3ull || mc_tail_mask(63, 0) != (~0ull >> 1))
        return 7;
    if (mc_from_below(1ull << 63, 1ull << 63) != 1ull || mc_from_above(1ull, 1ull) != (1ull << 63)) return 7;
    if (mc_reflect(mc_reflect(0x2A5F3C1u)) != 0x2A5F3C1u || mc_reflect(1u) != (1u << 26)) return 7;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int rc = check_fold();
    if (rc) return rc;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t ncases = 0;
    if (!read_ints(in, &ncases, 1)) return 3;
    for (int c = 0; c < ncases; ++c) {
        const int r = run_case(in, out);
        if (r) {
            std::fprintf(stderr, "case %d: error %d\n", c, r);
            return r;
        }
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
