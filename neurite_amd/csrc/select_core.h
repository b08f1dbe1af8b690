// The core of the exact order statistics (csrc/select.hip): the monotone key of a float and its inverse, the digits the
// passes of the radix select look at, and the walk that turns a rank into (bin, remaining rank) over a histogram row.  It compiles
// for the device and, as plain C++, for the host, where tests/select_core_main.cpp runs the whole select serially under the address
// and undefined-behaviour sanitizers.
//
// Key: a uint32 whose unsigned order is the order of the floats: all bits of a negative float flipped, the sign bit of the others
// set.  -0.0 is read as +0.0 (one key for both zeros) and every NaN as the one key 0xFFFFFFFF, above +inf (0xFF800000): a NaN with
// the sign bit set would otherwise sort below -inf.
//
// Digits: 12 + 10 + 10 bits from the top.  Pass 0 counts key bits [31:20] in 4096 bins, passes 1 and 2 bits [19:10] and [9:0] in 1024
// bins of the elements whose higher bits equal a prefix found before.  The NaN key alone has the first digit 4095 (+inf has 4088), so
// bin 4095 of pass 0 is the number of NaNs.  A float stored in 16 bits (bfloat16, float16), widened exactly to float32, has float
// bits [12:0] zero, so key bits [12:0] are all zero (all one for a negative float): the last digit is the same for all elements of a
// prefix, which holds the sign, decides nothing, and pass 2 is left out (sel_prefix_key).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEL_HD __host__ __device__ __forceinline__
#else
#define SEL_HD inline
#endif

constexpr int kSelPasses = 3;
constexpr int kSelBins0 = 4096;                      // bins of pass 0
constexpr int kSelBins = 1024;                       // bins of passes 1 and 2
constexpr uint32_t kSelNanKey = 0xFFFFFFFFu;
constexpr uint32_t kSelNanBin = 4095u;               // of pass 0

SEL_HD uint32_t sel_key(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return kSelNanKey;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}

// the bits of the float with this key (of the NaN key: a quiet NaN)
SEL_HD uint32_t sel_unkey(uint32_t key) { return (key & 0x80000000u) ? key & 0x7FFFFFFFu : ~key; }

SEL_HD int sel_shift(int pass) { return pass == 0 ? 20 : pass == 1 ? 10 : 0; }
SEL_HD int sel_bins(int pass) { return pass == 0 ? kSelBins0 : kSelBins; }
SEL_HD uint32_t sel_digit(uint32_t key, int pass) { return (key >> sel_shift(pass)) & (uint32_t)(sel_bins(pass) - 1); }
// the key bits above the digit of `pass` (pass >= 1): what a prefix found by the earlier passes is compared with
SEL_HD uint32_t sel_above(uint32_t key, int pass) { return key >> (sel_shift(pass) + 10); }
// a prefix extended by the digit found in `pass`
SEL_HD uint32_t sel_extend(uint32_t prefix, int pass, uint32_t digit) { return pass == 0 ? digit : (prefix << 10) | digit; }
// The key of a prefix after `passes` passes, for floats whose bits below the prefix are zero: those bits of the key are zero too, but
// for a negative float (key bit 31 clear), where the flip has set them.
SEL_HD uint32_t sel_prefix_key(uint32_t prefix, int passes) {
    const int s = sel_shift(passes - 1);
    const uint32_t key = prefix << s;
    return (key & 0x80000000u) ? key : key | ((1u << s) - 1u);
}

// The bin of `row` (n counters) that holds the element of rank `rank` (0-based, in ascending order of the bins), and the element's
// rank inside that bin.  False, and nothing written, when the row holds `rank` elements or fewer.
SEL_HD bool sel_walk(const unsigned *row, int n, unsigned rank, unsigned *bin, unsigned *rem) {
    for (int i = 0; i < n; ++i) {
        const unsigned c = row[i];
        if (rank < c) {
            *bin = (unsigned)i;
            *rem = rank;
            return true;
        }
        rank -= c;
    }
    return false;
}
