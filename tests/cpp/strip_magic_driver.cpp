// strip_magic (mlm_host.h): the multiplier k_bin_sectors divides a strip index by the strips per image row with, checked over its whole
// stated range — every divisor 1 .. STRIP_MAGIC_MAX_D against every operand below STRIP_MAGIC_MAX_I, the quotient kept by counting
// (no division in the loop) and evaluated as the kernel evaluates it: the high word of the 32-bit product (2 i) * m.
#include <cstdint>
#include <cstdio>

#include "mlm_host.h"

static inline uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); } // (__umulhi)

int main() {
    using namespace mlm_host;
    unsigned long long checked = 0, bad = 0;
    for (unsigned int d = 1; d <= STRIP_MAGIC_MAX_D; ++d) {
        const uint32_t m = strip_magic(d);
        if (m == 0u || (unsigned long long)m * d < (1ull << 31) || (unsigned long long)m * d >= (1ull << 31) + d) {
            std::printf("bad multiplier d=%u m=%u\n", d, m);
            return 1;
        }
        uint32_t q = 0, r = 0;
        for (uint32_t i = 0; i < STRIP_MAGIC_MAX_I; ++i) {
            bad += umulhi(i << 1, m) != q;
            if (++r == d) {
                r = 0;
                ++q;
            }
        }
        checked += STRIP_MAGIC_MAX_I;
        if (bad) {
            std::printf("inexact d=%u\n", d);
            return 1;
        }
    }
    // out of range: no multiplier
    const int refused = (strip_magic(0u) == 0u) + (strip_magic(STRIP_MAGIC_MAX_D + 1u) == 0u) + (strip_magic(0xFFFFFFFFu) == 0u);
    // the first operand past the stated range that the largest divisors get wrong, if any, is NOT below the range's end
    unsigned int first_wrong = 0;
    for (unsigned int d = STRIP_MAGIC_MAX_D; d > STRIP_MAGIC_MAX_D - 64u && !first_wrong; --d) {
        const uint32_t m = strip_magic(d);
        for (uint32_t i = STRIP_MAGIC_MAX_I; i < (1u << 24); ++i)
            if (umulhi(i << 1, m) != i / d) {
                first_wrong = i;
                break;
            }
    }
    std::printf("checked %llu bad %llu refused %d max_i %u max_d %u first_wrong_beyond %u\n", checked, bad, refused, STRIP_MAGIC_MAX_I, STRIP_MAGIC_MAX_D, first_wrong);
    return 0;
}
