// The integer forms of k_sector's reference pass (mlm_sector_refs.h) against the straightforward ones, on the CPU:
//   origin   a cell's packed origin (row and tile column of its first pixel; lists: its 64-item row), unpacked again, against
//            pixel / width, (pixel % width) >> 3 and item >> 6, for every pixel of the widths given on the command line (all pixels below
//            2^21 — the sector path's largest frame — where that is feasible, else both sides of every row end and the last pixels), every kind
//   rows     the flags of a mask's non-empty rows and the rows taken from them one by one, against a loop over the eight bytes:
//            all 256 row patterns x 1 000 random masks each
//   repack   the reference word built from a group's shared base plus row and byte, against mlm_ref_pack
//   miss     the row of a word of the miss mask, w / RW, as the kernel takes it (high word of (2 w) * strip_magic(RW))
// Prints one line of counters; the test asserts on them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "mlm_host.h"
#include "mlm_sector_refs.h"

static unsigned long long n_origin = 0, bad_origin = 0, n_rows = 0, bad_rows = 0, n_repack = 0, bad_repack = 0, n_miss = 0, bad_miss = 0, n_row_ends = 0;
static const uint32_t MAX_PIX = 1u << 21; // mlm_limits.max_points < 2^21 on the sector path (MLM_SEC_CNT_BITS)

static void check_pixel(uint32_t pix, int width, uint32_t osh, unsigned long long m, int s) {
    for (uint32_t kind = 0; kind < MLM_TIME_SLOTS; kind += (pix & 1u) ? 20u : 7u) { // (kinds 0, 7, 14 / 0, 20: the time's remainder must not leak)
        const uint32_t tmin = pix * MLM_TIME_SLOTS + kind;
        const uint32_t o = mlm_sec_origin(tmin, width, osh, m, s);
        const uint32_t row = pix / (uint32_t)width, xt = (pix % (uint32_t)width) >> 3;
        bad_origin += mlm_sec_origin_row(o, true, osh) != row || mlm_sec_origin_xt(o, osh) != xt;
        ++n_origin;
    }
}

int main(int argc, char **argv) {
    using namespace mlm_host;
    // ---- origin, dense images
    for (int a = 1; a < argc; ++a) {
        const int width = std::atoi(argv[a]);
        const uint32_t osh = mlm_sec_origin_shift(width);
        unsigned long long m;
        int s;
        div_magic((unsigned int)width, m, s);
        if ((((uint32_t)width - 1u) >> 3) >> osh) ++bad_origin; // (the last tile column fits the shift)
        if (width <= 1280) {
            for (uint32_t pix = 0; pix < MAX_PIX; ++pix) check_pixel(pix, width, osh, m, s);
            n_row_ends += (MAX_PIX - 1u) / (uint32_t)width;
        } else {
            for (uint32_t end = (uint32_t)width; end < MAX_PIX; end += (uint32_t)width) { // both sides of every row end, and of every tile column's there
                for (uint32_t d = 0; d < 10u; ++d) {
                    check_pixel(end - 1u - d, width, osh, m, s);
                    if (end + d < MAX_PIX) check_pixel(end + d, width, osh, m, s);
                }
                ++n_row_ends;
            }
            for (uint32_t pix = 0; pix < 4096u && pix < MAX_PIX; ++pix) check_pixel(pix, width, osh, m, s);
        }
        for (uint32_t d = 1; d <= 64u; ++d) check_pixel(MAX_PIX - d, width, osh, m, s); // the last pixels below 2^21
    }
    // ---- origin, lists: the 64-item row of every item below 2^21 (and the shift of a list is 0)
    if (mlm_sec_origin_shift(0) != 0u) ++bad_origin;
    for (uint32_t item = 0; item < MAX_PIX; ++item)
        for (uint32_t kind = 0; kind < MLM_TIME_SLOTS; kind += 10u) {
            const uint32_t o = mlm_sec_origin(item * MLM_TIME_SLOTS + kind, 0, 0u, 0ull, 0);
            bad_origin += mlm_sec_origin_row(o, false, 0u) != item >> 6;
            ++n_origin;
        }
    // ---- rows and repack
    std::mt19937_64 rng(12345);
    for (uint32_t pattern = 0; pattern < 256u; ++pattern)
        for (int rep = 0; rep < 1000; ++rep) {
            unsigned long long mask = 0;
            for (uint32_t row = 0; row < 8u; ++row) {
                if (!((pattern >> row) & 1u)) continue;
                uint32_t byte = (uint32_t)(rng() & 0xFFu);
                if (rep < 8) byte = 1u << rep; // (single lanes: bit 7 alone and bit 0 alone are the detection's edge cases)
                if (!byte) byte = 0x80u;
                mask |= (unsigned long long)byte << (8u * row);
            }
            uint32_t flags = mlm_sec_row_flags(mask), seen = 0, count = 0;
            bool ok = (uint32_t)__builtin_popcount(flags) == (uint32_t)__builtin_popcount(pattern);
            const bool dense = rep & 1;
            const uint32_t kind = (uint32_t)(rng() % MLM_TIME_SLOTS), dy0 = (uint32_t)(rng() % ((dense ? MLM_REF_DY_DENSE : MLM_REF_DY_LIST) - 6u)),
                           xrel = dense ? (uint32_t)(rng() & 0xFFu) : 0u;
            const uint32_t base = mlm_ref_pack(0u, kind, dense, dy0, 0u, xrel), rsh = mlm_ref_row_shift(dense);
            for (; flags; flags &= flags - 1u, ++count) {
                uint32_t row, bits;
                mlm_sec_row_take(flags, mask, row, bits);
                ok = ok && row < 8u && !((seen >> row) & 1u) && ((pattern >> row) & 1u) && bits == (uint32_t)((mask >> (8u * row)) & 0xFFu);
                seen |= 1u << (row & 7u);
                bad_repack += mlm_ref_repack(base, rsh, row, bits) != mlm_ref_pack(bits, kind, dense, dy0, row, xrel);
                ++n_repack;
            }
            ok = ok && seen == pattern;
            bad_rows += !ok;
            ++n_rows;
        }
    // ---- the miss passes' row of a mask word: every RW up to 64 words (nRho <= 512 on the sector path: 16), every w below 2^16 (nZ * nRho < 65 536)
    for (unsigned int rw = 1; rw <= 64u; ++rw) {
        const uint32_t mg = strip_magic(rw);
        for (uint32_t w = 0; w < 65536u; ++w) {
            bad_miss += (uint32_t)(((uint64_t)(w << 1) * mg) >> 32) != w / rw;
            ++n_miss;
        }
    }
    std::printf("n_origin %llu bad_origin %llu n_row_ends %llu n_rows %llu bad_rows %llu n_repack %llu bad_repack %llu n_miss %llu bad_miss %llu\n", n_origin, bad_origin,
                n_row_ends, n_rows, bad_rows, n_repack, bad_repack, n_miss, bad_miss);
    return 0;
}
