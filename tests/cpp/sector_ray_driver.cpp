// The walk of one lane's share of a k_sector ray (mlm_sector_ray.h) on the CPU, against the reference's own sequence
// z' = round(z - k * ((z - zc) / rho)), k = 1 .. rho-1 (map_awareness.cpp:266-274, C round), clipped to the rows [0, nZ):
// every rho in 2 .. 512, every z, zc = (nZ - 1) / 2 for nZ = 41, 81, 161, with 4 and with 16 lanes per ray.
//   mask mode      the union of the lanes' visited (row, cell) sets plus their ties, resolved as the kernel resolves them, equals the reference's
//                  set; no cell is visited twice; a visit's bits stay in the cells the lane's share covers
//   frontier mode  every (row, cell) of the reference is visited exactly once, with cell = rho - step: the time t0 + step - 1 is k - 1
// Prints the counters the test asserts on.
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>

#include "mlm_sector_ray.h"

int main() {
    unsigned long long cases = 0, tie_cases = 0, tie_steps = 0, late_ties = 0, bad_mask = 0, bad_frontier = 0, twice = 0, visits = 0, steps = 0;
    const int NZ[3] = {41, 81, 161};
    std::vector<uint8_t> want(161 * 512), got(161 * 512), gotf(161 * 512);
    for (int nZ : NZ) {
        const int zc = (nZ - 1) / 2;
        for (int rho = 2; rho <= 512; ++rho)
            for (int z = 0; z < nZ; ++z) {
                std::memset(want.data(), 0, (size_t)nZ * 512);
                unsigned long long n_want = 0;
                const double slope = (z - zc) / (rho * 1.0);
                for (int k = 1; k < rho; ++k) {
                    const int zr = (int)round(z - (k * slope));
                    if (0 <= zr && zr < nZ) want[(size_t)zr * 512 + (rho - k)] = 1, ++n_want;
                }
                steps += (unsigned long long)(rho - 1);
                for (uint32_t sh : {2u, 4u}) {
                    std::memset(got.data(), 0, (size_t)nZ * 512);
                    std::memset(gotf.data(), 0, (size_t)nZ * 512);
                    bool any_tie = false;
                    for (uint32_t lane = 0; lane < (1u << sh); ++lane) {
                        int k_lo, k_hi;
                        mlm_sray_share(rho, lane, sh, k_lo, k_hi);
                        auto mark = [&](std::vector<uint8_t> &g, int row, int cell) {
                            if (row < 0 || row >= nZ || cell <= rho - k_hi || cell > rho - k_lo) { // (outside the rows, or outside the lane's share)
                                ++bad_mask;
                                return;
                            }
                            twice += g[(size_t)row * 512 + cell];
                            g[(size_t)row * 512 + cell] = 1;
                        };
                        auto resolve = [&](unsigned long long ties, std::vector<uint8_t> &g) { // (the kernel's tie loop)
                            for (; ties; ties &= ties - 1) {
                                const int k = k_lo + __builtin_ctzll(ties);
                                const int zr = mlm_sray_row_fp64(rho, z, zc, k);
                                ++tie_steps;
                                any_tie = true;
                                if (0 <= zr && zr < nZ) mark(g, zr, rho - k);
                            }
                        };
                        // (as the kernel calls it: a share in pieces of at most MLM_SRAY_MAX_STEPS steps, each piece's ties resolved after it)
                        const int s_lo = k_lo, s_hi = k_hi;
                        for (k_lo = s_lo; k_lo < s_hi; k_lo += MLM_SRAY_MAX_STEPS) {
                            k_hi = s_hi < k_lo + MLM_SRAY_MAX_STEPS ? s_hi : k_lo + MLM_SRAY_MAX_STEPS;
                            const unsigned long long before = tie_steps;
                            resolve(mlm_sray_walk<false>(rho, z, zc, nZ, k_lo, k_hi, [&](int row, int word, uint32_t bits) {
                                ++visits;
                                if (!bits || word < 0 || word > 15) ++bad_mask;
                                for (uint32_t b = bits; b; b &= b - 1) mark(got, row, word * 32 + __builtin_ctz(b));
                            }), got);
                            if (k_lo != s_lo) late_ties += tie_steps - before; // (ties of a later piece)
                            resolve(mlm_sray_walk<true>(rho, z, zc, nZ, k_lo, k_hi, [&](int row, int cell, uint32_t k) {
                                if (cell != rho - (int)k || (int)k < k_lo || (int)k >= k_hi) ++bad_frontier; // (time = t0 + k - 1: the step is the cell's)
                                mark(gotf, row, cell);
                            }), gotf);
                        }
                    }
                    bad_mask += std::memcmp(got.data(), want.data(), (size_t)nZ * 512) != 0;
                    bad_frontier += std::memcmp(gotf.data(), want.data(), (size_t)nZ * 512) != 0;
                    ++cases;
                    tie_cases += any_tie;
                }
                (void)n_want;
            }
    }
    std::printf("cases %llu tie_cases %llu tie_steps %llu late_ties %llu bad_mask %llu bad_frontier %llu twice %llu visits %llu steps %llu\n", cases, tie_cases, tie_steps,
                late_ties, bad_mask, bad_frontier, twice, visits, steps);
    return 0;
}
