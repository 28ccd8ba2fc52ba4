// Test driver for mlm_apply_lds (mlmapping_amd/csrc/mlm_host.h): the dynamic LDS layout of k_apply_tiles, built by
// tests/test_gpu_apply_footprint.py with g++ -fsanitize=address,undefined.
//   apply_lds_driver EDGE NZ N ...   one line per triple: edge nz n occ ztab blk total
//   apply_lds_driver sweep           the same for a sweep of geometries, with the most blocks a tile column of edge x edge x nz
//                                    voxels overlaps at any grid offset (counted, not bounded): ... max_bxy max_bz
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlm_host.h"

static int floor_div(int a, int n) { // k_apply_tiles' mlm_floor_div
    int q = a / n;
    if ((a % n) < 0) --q;
    return q;
}
static int blocks_over(int extent, int n) { // most blocks of n an extent covers, over every offset (and negative ones)
    int m = 0;
    for (int o = -2 * n; o < 2 * n; ++o) {
        const int c = floor_div(o + extent - 1, n) - floor_div(o, n) + 1;
        if (c > m) m = c;
    }
    return m;
}
static void row(uint32_t edge, uint32_t nz, uint32_t n, bool counted) {
    const MlmApplyLds L = mlm_apply_lds(edge, nz, n);
    std::printf("%u %u %u %u %u %u %u", edge, nz, n, L.occ, L.ztab, L.blk, L.total);
    if (counted) std::printf(" %d %d", blocks_over((int)edge, (int)n), blocks_over((int)nz, (int)n));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const uint32_t edges[] = {1, 2, 4, 8}, ns[] = {1, 2, 3, 5, 7, 10, 16, 31, 64, 255};
        for (uint32_t e : edges)
            for (uint32_t n : ns)
                for (uint32_t nz = 1; nz <= 2048; nz = nz < 24 ? nz + 1 : nz * 5 / 4 + 1) row(e, nz, n, true);
        return 0;
    }
    for (int i = 1; i + 2 < argc; i += 3) row((uint32_t)std::atoi(argv[i]), (uint32_t)std::atoi(argv[i + 1]), (uint32_t)std::atoi(argv[i + 2]), false);
    return 0;
}
