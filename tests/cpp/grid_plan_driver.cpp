// Test driver for mlm_grid_plan (mlmapping_amd/csrc/mlm_host.h): the tiles of mlm_export_grid2d, built by tests/test_grid_plan.py
// with g++ -fsanitize=address,undefined.  One line per case:
//   D0 D1 C dist box_cap out_cap  T0 T1  n0 n1  H grown
//   grid_plan_driver D0 D1 C DIST BOX OUT ...   the cases given (6 numbers each; OUT 0: no cell cap)
//   grid_plan_driver sweep                      a sweep of plane dims, C, distances on / off, the default and the smallest box cap,
//                                               without a cell cap, with the staging cap and with small "grid_tile" caps
//   grid_plan_driver knob V ...                 one line "V ok" per value: mlm_grid_tile_ok, the range check of the knob
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlm_host.h"

static void row(long long d0, long long d1, int C, int dist, long long box, long long out) {
    const long long D[2] = {d0, d1};
    const MlmGridPlan p = mlm_grid_plan(D, C, dist != 0, box, out ? out : (1ll << 62));
    std::printf("%lld %lld %d %d %lld %lld  %lld %lld  %lld %lld  %lld %lld\n", d0, d1, C, dist, box, out, p.T[0], p.T[1], p.n[0], p.n[1], p.H,
                p.grown);
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const long long dims[] = {1, 2, 7, 64, 129, 500, 1000, 4096, 65536, 1ll << 20, (1ll << 31) - 1};
        const int Cs[] = {1, 2, 5, 16, 32, 63, 64};
        const long long boxes[] = {kGridBoxCells, kGridMinBoxCells, 300000};
        const long long outs[] = {0, kGridStageCells, 1, 2, 50, 4097};
        for (long long d0 : dims)
            for (long long d1 : dims) {
                if (d0 * d1 > 0x7FFFFFFFll) continue;
                for (int C : Cs)
                    for (int g = 0; g < 2; ++g)
                        for (long long box : boxes)
                            for (long long out : outs) row(d0, d1, C, g, box, out);
            }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "knob")) {
        for (int i = 2; i < argc; ++i) std::printf("%lld %d\n", std::atoll(argv[i]), (int)mlm_grid_tile_ok(std::atoll(argv[i])));
        return 0;
    }
    for (int i = 1; i + 5 < argc; i += 6)
        row(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoll(argv[i + 4]),
            std::atoll(argv[i + 5]));
    return 0;
}
