// Test driver for mlm_esdf_plan (mlmapping_amd/csrc/mlm_host.h): the tiles of mlm_export_esdf, built by tests/test_esdf_plan.py
// with g++ -fsanitize=address,undefined.  One line per case:
//   D0 D1 D2 C grad box_cap out_cap  T0 T1 T2  n0 n1 n2  H grown
//   esdf_plan_driver D0 D1 D2 C GRAD BOX OUT ...   the cases given (7 numbers each; OUT 0: no staging cap)
//   esdf_plan_driver sweep                         a sweep of window dims, C, gradients on / off, the default and the smallest
//                                                  voxel cap, with and without the staging cap
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlm_host.h"

static void row(long long d0, long long d1, long long d2, int C, int grad, long long box, long long out) {
    const long long D[3] = {d0, d1, d2};
    const MlmEsdfPlan p = mlm_esdf_plan(D, C, grad != 0, box, out ? out : (1ll << 62));
    std::printf("%lld %lld %lld %d %d %lld %lld  %lld %lld %lld  %lld %lld %lld  %lld %lld\n", d0, d1, d2, C, grad, box, out, p.T[0], p.T[1],
                p.T[2], p.n[0], p.n[1], p.n[2], p.H, p.grown);
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const long long dims[] = {1, 2, 7, 64, 129, 500, 1000, 4096, 65536, 1ll << 20};
        const int Cs[] = {1, 2, 5, 16, 32, 63, 64};
        const long long boxes[] = {kEsdfBoxVoxels, kEsdfMinBoxVoxels, 3000000};
        for (long long d0 : dims)
            for (long long d1 : dims)
                for (long long d2 : dims) {
                    if (d0 * d1 > 0x7FFFFFFFll || d0 * d1 * d2 > 0x7FFFFFFFll) continue;
                    for (int C : Cs)
                        for (int g = 0; g < 2; ++g)
                            for (long long box : boxes)
                                for (long long out : {0ll, kEsdfStageVoxels}) row(d0, d1, d2, C, g, box, out);
                }
        return 0;
    }
    for (int i = 1; i + 6 < argc; i += 7)
        row(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4]),
            std::atoll(argv[i + 5]), std::atoll(argv[i + 6]));
    return 0;
}
