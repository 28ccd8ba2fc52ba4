// Test driver for the read-outs' host arithmetic (mlmapping_amd/csrc/mlm_host.h): mlm_brick_cover, mlm_box_check, mlm_stage_layout
// and mlm_export_window's use of mlm_esdf_plan, built by tests/test_readout_host.py with g++ -fsanitize=address,undefined.
//   readout_host_driver cover                     n lo d  b0 nb          a sweep of brick edges, origins (around 0 and the int32 edges) and extents
//   readout_host_driver box LO0 LO1 LO2 D0 D1 D2 ...   rc D0 D1 D2 nvox  per case (D and nvox as the call left them; preset to -7)
//   readout_host_driver layout N (PRESENT STAGED ELEM COUNT) x N ...   off[0] .. off[N - 1] total  per case
//   readout_host_driver window                    D0 D1 D2 H grad staged  T0 T1 T2 (mlm_esdf_plan)  T0 T1 T2 (the rule below)
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mlm_host.h"

// mlm_export_window's tile rule as it stood before it called mlm_esdf_plan, kept here for the comparison alone
static void window_rule_before(const long long D[3], long long H, long long box_cap, long long out_cap, long long T[3]) {
    auto fits = [&](long long tx, long long ty, long long tz) { return (tx + 2 * H) * (ty + 2 * H) * (tz + 2 * H) <= box_cap && tx * ty * tz <= out_cap; };
    if (fits(D[0], D[1], 1)) {
        T[0] = D[0];
        T[1] = D[1];
        T[2] = std::min({D[2], box_cap / ((D[0] + 2 * H) * (D[1] + 2 * H)) - 2 * H, out_cap / (D[0] * D[1])});
    } else if (fits(D[0], 1, 1)) {
        T[0] = D[0];
        T[1] = std::min({D[1], box_cap / ((D[0] + 2 * H) * (1 + 2 * H)) - 2 * H, out_cap / D[0]});
        T[2] = 1;
    } else {
        T[0] = std::min({D[0], box_cap / ((1 + 2 * H) * (1 + 2 * H)) - 2 * H, out_cap});
        T[1] = T[2] = 1;
    }
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "cover")) {
        for (int n : {1, 2, 3, 4, 5, 8, 16}) {
            std::vector<long long> los;
            for (long long lo = -2 * n - 1; lo <= 2 * n + 1; ++lo) los.push_back(lo);
            for (long long c : {(long long)INT32_MIN - 64, (long long)INT32_MIN, (long long)INT32_MAX, (long long)INT32_MAX + 64})
                for (long long k = -8; k <= 8; ++k) los.push_back(c + k);
            for (long long lo : los)
                for (long long d : {1ll, 2ll, (long long)n - 1, (long long)n, (long long)n + 1, 130ll}) {
                    if (d < 1) continue;
                    long long b0 = -7;
                    int nb = -7;
                    mlm_brick_cover(n, lo, d, b0, nb);
                    std::printf("%d %lld %lld %lld %d\n", n, lo, d, b0, nb);
                }
        }
        return 0;
    }
    if (!std::strcmp(mode, "box")) {
        for (int i = 2; i + 5 < argc; i += 6) {
            int32_t lo[3], dims[3];
            for (int a = 0; a < 3; ++a) {
                lo[a] = (int32_t)std::atoll(argv[i + a]);
                dims[a] = (int32_t)std::atoll(argv[i + 3 + a]);
            }
            long long D[3] = {-7, -7, -7}, nvox = -7;
            const int rc = mlm_box_check(lo, dims, D, nvox);
            std::printf("%d %lld %lld %lld %lld\n", rc, D[0], D[1], D[2], nvox);
        }
        return 0;
    }
    if (!std::strcmp(mode, "layout")) {
        for (int i = 2; i < argc;) {
            const int N = std::atoi(argv[i++]);
            if (N < 1 || i + 4 * N > argc) return 2;
            std::unique_ptr<bool[]> present(new bool[(size_t)N]), staged(new bool[(size_t)N]);
            std::vector<size_t> elem((size_t)N), count((size_t)N), off((size_t)N, (size_t)-7);
            for (int c = 0; c < N; ++c, i += 4) {
                present[c] = std::atoi(argv[i]) != 0;
                staged[c] = std::atoi(argv[i + 1]) != 0;
                elem[(size_t)c] = (size_t)std::atoll(argv[i + 2]);
                count[(size_t)c] = (size_t)std::atoll(argv[i + 3]);
            }
            const size_t total = mlm_stage_layout(N, present.get(), staged.get(), elem.data(), count.data(), off.data());
            for (int c = 0; c < N; ++c) std::printf("%zu ", off[(size_t)c]);
            std::printf("%zu\n", total);
        }
        return 0;
    }
    if (!std::strcmp(mode, "window")) {
        const long long dims[] = {1, 2, 7, 64, 129, 500, 1000, 4096, 65536, 1ll << 20}; // (esdf_plan_driver's sweep)
        for (long long d0 : dims)
            for (long long d1 : dims)
                for (long long d2 : dims) {
                    if (d0 * d1 > 0x7FFFFFFFll || d0 * d1 * d2 > 0x7FFFFFFFll) continue;
                    const long long D[3] = {d0, d1, d2};
                    for (long long H = 0; H <= 8; ++H)
                        for (int grad = 0; grad < 2; ++grad) {
                            if (!grad && H) continue; // (no gradients: no halo)
                            for (int staged = 0; staged < 2; ++staged) {
                                const long long box_cap = grad ? kEsdfBoxVoxels : 1ll << 62, out_cap = staged ? kEsdfStageVoxels : 1ll << 62;
                                const MlmEsdfPlan p = mlm_esdf_plan(D, (int)H + 1, false, box_cap, out_cap);
                                long long T[3];
                                window_rule_before(D, H, box_cap, out_cap, T);
                                std::printf("%lld %lld %lld %lld %d %d  %lld %lld %lld  %lld %lld %lld  %lld %lld\n", d0, d1, d2, H, grad, staged, p.T[0],
                                            p.T[1], p.T[2], T[0], T[1], T[2], p.H, p.grown);
                            }
                        }
                }
        return 0;
    }
    return 2;
}
