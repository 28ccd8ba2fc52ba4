// Test driver for the read-outs' host arithmetic (mlmapping_amd/csrc/mlm_host.h): mlm_brick_cover, mlm_box_check, mlm_stage_layout
// and mlm_export_window's use of mlm_esdf_plan, built by tests/test_readout_host.py with g++ -fsanitize=address,undefined.
//   readout_host_driver cover                     n lo d  b0 nb          a sweep of brick edges, origins (around 0 and the int32 edges) and extents
//   readout_host_driver box LO0 LO1 LO2 D0 D1 D2 ...   rc D0 D1 D2 nvox  per case (D and nvox as the call left them; preset to -7)
//   readout_host_driver layout N (PRESENT STAGED ELEM COUNT) x N ...   off[0] .. off[N - 1] total  per case
//   readout_host_driver window                    D0 D1 D2 H grad staged  T0 T1 T2 (mlm_esdf_plan)  T0 T1 T2 (the rule below)
//   readout_host_driver tiles (DIMS D0 D1 D2 T0 T1 T2) ...   the tiles of mlm_for_tiles and of the loops it replaced; tiles_stop: its early end
//   readout_host_driver rows                      mlm_stage_rows against the three lines of crop_run it replaced
// (MlmCtrlBlock's layout is checked by the static_assert beside it, which this translation unit compiles.)
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

// the tile walk of mlm_export_window, mlm_export_esdf and esdf_tiles (and, with two loops, of mlm_export_grid2d) as each of them spelled
// it out before mlm_for_tiles, kept here for the comparison alone
template <class F> static void tiles_before(const long long D[3], const long long T[3], F fn) {
    for (long long z0 = 0; z0 < D[2]; z0 += T[2])
        for (long long y0 = 0; y0 < D[1]; y0 += T[1])
            for (long long x0 = 0; x0 < D[0]; x0 += T[0]) {
                const long long org[3] = {x0, y0, z0};
                int td[3];
                for (int a = 0; a < 3; ++a) td[a] = (int)std::min(T[a], D[a] - org[a]);
                fn(org, td, (z0 * D[1] + y0) * D[0] + x0);
            }
}
template <class F> static void tiles2d_before(const long long D[2], const long long T[2], F fn) {
    for (long long y0 = 0; y0 < D[1]; y0 += T[1])
        for (long long x0 = 0; x0 < D[0]; x0 += T[0]) {
            const long long org[3] = {x0, y0, 0};
            int td[3] = {0, 0, 1};
            for (int a = 0; a < 2; ++a) td[a] = (int)std::min(T[a], D[a] - org[a]);
            fn(org, td, y0 * D[0] + x0);
        }
}
// the rows per round of crop_run's page-out as its three lines computed them before mlm_stage_rows (per_row > 0: something is staged)
static size_t stage_rows_before(size_t D, size_t per_row, size_t cap_bytes, bool any_staged, bool knob_set, long long kv) {
    size_t rows = !any_staged ? (size_t)D : std::min<size_t>(D, std::max<size_t>(1, cap_bytes / per_row));
    if (any_staged && knob_set) rows = std::min<size_t>(D, (size_t)kv);
    return rows;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "tiles")) { // (DIMS D0 D1 D2 T0 T1 T2) ...: which (0: mlm_for_tiles, 1: before) case org[3] td[3] out_base per tile
        for (int i = 2, k = 0; i + 6 < argc; i += 7, ++k) {
            const int nd = std::atoi(argv[i]);
            long long D[3], T[3];
            for (int a = 0; a < 3; ++a) D[a] = std::atoll(argv[i + 1 + a]), T[a] = std::atoll(argv[i + 4 + a]);
            auto row = [&](int which) {
                return [k, which](const long long org[3], const int td[3], long long base) {
                    std::printf("%d %d %lld %lld %lld %d %d %d %lld\n", which, k, org[0], org[1], org[2], td[0], td[1], td[2], base);
                    return 0;
                };
            };
            if (mlm_for_tiles(D, T, row(0))) return 3;
            if (nd == 2)
                tiles2d_before(D, T, row(1));
            else
                tiles_before(D, T, row(1));
        }
        return 0;
    }
    if (!std::strcmp(mode, "tiles_stop")) { // the walk ends at the first non-zero answer: calls made, value returned
        const long long D[3] = {5, 3, 2}, T[3] = {2, 2, 1};
        int calls = 0;
        const int rc = mlm_for_tiles(D, T, [&](const long long *, const int *, long long) { return ++calls == 3 ? 7 : 0; });
        std::printf("%d %d\n", calls, rc);
        return 0;
    }
    if (!std::strcmp(mode, "rows")) { // n per_row cap knob  rows (mlm_stage_rows)  rows (before)
        const size_t wide = 12 + 6 * 512;
        for (size_t n : {(size_t)1, (size_t)2, (size_t)1000})
            for (size_t per_row : {(size_t)0, (size_t)1, (size_t)12, wide})
                for (size_t cap : {(size_t)1, per_row ? per_row - 1 : 0, per_row, (size_t)64 << 20})
                    for (long long kv : {0ll, 1ll, (long long)n + 5}) // (0: the knob is not set)
                        std::printf("%zu %zu %zu %lld %zu %zu\n", n, per_row, cap, kv, mlm_stage_rows(n, per_row, cap, kv),
                                    stage_rows_before(n, per_row, cap, per_row != 0, kv != 0, kv));
        return 0;
    }
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
