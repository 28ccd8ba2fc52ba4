// Test driver for mlm_query_sweeps on the host: the walk of mlmapping_amd/csrc/mlm_sweep.h (the control flow the kernel k_sweeps runs
// too) under MapView::sweep (mlm_mapview.h, what the library's host mirror answers small batches with) — built by
// tests/test_sweep_plan.py with g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n, n_blocks, n_rays,
// n_cases i32; cases [n_cases][2] i32 (flags, radius); keys [n_blocks*3] i32; collapsed [n_blocks] u8; occ, infl [n_blocks*cells] u8;
// p0, p1 [n_rays*3] f64.  Output: per case and ray "status voxel3 t n_steps n_unknown hit3 hit_sq", t as the 16 hex digits of its bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_mapview.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double d_sub;
    int32_t hdr[4]; // n, n_blocks, n_rays, n_cases
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr)) return 2;
    const int n = hdr[0], nb = hdr[1], nr = hdr[2], nc = hdr[3], C = n * n * n;
    std::vector<int32_t> cases((size_t)nc * 2), keys((size_t)nb * 3);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    std::vector<double> p0((size_t)nr * 3), p1((size_t)nr * 3);
    if (!rd(f, cases.data(), cases.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) || !rd(f, p0.data(), p0.size() * 8) || !rd(f, p1.data(), p1.size() * 8))
        return 2;
    std::fclose(f);
    // the column tables: L(r) of the contract, every column inside the disc, m the largest that stays inside the ball
    {
        static const int want[17] = {1, 5, 13, 29, 49, 81, 113, 149, 197, 253, 317, 377, 441, 529, 613, 709, 797};
        std::vector<uint32_t> tab(MLM_SWEEP_MAX_COLS);
        for (int r = 0; r <= MLM_SWEEP_MAX_R; ++r) {
            const int L = mlm_sweep_table(r, tab.data());
            if (L != want[r] || L != mlm_sweep_columns(r)) return 3;
            for (int j = 0; j < L; ++j) {
                const int p = (int)(tab[j] & 63u) - 16, q = (int)((tab[j] >> 6) & 63u) - 16, m = (int)((tab[j] >> 12) & 31u), sq = (int)(tab[j] >> 18);
                if (sq != m * m + p * p + q * q || sq > r * r || (m + 1) * (m + 1) + p * p + q * q <= r * r) return 3;
            }
        }
    }
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n; // map_local.cpp:60
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    std::vector<int8_t> st((size_t)nr);
    std::vector<int32_t> vx((size_t)nr * 3), hit((size_t)nr * 3), ns((size_t)nr), nu((size_t)nr), hsq((size_t)nr);
    std::vector<double> t((size_t)nr);
    for (int k = 0; k < nc; ++k) {
        const int flags = cases[2 * (size_t)k], radius = cases[2 * (size_t)k + 1];
        // the batch form, then one ray per call with a single output (null outputs are skipped)
        v.sweep(p0.data(), p1.data(), nr, radius, flags, st.data(), vx.data(), t.data(), ns.data(), nu.data(), hit.data(), hsq.data());
        for (int i = 0; i < nr; ++i) {
            int32_t one = -7;
            v.sweep(&p0[3 * (size_t)i], &p1[3 * (size_t)i], 1, radius, flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &one);
            if (one != hsq[(size_t)i]) return 4;
            unsigned long long bits;
            std::memcpy(&bits, &t[(size_t)i], 8);
            std::printf("%d %d %d %d %016llx %d %d %d %d %d %d\n", (int)st[(size_t)i], vx[3 * (size_t)i], vx[3 * (size_t)i + 1], vx[3 * (size_t)i + 2], bits,
                        ns[(size_t)i], nu[(size_t)i], hit[3 * (size_t)i], hit[3 * (size_t)i + 1], hit[3 * (size_t)i + 2], hsq[(size_t)i]);
        }
    }
    return 0;
}
