// Test driver for the segment casts of mlm_query_rays on the host: the integer walk of mlmapping_amd/csrc/mlm_raywalk.h (the
// arithmetic the kernel k_rays runs too) under MapView::ray (mlm_mapview.h, what the library's host mirror answers small batches
// with) — built by tests/test_ray_walk.py with g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n,
// n_blocks, n_rays, n_flag_sets i32; flag sets [n_flag_sets] i32; keys [n_blocks*3] i32; collapsed [n_blocks] u8; occ, infl
// [n_blocks*cells] u8; p0, p1 [n_rays*3] f64.  Output: per flag set and ray "status vx vy vz t n_steps n_unknown" (t as a hex float).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mlm_mapview.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double d_sub;
    int32_t hdr[4]; // n, n_blocks, n_rays, n_flag_sets
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr)) return 2;
    const int n = hdr[0], nb = hdr[1], nr = hdr[2], nf = hdr[3], C = n * n * n;
    std::vector<int32_t> flags((size_t)nf), keys((size_t)nb * 3);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    std::vector<double> p0((size_t)nr * 3), p1((size_t)nr * 3);
    if (!rd(f, flags.data(), flags.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) || !rd(f, p0.data(), p0.size() * 8) || !rd(f, p1.data(), p1.size() * 8))
        return 2;
    std::fclose(f);
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n; // map_local.cpp:60
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    // an empty view: every voxel UNKNOWN
    {
        const double a[3] = {0.05 * d_sub, 0.5 * d_sub, 0.5 * d_sub}, b[3] = {3.5 * d_sub, 0.5 * d_sub, 0.5 * d_sub};
        MlmRayResult o;
        v.ray(a, b, 1, o);
        if (o.status != 0 || o.n_steps != 4 || o.n_unknown != 4 || o.voxel[0] != 3 || o.t != 1.0) return 3;
        v.ray(a, b, 4, o);
        if (o.status != 1 || o.n_steps != 0 || o.n_unknown != 0 || o.voxel[0] != 0 || o.t != 0.0) return 3;
    }
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    std::vector<int8_t> st((size_t)nr);
    std::vector<int32_t> vox((size_t)nr * 3), ns((size_t)nr), nu((size_t)nr);
    std::vector<double> t((size_t)nr);
    for (int k = 0; k < nf; ++k) {
        // the batch form, then one ray per call with a single output each (null outputs are skipped)
        v.rays(p0.data(), p1.data(), nr, flags[(size_t)k], st.data(), vox.data(), t.data(), ns.data(), nu.data());
        for (int i = 0; i < nr; ++i) {
            MlmRayResult o;
            v.ray(&p0[3 * (size_t)i], &p1[3 * (size_t)i], flags[(size_t)k], o);
            int32_t one = -7;
            v.rays(&p0[3 * (size_t)i], &p1[3 * (size_t)i], 1, flags[(size_t)k], nullptr, nullptr, nullptr, &one, nullptr);
            if (o.status != st[(size_t)i] || o.n_steps != ns[(size_t)i] || one != ns[(size_t)i]) return 4;
            std::printf("%d %d %d %d %a %d %d\n", (int)st[(size_t)i], vox[3 * (size_t)i], vox[3 * (size_t)i + 1], vox[3 * (size_t)i + 2], t[(size_t)i],
                        ns[(size_t)i], nu[(size_t)i]);
        }
    }
    return 0;
}
