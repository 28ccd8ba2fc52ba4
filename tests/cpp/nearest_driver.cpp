// Test driver for mlm_query_nearest on the host: the search of mlmapping_amd/csrc/mlm_nearest.h (the control flow the kernel k_nearest
// runs too) under MapView::nearest (mlm_mapview.h, what the library's host mirror answers small batches with) — built by
// tests/test_nearest_plan.py with g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n, n_blocks, n_points,
// n_cases i32; cases [n_cases][2] i32 (flags, max_dist); keys [n_blocks*3] i32; collapsed [n_blocks] u8; occ, infl [n_blocks*cells] u8;
// points [n_points*3] f64.  Output: per case and point "status voxel3 delta3 sq dist", dist as the 16 hex digits of its bits.
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
    int32_t hdr[4]; // n, n_blocks, n_points, n_cases
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr)) return 2;
    const int n = hdr[0], nb = hdr[1], np = hdr[2], nc = hdr[3], C = n * n * n;
    std::vector<int32_t> cases((size_t)nc * 2), keys((size_t)nb * 3);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    std::vector<double> pos((size_t)np * 3);
    if (!rd(f, cases.data(), cases.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) || !rd(f, pos.data(), pos.size() * 8))
        return 2;
    std::fclose(f);
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n; // map_local.cpp:60
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    // an empty view: every voxel UNKNOWN — nothing without the bit; with it the point's own voxel, or on a face the one below
    {
        const double mid[3] = {0.5 * d_sub, 0.5 * d_sub, 0.5 * d_sub}, face[3] = {0.5 * d_sub, 0.0, 0.5 * d_sub};
        MlmNearResult o;
        v.nearest_one(mid, 3, 1, o);
        if (o.status != 0 || o.voxel[0] != 0 || o.sq != -1 || o.dist != -1.0) return 3;
        v.nearest_one(mid, 3, 4, o);
        if (o.status != 1 || o.voxel[0] != 0 || o.voxel[1] != 0 || o.voxel[2] != 0 || o.sq != 0 || o.dist != 0.0) return 3;
        v.nearest_one(face, 3, 4, o);
        if (o.status != 1 || o.voxel[0] != 0 || o.voxel[1] != -1 || o.voxel[2] != 0 || o.delta[1] != -512 || o.sq != 512 * 512) return 3;
    }
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    std::vector<int8_t> st((size_t)np);
    std::vector<int32_t> vx((size_t)np * 3), dl((size_t)np * 3);
    std::vector<int64_t> sq((size_t)np);
    std::vector<double> dist((size_t)np);
    for (int k = 0; k < nc; ++k) {
        const int flags = cases[2 * (size_t)k], md = cases[2 * (size_t)k + 1];
        // the batch form, then one point per call with a single output each (null outputs are skipped)
        v.nearest(pos.data(), np, md, flags, st.data(), vx.data(), dl.data(), sq.data(), dist.data());
        for (int i = 0; i < np; ++i) {
            MlmNearResult o;
            v.nearest_one(&pos[3 * (size_t)i], md, flags, o);
            int64_t one = -7;
            v.nearest(&pos[3 * (size_t)i], 1, md, flags, nullptr, nullptr, nullptr, &one, nullptr);
            if (o.status != st[(size_t)i] || o.voxel[2] != vx[3 * (size_t)i + 2] || one != sq[(size_t)i]) return 4;
            unsigned long long bits;
            std::memcpy(&bits, &dist[(size_t)i], 8);
            std::printf("%d %d %d %d %d %d %d %lld %016llx\n", (int)st[(size_t)i], vx[3 * (size_t)i], vx[3 * (size_t)i + 1], vx[3 * (size_t)i + 2],
                        dl[3 * (size_t)i], dl[3 * (size_t)i + 1], dl[3 * (size_t)i + 2], (long long)sq[(size_t)i], bits);
        }
    }
    return 0;
}
