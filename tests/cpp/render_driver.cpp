// Test driver for mlm_render_depth on the host: the pinhole arithmetic of mlmapping_amd/csrc/mlm_render.h (what the kernel k_render
// runs too) in front of the integer walk of mlm_raywalk.h over the classes of a block dump (MapView::ray, mlm_mapview.h) — built by
// tests/test_render_plan.py with g++ -fsanitize=address,undefined -ffp-contract=off (no HIP, no GPU).  Input blob: d_sub f64; n,
// n_blocks, n_flag_sets, n_cases, n_depth i32; flag sets [n_flag_sets] i32; keys [n_blocks*3] i32; collapsed [n_blocks] u8; occ, infl
// [n_blocks*cells] u8; per case T_ws [12] f64, K [4] f64, max_depth_mm, width, height i32; per depth case status, max_depth_mm i32,
// t f64.  Output: per case, flag set and pixel (u fastest) "status vx vy vz t n_steps n_unknown depth p0 (3) p1 (3)", then one
// depth per depth case (t, p0 and p1 as hex floats).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mlm_mapview.h"
#include "mlm_render.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double d_sub;
    int32_t hdr[5]; // n, n_blocks, n_flag_sets, n_cases, n_depth
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr)) return 2;
    const int n = hdr[0], nb = hdr[1], nf = hdr[2], nc = hdr[3], nd = hdr[4], C = n * n * n;
    std::vector<int32_t> flags((size_t)nf), keys((size_t)nb * 3);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    if (!rd(f, flags.data(), flags.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()))
        return 2;
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n;
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    for (int c = 0; c < nc; ++c) {
        double T[12], K[4];
        int32_t g[3]; // max_depth_mm, width, height
        if (!rd(f, T, sizeof T) || !rd(f, K, sizeof K) || !rd(f, g, sizeof g)) return 2;
        const double Z = (double)g[0] / 1000.0;
        for (int k = 0; k < nf; ++k)
            for (int y = 0; y < g[2]; ++y)
                for (int x = 0; x < g[1]; ++x) {
                    double p0[3], p1[3];
                    mlm_render_segment(T, T + 9, K, Z, x, y, p0, p1);
                    MlmRayResult o;
                    v.ray(p0, p1, flags[(size_t)k], o);
                    std::printf("%d %d %d %d %a %d %d %d %a %a %a %a %a %a\n", o.status, o.voxel[0], o.voxel[1], o.voxel[2], o.t, o.n_steps, o.n_unknown,
                                mlm_render_depth_mm(o.status, o.t, g[0]), p0[0], p0[1], p0[2], p1[0], p1[1], p1[2]);
                }
    }
    for (int i = 0; i < nd; ++i) {
        int32_t sm[2];
        double t;
        if (!rd(f, sm, sizeof sm) || !rd(f, &t, 8)) return 2;
        std::printf("%d\n", mlm_render_depth_mm(sm[0], t, sm[1]));
    }
    std::fclose(f);
    return 0;
}
