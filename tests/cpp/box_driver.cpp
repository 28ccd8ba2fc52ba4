// Test driver for mlm_query_boxes on the host: the growth of mlmapping_amd/csrc/mlm_boxgrow.h (the control flow the kernel k_boxes
// runs too) under MapView::boxes (mlm_mapview.h, what the library's host mirror answers small batches with) — built by
// tests/test_box_grow.py with g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n, n_blocks, n_boxes,
// n_cases i32; cases [n_cases][14] i32 (flags, window given, max_grow[6], window lo[3], window dims[3]); keys [n_blocks*3] i32;
// collapsed [n_blocks] u8; occ, infl [n_blocks*cells] u8; boxes [n_boxes*6] i32.  Output: per case and box
// "status lo3 hi3 closed row4".
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
    int32_t hdr[4]; // n, n_blocks, n_boxes, n_cases
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr)) return 2;
    const int n = hdr[0], nb = hdr[1], nx = hdr[2], nc = hdr[3], C = n * n * n;
    std::vector<int32_t> cases((size_t)nc * 14), keys((size_t)nb * 3), boxes((size_t)nx * 6);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    if (!rd(f, cases.data(), cases.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) || !rd(f, boxes.data(), boxes.size() * 4))
        return 2;
    std::fclose(f);
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n; // map_local.cpp:60
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    // an empty view: every voxel UNKNOWN — nothing blocks without the bit, the start is blocked with it
    {
        const int32_t b[6] = {-1, -1, -1, 1, 1, 1};
        MlmBoxLimits L{};
        for (int c = 0; c < 6; ++c) L.grow[c] = 2;
        MlmBoxResult o;
        v.box(b, 1, L, o);
        if (o.status != 1 || o.box[0] != -3 || o.box[5] != 3 || o.closed != 0 || o.row[0] != 343 || o.row[1] != 343 || o.row[3] != 12) return 3;
        v.box(b, 4, L, o);
        if (o.status != 0 || o.box[0] != -1 || o.row[0] != 27 || o.row[2] != 27 || o.row[3] != 0) return 3;
    }
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    std::vector<int8_t> st((size_t)nx);
    std::vector<int32_t> out((size_t)nx * 6);
    std::vector<uint8_t> cl((size_t)nx);
    std::vector<int64_t> tab((size_t)nx * 4);
    for (int k = 0; k < nc; ++k) {
        const int32_t *cs = &cases[(size_t)k * 14];
        MlmBoxLimits L{};
        for (int c = 0; c < 6; ++c) L.grow[c] = cs[2 + c];
        L.on = cs[1];
        for (int a = 0; a < 3; ++a) {
            L.wlo[a] = cs[8 + a];
            L.whi[a] = L.on ? cs[8 + a] + (cs[11 + a] - 1) : 0;
        }
        // the batch form, then one box per call with a single output each (null outputs are skipped)
        v.boxes(boxes.data(), nx, cs[0], L, st.data(), out.data(), cl.data(), tab.data());
        for (int i = 0; i < nx; ++i) {
            MlmBoxResult o;
            v.box(&boxes[6 * (size_t)i], cs[0], L, o);
            int64_t row[4] = {-7, -7, -7, -7};
            v.boxes(&boxes[6 * (size_t)i], 1, cs[0], L, nullptr, nullptr, nullptr, row);
            if (o.status != st[(size_t)i] || o.row[0] != tab[4 * (size_t)i] || row[1] != tab[4 * (size_t)i + 1] || o.closed != cl[(size_t)i]) return 4;
            std::printf("%d", (int)st[(size_t)i]);
            for (int j = 0; j < 6; ++j) std::printf(" %d", out[6 * (size_t)i + j]);
            std::printf(" %u", (unsigned)cl[(size_t)i]);
            for (int j = 0; j < 4; ++j) std::printf(" %lld", (long long)tab[4 * (size_t)i + j]);
            std::printf("\n");
        }
    }
    return 0;
}
