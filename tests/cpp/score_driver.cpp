// Test driver for mlm_score_poses on the host: the rule of mlmapping_amd/csrc/mlm_score.h (the arithmetic the kernel k_score runs too)
// under MapView::score (mlm_mapview.h, what the library answers small batches with) — built by tests/test_score_plan.py with
// g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n, n_blocks, n_pts, n_poses, n_fields, n_cases i32;
// lo[3], dims[3] i32; cases [n_cases][3] i32 (classes 0 / 1, field index or -1, sq_cap); keys [n_blocks*3] i32; collapsed [n_blocks] u8;
// occ, infl [n_blocks*cells] u8; pts [n_pts*3] f64; T [n_poses*12] f64; fields [n_fields][dims2*dims1*dims0] i32.  Output: per case and
// pose the eight words of its row.
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
    int32_t hdr[6], box[6]; // n, n_blocks, n_pts, n_poses, n_fields, n_cases; lo, dims
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr) || !rd(f, box, sizeof box)) return 2;
    const int n = hdr[0], nb = hdr[1], np = hdr[2], nk = hdr[3], nf = hdr[4], nc = hdr[5], C = n * n * n;
    const size_t nvox = (size_t)box[3] * box[4] * box[5];
    std::vector<int32_t> cases((size_t)nc * 3), keys((size_t)nb * 3), fields((size_t)nf * nvox);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C);
    std::vector<double> pts((size_t)np * 3), T((size_t)nk * 12);
    if (!rd(f, cases.data(), cases.size() * 4) || !rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) ||
        !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) || !rd(f, pts.data(), pts.size() * 8) || !rd(f, T.data(), T.size() * 8) ||
        !rd(f, fields.data(), fields.size() * 4))
        return 2;
    std::fclose(f);
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n; // map_local.cpp:60
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);
    // a view with no planes at all: what a field-only call runs on
    mlm_host::MapView bare;
    bare.d_sub = d_sub;
    bare.n = n;
    std::vector<int64_t> table((size_t)nk * MLM_SCORE_WORDS), one(MLM_SCORE_WORDS);
    for (int k = 0; k < nc; ++k) {
        const bool classes = cases[3 * (size_t)k] != 0;
        const int fi = cases[3 * (size_t)k + 1];
        if (fi >= nf || (!classes && fi < 0)) return 3;
        MlmScoreField F{};
        if (fi >= 0) {
            F.sqdist = fields.data() + (size_t)fi * nvox;
            for (int a = 0; a < 3; ++a) F.lo[a] = box[a], F.dims[a] = box[3 + a];
            F.cap = cases[3 * (size_t)k + 2];
        }
        std::fill(table.begin(), table.end(), (int64_t)-7);
        (classes ? v : bare).score(pts.data(), np, T.data(), nk, classes, F, table.data());
        for (int i = 0; i < nk; ++i) {
            // the batch form, then the pose on its own
            (classes ? v : bare).score(pts.data(), np, &T[12 * (size_t)i], 1, classes, F, one.data());
            if (std::memcmp(one.data(), &table[MLM_SCORE_WORDS * (size_t)i], sizeof(int64_t) * MLM_SCORE_WORDS)) return 4;
            for (int w = 0; w < MLM_SCORE_WORDS; ++w) std::printf("%lld%c", (long long)one[(size_t)w], w + 1 < MLM_SCORE_WORDS ? ' ' : '\n');
        }
    }
    return 0;
}
