// Test driver for mlm_query_paths on the host: mlmapping_amd/csrc/mlm_path.h (the rule the kernel k_paths and the entry point's host
// branch run too) with its serial executor — built by tests/test_path_plan.py with g++ -fsanitize=address,undefined (no HIP, no GPU).
// Input blob: 11 x i32 (dx, dy, dz, lo[3], kind, n, lookahead, max_moves, cap); d f64 (already (double)(float)subbox_d_xyz); parent
// [dz*dy*dx] u8; goals [n*3] i32; way [n*cap*3] i32, the buffer's content before the call.  Output blob: status [n] i8, way
// [n*cap*3] i32, length [n] f64, table [n*8] i64.  "pairs" mode: instead of goals, n x 6 i32 (a, b relative to the box, both open,
// within 4096 per axis); output [n] u8: vis(a, b) | tie bits << 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_path.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const bool pairs = !std::strcmp(argv[1], "pairs");
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t hdr[11];
    double d;
    if (!rd(f, hdr, sizeof hdr) || !rd(f, &d, 8)) return 2;
    const int32_t lo[3] = {hdr[3], hdr[4], hdr[5]};
    const int kind = hdr[6], n = hdr[7], L = hdr[8], max_moves = hdr[9], cap = hdr[10];
    const size_t nvox = (size_t)hdr[0] * hdr[1] * hdr[2];
    // exact-size heap blocks, so that the sanitizer sees any access beyond the field, the path or an output
    std::vector<uint8_t> parent(nvox);
    std::vector<int32_t> goals((size_t)n * (pairs ? 6 : 3)), way((size_t)n * cap * 3);
    if (!rd(f, parent.data(), nvox) || !rd(f, goals.data(), goals.size() * 4) || (!pairs && !rd(f, way.data(), way.size() * 4))) return 2;
    std::fclose(f);
    const MlmPathField F{parent.data(), {hdr[0], hdr[1], hdr[2]}, mlm_path_seed_code(kind)};
    FILE *g = std::fopen(argv[3], "wb");
    if (!g) return 2;
    if (pairs) {
        std::vector<uint8_t> out((size_t)n);
        for (int i = 0; i < n; ++i) {
            int ties = 0;
            const int *p = &goals[6 * (size_t)i];
            const bool v = mlm_path_vis(F, p, p + 3, &ties);
            if (v != mlm_path_vis(F, p, p + 3)) return 4;
            out[(size_t)i] = (uint8_t)((v ? 1 : 0) | ties << 1);
        }
        if (!wr(g, out.data(), out.size())) return 2;
        return std::fclose(g) ? 2 : 0;
    }
    const size_t len = (size_t)max_moves + 1;
    std::vector<int32_t> path(3 * len);
    MlmPathSerial X{path.data(), path.data() + len, path.data() + 2 * len};
    std::vector<int8_t> status((size_t)n);
    std::vector<double> length((size_t)n);
    std::vector<int64_t> table((size_t)n * MLM_PATH_WORDS);
    for (int i = 0; i < n; ++i) {
        const MlmPathOut o{&status[(size_t)i], cap ? &way[3 * (size_t)i * cap] : nullptr, &length[(size_t)i], &table[(size_t)i * MLM_PATH_WORDS]};
        const int st = mlm_path_goal(F, lo, &goals[3 * (size_t)i], L, max_moves, cap, d, X, o);
        // a single output at a time gives the same (null outputs are skipped)
        int64_t row[MLM_PATH_WORDS];
        double one = 0.0;
        const MlmPathOut t{nullptr, nullptr, nullptr, row}, l{nullptr, nullptr, &one, nullptr};
        if (mlm_path_goal(F, lo, &goals[3 * (size_t)i], L, max_moves, 0, d, X, t) != st ||
            std::memcmp(row, &table[(size_t)i * MLM_PATH_WORDS], sizeof row) || st != status[(size_t)i])
            return 4;
        mlm_path_goal(F, lo, &goals[3 * (size_t)i], L, max_moves, 0, d, X, l);
        if (std::memcmp(&one, &length[(size_t)i], 8)) return 4;
    }
    if (!wr(g, status.data(), status.size()) || !wr(g, way.data(), way.size() * 4) || !wr(g, length.data(), length.size() * 8) ||
        !wr(g, table.data(), table.size() * 8))
        return 2;
    return std::fclose(g) ? 2 : 0;
}
