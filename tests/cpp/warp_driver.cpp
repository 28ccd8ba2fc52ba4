// warp_driver.cpp — mlm_warp_blocks on the CPU (tests/test_warp_plan.py): the rule of mlmapping_amd/csrc/mlm_warp.h run in the order
// of the device phases — argument check, candidates of every source block into a set, sort, the gather counted per candidate by 64
// lanes that each keep the source block of their previous voxel, exclusive prefix of the emitted flags, capacity check, the gather
// again into the rows — built with -fsanitize=address,undefined and compared byte for byte with tests/warp_ref.py.
//
//   warp_driver IN OUT
// IN:  int64 [16]: nb, n, flags, cap, have_T, have_lo, have_dims, key_lo[3], key_dims[3], want_out, 0, 0; double [13]: d_sub, T[12];
//      keys int32 [nb][3], log_odds float [nb][C], occ, infl uint8 [nb][C], collapsed uint8 [nb]
// OUT: int64 [10]: status (0, -1 invalid, -3 capacity), the check's code, summary[8]; then the written rows: keys, log_odds, occ, infl
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "mlm_warp.h"

namespace {
struct Map {
    int n, cells;
    std::unordered_map<unsigned long long, int> table;
    std::vector<float> lo;
    std::vector<uint8_t> occ, infl, col;
};

// mlm_warp.h's callable over the host map
struct Src {
    const Map &M;
    int slot;
    bool whole;
    bool operator()(const int g[3], const int c[3], bool new_block, float &lo, uint8_t &occ, uint8_t &infl) {
        if (new_block) {
            slot = -1;
            if (mlm_warp_key_ok(g)) {
                const auto it = M.table.find(mlm_warp_pack(g));
                if (it != M.table.end()) slot = it->second;
            }
            whole = slot >= 0 && M.col[(size_t)slot] != 0;
        }
        if (slot < 0) return false;
        const size_t at = (size_t)slot * M.cells + (whole ? (size_t)0 : (size_t)((c[2] * M.n + c[1]) * M.n + c[0]));
        lo = M.lo[at];
        occ = M.occ[at];
        infl = whole ? (uint8_t)'u' : M.infl[at];
        return true;
    }
};

template <class T> void read(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "warp_driver: short input\n");
        exit(2);
    }
}
template <class T> void write(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(2);
}
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int64_t hd[16];
    double dv[13];
    read(fi, hd, 16);
    read(fi, dv, 13);
    const int nb = (int)hd[0], n = (int)hd[1], flags = (int)hd[2];
    const long long cap = hd[3];
    const int32_t key_lo[3] = {(int32_t)hd[7], (int32_t)hd[8], (int32_t)hd[9]}, key_dims[3] = {(int32_t)hd[10], (int32_t)hd[11], (int32_t)hd[12]};
    const bool want_out = hd[13] != 0;
    Map M{n, n * n * n, {}, {}, {}, {}, {}};
    const size_t C = (size_t)M.cells;
    std::vector<int32_t> keys((size_t)nb * 3);
    M.lo.resize((size_t)nb * C), M.occ.resize((size_t)nb * C), M.infl.resize((size_t)nb * C), M.col.resize((size_t)nb);
    read(fi, keys.data(), keys.size());
    read(fi, M.lo.data(), M.lo.size());
    read(fi, M.occ.data(), M.occ.size());
    read(fi, M.infl.data(), M.infl.size());
    read(fi, M.col.data(), M.col.size());
    fclose(fi);

    int64_t head[10] = {};
    std::vector<int32_t> o_keys;
    std::vector<float> o_lo;
    std::vector<uint8_t> o_occ, o_infl;
    MlmWarpPlan W{};
    const int bad = mlm_warp_check(hd[4] ? dv + 1 : nullptr, hd[5] ? key_lo : nullptr, hd[6] ? key_dims : nullptr, flags, cap, W);
    head[1] = bad;
    if (bad) {
        if (!mlm_warp_check_text(bad)[0]) return 3;
        head[0] = -1;
    } else {
        const MlmWarpGeom G{dv[0], dv[0] * n, dv[0] * 0.5, n};
        for (int s = 0; s < nb; ++s) {
            const int g[3] = {keys[3 * (size_t)s], keys[3 * (size_t)s + 1], keys[3 * (size_t)s + 2]};
            M.table[mlm_warp_pack(g)] = s;
        }
        // candidates: a set, then sorted — the emission order
        const unsigned long long most = (unsigned long long)nb * mlm_warp_span(W, G, 0) * mlm_warp_span(W, G, 1) * mlm_warp_span(W, G, 2);
        std::unordered_set<unsigned long long> set;
        for (int s = 0; s < nb; ++s) {
            const int g[3] = {keys[3 * (size_t)s], keys[3 * (size_t)s + 1], keys[3 * (size_t)s + 2]};
            int32_t klo[3], khi[3];
            if (!mlm_warp_candidates(W, G, g, klo, khi)) continue;
            unsigned long long mine = 0;
            for (int x = klo[0]; x <= khi[0]; ++x)
                for (int y = klo[1]; y <= khi[1]; ++y)
                    for (int z = klo[2]; z <= khi[2]; ++z) {
                        const int k[3] = {x, y, z};
                        if (!mlm_warp_key_ok(k) || !mlm_warp_in_box(W, k)) return 4; // (the rule names keys of the box only)
                        set.insert(mlm_warp_pack(k));
                        ++mine;
                    }
            if (mine > (unsigned long long)mlm_warp_span(W, G, 0) * mlm_warp_span(W, G, 1) * mlm_warp_span(W, G, 2)) return 5; // (the bound the set is sized by)
        }
        if (set.size() > most) return 5;
        std::vector<unsigned long long> cand(set.begin(), set.end());
        std::sort(cand.begin(), cand.end());
        const size_t NC = cand.size();
        // count: 64 lanes over the cells of a candidate, x fastest
        auto cell_div = [n](uint32_t i) { return i / (uint32_t)n; };
        std::vector<uint32_t> cnt(NC * 4, 0);
        for (size_t i = 0; i < NC; ++i) {
            int g[3];
            mlm_warp_unpack(cand[i], g);
            for (int lane = 0; lane < 64; ++lane) {
                MlmScoreBlock B{};
                Src src{M, -1, false};
                for (uint32_t ci = (uint32_t)lane; ci < (uint32_t)C; ci += 64) {
                    int c[3];
                    mlm_warp_cell(ci, n, cell_div, c);
                    float lo;
                    uint8_t occ, infl;
                    if (!mlm_warp_voxel(W.T, W.seen != 0, G, g, c, src, B, lo, occ, infl)) {
                        if (lo != 0.0f || occ != 'u' || infl != 'u') return 6;
                        continue;
                    }
                    cnt[4 * i] += 1, cnt[4 * i + 1] += occ == 'o', cnt[4 * i + 2] += occ == 'f', cnt[4 * i + 3] += infl == 'o';
                }
            }
        }
        // scan: rank of every emitted candidate
        std::vector<uint32_t> elist;
        for (size_t i = 0; i < NC; ++i) {
            if (cnt[4 * i]) elist.push_back((uint32_t)i);
            for (int k = 0; k < 4; ++k) head[6 + k] += cnt[4 * i + k];
        }
        const size_t E = elist.size();
        head[2] = nb, head[3] = (int64_t)NC, head[4] = (int64_t)E;
        if (want_out && (unsigned long long)cap < E) {
            head[0] = -3;
        } else if (want_out && !(flags & MLM_WARP_F_DRY)) {
            o_keys.resize(E * 3), o_lo.resize(E * C), o_occ.resize(E * C), o_infl.resize(E * C);
            for (size_t r = 0; r < E; ++r) {
                int g[3];
                mlm_warp_unpack(cand[elist[r]], g);
                for (int a = 0; a < 3; ++a) o_keys[3 * r + a] = g[a];
                for (int lane = 0; lane < 64; ++lane) {
                    MlmScoreBlock B{};
                    Src src{M, -1, false};
                    for (uint32_t ci = (uint32_t)lane; ci < (uint32_t)C; ci += 64) {
                        int c[3];
                        mlm_warp_cell(ci, n, cell_div, c);
                        mlm_warp_voxel(W.T, W.seen != 0, G, g, c, src, B, o_lo[r * C + ci], o_occ[r * C + ci], o_infl[r * C + ci]);
                    }
                }
            }
            head[5] = (int64_t)E;
        }
    }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    write(fo, head, 10);
    write(fo, o_keys.data(), o_keys.size());
    write(fo, o_lo.data(), o_lo.size());
    write(fo, o_occ.data(), o_occ.size());
    write(fo, o_infl.data(), o_infl.size());
    fclose(fo);
    return 0;
}
