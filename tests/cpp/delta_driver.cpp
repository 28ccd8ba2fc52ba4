// delta_driver.cpp — mlm_delta_blocks on the CPU: mlmapping_amd/csrc/mlm_delta.h run in the device's phases (digest and packed key per
// slot; the sort of (packed key, slot); the join by binary search both ways with the check of the previous table; the ranks of the
// emitted blocks and of the gone rows; the cap check; the emission) over a plain host model of the pool.  Built by
// tests/test_delta_plan.py with -fsanitize=address,undefined and held byte for byte to tests/delta_ref.py.
//
// in:  int64 [20]: map blocks, subbox_n, flags, key_lo given, key_dims given, key_lo [3], key_dims [3], n_prev, previous table given,
//      cap_table, cap, cap_gone, outputs given (1 table | 2 blocks | 4 gone keys), 0...; the map's keys / log_odds / occ / infl /
//      released flags in slot order; prev_keys [n_prev][3]; prev_digest [n_prev][2].
// out: int64 [16]: status, check code, summary [12], 0, 0; the check's text (64 bytes, zero padded); then the outputs at their full caps,
//      every byte 7 where nothing was written: cur_keys, cur_digest, keys, log_odds, occ, infl, kind, gone_keys.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "mlm_delta.h"

namespace {
template <class T> std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "delta_driver: short input\n");
        exit(2);
    }
    return v;
}
template <class T> void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(3);
}
template <class T> std::vector<T> sevens(size_t n) {
    std::vector<T> v(n);
    if (n) memset(v.data(), 7, n * sizeof(T));
    return v;
}
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = take<int64_t>(f, 20);
    const uint32_t nb = (uint32_t)head[0];
    const size_t C = (size_t)(head[1] * head[1] * head[1]);
    const int flags = (int)head[2];
    const int32_t key_lo[3] = {(int32_t)head[5], (int32_t)head[6], (int32_t)head[7]}, key_dims[3] = {(int32_t)head[8], (int32_t)head[9], (int32_t)head[10]};
    const long long n_prev = head[11], cap_table = head[13], cap = head[14], cap_gone = head[15];
    const bool table_out = head[16] & 1, block_out = head[16] & 2, gone_out = head[16] & 4;
    const std::vector<int32_t> keys = take<int32_t>(f, 3 * (size_t)nb);
    const std::vector<float> lo = take<float>(f, nb * C);
    const std::vector<uint8_t> occ = take<uint8_t>(f, nb * C), infl = take<uint8_t>(f, nb * C), released = take<uint8_t>(f, nb);
    const size_t np_read = n_prev > 0 && head[12] ? (size_t)n_prev : 0;
    const std::vector<int32_t> prev_keys = take<int32_t>(f, 3 * np_read);
    const std::vector<uint64_t> prev_dg = take<uint64_t>(f, 2 * np_read);
    fclose(f);

    int64_t out[16] = {};
    int64_t *const sum = out + 2;
    char text[64] = {};
    const size_t ct = cap_table > 0 ? (size_t)cap_table : 0, cb = cap > 0 ? (size_t)cap : 0, cg = cap_gone > 0 ? (size_t)cap_gone : 0;
    std::vector<int32_t> cur_keys = sevens<int32_t>(3 * ct), e_keys = sevens<int32_t>(3 * cb), gone_keys = sevens<int32_t>(3 * cg);
    std::vector<uint64_t> cur_dg = sevens<uint64_t>(2 * ct);
    std::vector<float> e_lo = sevens<float>(cb * C);
    std::vector<uint8_t> e_occ = sevens<uint8_t>(cb * C), e_infl = sevens<uint8_t>(cb * C), e_kind = sevens<uint8_t>(cb);
    auto finish = [&](int status, int code, bool with_summary) {
        out[0] = status, out[1] = code;
        if (!with_summary) memset(sum, 0, MLM_DELTA_SUMS * sizeof(int64_t));
        if (code) snprintf(text, sizeof(text), "%s", mlm_delta_check_text(code));
        FILE *g = fopen(argv[2], "wb");
        if (!g) return 3;
        put(g, out, 16);
        put(g, text, sizeof(text));
        put(g, cur_keys.data(), cur_keys.size()), put(g, cur_dg.data(), cur_dg.size()), put(g, e_keys.data(), e_keys.size()), put(g, e_lo.data(), e_lo.size());
        put(g, e_occ.data(), e_occ.size()), put(g, e_infl.data(), e_infl.size()), put(g, e_kind.data(), e_kind.size()), put(g, gone_keys.data(), gone_keys.size());
        fclose(g);
        return 0;
    };
    MlmAgeSel S{};
    const int bad = mlm_delta_check(head[3] ? key_lo : nullptr, head[4] ? key_dims : nullptr, n_prev, head[12] ? (const void *)&head : nullptr,
                                    head[12] ? (const void *)&head : nullptr, flags, cap_table, cap, cap_gone, S);
    if (bad) return finish(-1, bad, false);
    const uint32_t np = (uint32_t)n_prev;
    const bool no_infl = (flags & MLM_DELTA_F_NO_INFL) != 0;
    sum[0] = nb, sum[2] = np;
    if (nb == 0 && np == 0) return finish(0, 0, true);

    // digest: per slot the packed key (none where not selected), the two sums over the view, the empty flag
    std::vector<std::pair<unsigned long long, uint32_t>> order(nb);
    std::vector<unsigned long long> dg(2 * (size_t)nb, 0);
    int64_t n_sel = 0, n_empty = 0;
    for (uint32_t s = 0; s < nb; ++s) {
        const int32_t *k = &keys[3 * (size_t)s];
        order[s] = {MLM_WARP_EMPTY, s};
        if (!mlm_age_selects(S, k[0], k[1], k[2])) continue;
        order[s].first = mlm_delta_pack3(k);
        unsigned long long d0 = 0, d1 = 0;
        bool full = false;
        for (size_t c = 0; c < C; ++c) {
            const size_t at = (size_t)s * C + (released[s] ? 0 : c);
            const uint8_t fl = released[s] ? (uint8_t)'u' : infl[at];
            full = full || !mlm_age_voxel_empty(lo[at], occ[at], fl);
            mlm_delta_cell((unsigned long long)(c + 1) * MLM_DELTA_GOLD, mlm_delta_word(mlm_fuse_bits(lo[at]), occ[at], no_infl ? (uint8_t)'u' : fl), d0, d1);
        }
        dg[2 * (size_t)s] = d0, dg[2 * (size_t)s + 1] = d1;
        n_sel += 1, n_empty += !full;
    }
    std::sort(order.begin(), order.end());

    // join: every sorted live block against the previous table, every previous row against its neighbour and the live keys
    auto prev_at = [&](uint32_t m) { return mlm_delta_pack3(&prev_keys[3 * (size_t)m]); };
    auto live_at = [&](uint32_t m) { return order[m].first; };
    std::vector<uint32_t> kind(nb, MLM_DELTA_K_NONE), pstate(np, MLM_DELTA_P_OUTSIDE);
    int64_t cnt_kind[3] = {}, inbox = 0, gone = 0;
    bool bad_range = false, bad_order = false;
    for (uint32_t i = 0; i < nb; ++i) {
        const unsigned long long key = order[i].first;
        if (key == MLM_WARP_EMPTY) continue;
        const uint32_t j = mlm_delta_lower_bound(prev_at, np, key);
        const bool found = j < np && prev_at(j) == key;
        const size_t s = order[i].second;
        const bool same = found && prev_dg[2 * (size_t)j] == dg[2 * s] && prev_dg[2 * (size_t)j + 1] == dg[2 * s + 1];
        kind[i] = (uint32_t)mlm_delta_kind(found, same);
        cnt_kind[kind[i]] += 1;
    }
    for (uint32_t j = 0; j < np; ++j) {
        const int32_t *k = &prev_keys[3 * (size_t)j];
        const unsigned long long key = mlm_delta_pack3(k);
        if (!mlm_delta_key_ok(k)) bad_range = true;
        if (j + 1 < np && key >= prev_at(j + 1)) bad_order = true;
        if (!mlm_age_selects(S, k[0], k[1], k[2])) continue;
        const uint32_t i = mlm_delta_lower_bound(live_at, nb, key);
        const bool held = i < nb && live_at(i) == key;
        pstate[j] = held ? MLM_DELTA_P_HELD : MLM_DELTA_P_GONE;
        inbox += 1, gone += !held;
    }
    if (bad_range || bad_order) return finish(-1, bad_range ? 7 : 8, false);

    // ranks: the emitted sorted positions and the gone rows, ascending
    std::vector<uint32_t> elist, glist;
    for (uint32_t i = 0; i < nb; ++i)
        if (mlm_delta_emits((int)kind[i])) elist.push_back(i);
    for (uint32_t j = 0; j < np; ++j)
        if (pstate[j] == MLM_DELTA_P_GONE) glist.push_back(j);
    const size_t E = elist.size(), G = glist.size();
    if ((int64_t)E != cnt_kind[MLM_DELTA_K_CHANGED] + cnt_kind[MLM_DELTA_K_NEW] || (int64_t)G != gone) return 4;
    sum[1] = n_sel, sum[3] = inbox, sum[4] = cnt_kind[0], sum[5] = cnt_kind[1], sum[6] = cnt_kind[2], sum[7] = gone, sum[11] = n_empty;
    if ((table_out && cap_table < n_sel) || (block_out && (size_t)cap < E) || (gone_out && (size_t)cap_gone < G)) return finish(-3, 0, true);
    if (flags & MLM_DELTA_F_DRY) return finish(0, 0, true);

    // emission: the table (the first S sorted positions), the gone keys, the planes of the view
    if (table_out) {
        for (uint32_t i = 0; i < (uint32_t)n_sel; ++i) {
            int g[3];
            mlm_warp_unpack(order[i].first, g);
            for (int a = 0; a < 3; ++a) cur_keys[3 * (size_t)i + a] = g[a];
            cur_dg[2 * (size_t)i] = dg[2 * (size_t)order[i].second], cur_dg[2 * (size_t)i + 1] = dg[2 * (size_t)order[i].second + 1];
        }
        sum[9] = n_sel;
    }
    if (gone_out) {
        for (size_t r = 0; r < G; ++r) memcpy(&gone_keys[3 * r], &prev_keys[3 * (size_t)glist[r]], 12);
        sum[10] = (int64_t)G;
    }
    if (block_out && E) {
        for (size_t r = 0; r < E; ++r) {
            const size_t s = order[elist[r]].second;
            memcpy(&e_keys[3 * r], &keys[3 * s], 12);
            e_kind[r] = (uint8_t)kind[elist[r]];
            for (size_t c = 0; c < C; ++c) {
                const size_t at = s * C + (released[s] ? 0 : c);
                e_lo[r * C + c] = lo[at], e_occ[r * C + c] = occ[at];
                e_infl[r * C + c] = released[s] || no_infl ? (uint8_t)'u' : infl[at];
            }
        }
        sum[8] = (int64_t)E;
    }
    return finish(0, 0, true);
}
