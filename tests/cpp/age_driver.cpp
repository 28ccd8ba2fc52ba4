// age_driver.cpp — mlm_age_blocks on the CPU: mlmapping_amd/csrc/mlm_age.h and mlm_crop.h run in the device's phases (apply and block
// states; count, scan and rank of the empty selected blocks into the list; the move by (hole, filler) pairs; the tail reset) over a plain
// host model of the pool.  Built by tests/test_age_plan.py with -fsanitize=address,undefined and held byte for byte to tests/age_ref.py.
//
// in:  int64 [16]: map blocks, subbox_n, mode, flags, key_lo given, key_dims given, key_lo [3], key_dims [3], per_block wanted, 0...;
//      float [5]: log_odds_min, log_odds_max, occupied_sh, amount, forget; the map's keys / log_odds / occ / infl in slot order.
// out: int64 [16]: status, check code, summary [12], blocks afterwards, per_block rows; the check's text (64 bytes, zero padded);
//      per_block; the map's keys / log_odds / occ / infl.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_age.h"
#include "mlm_crop.h"

namespace {
constexpr int kWorkgroup = 256, kWave = 64;

template <class T> std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "age_driver: short input\n");
        exit(2);
    }
    return v;
}
template <class T> void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(3);
}
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = take<int64_t>(f, 16);
    const std::vector<float> par = take<float>(f, 5);
    const uint32_t nb = (uint32_t)head[0];
    const size_t C = (size_t)(head[1] * head[1] * head[1]);
    const int mode = (int)head[2], flags = (int)head[3];
    const int32_t key_lo[3] = {(int32_t)head[6], (int32_t)head[7], (int32_t)head[8]}, key_dims[3] = {(int32_t)head[9], (int32_t)head[10], (int32_t)head[11]};
    const bool want_rows = head[12] != 0;
    std::vector<int32_t> keys = take<int32_t>(f, 3 * (size_t)nb);
    std::vector<float> lo = take<float>(f, nb * C);
    std::vector<uint8_t> occ = take<uint8_t>(f, nb * C), infl = take<uint8_t>(f, nb * C);
    fclose(f);

    int64_t out[16] = {};
    int64_t *const sum = out + 2;
    char text[64] = {};
    std::vector<int32_t> per_block;
    uint32_t nb_after = nb;
    auto finish = [&](int status, int code) {
        out[0] = status, out[1] = code, out[14] = (int64_t)nb_after, out[15] = (int64_t)(per_block.size() / MLM_AGE_PB);
        if (code) snprintf(text, sizeof(text), "%s", mlm_age_check_text(code));
        FILE *g = fopen(argv[2], "wb");
        if (!g) return 3;
        put(g, out, 16);
        put(g, text, sizeof(text));
        put(g, per_block.data(), per_block.size());
        put(g, keys.data(), 3 * (size_t)nb_after), put(g, lo.data(), nb_after * C), put(g, occ.data(), nb_after * C), put(g, infl.data(), nb_after * C);
        fclose(g);
        return 0;
    };
    MlmAgeSel S{};
    const int bad = mlm_age_check(head[4] ? key_lo : nullptr, head[5] ? key_dims : nullptr, mode, par[3], par[4], flags, S);
    if (bad) return finish(-1, bad);
    if (nb == 0) return finish(0, 0);
    MlmAgeRule A{};
    A.R = MlmFuseRule{par[0], par[1], par[2], 0, 0};
    A.mode = mode, A.flags = flags, A.amount = par[3], A.forget = par[4];
    const bool dry = (flags & MLM_AGE_F_DRY) != 0, drop = (flags & MLM_AGE_F_DROP) != 0;

    // apply: the rule over the selected blocks, only what changed stored (nothing with DRY); per block its counts and its state
    std::vector<uint32_t> state(nb, MLM_AGE_B_UNSELECTED);
    if (want_rows) per_block.assign((size_t)nb * MLM_AGE_PB, -1);
    uint32_t n_empty = 0;
    sum[0] = nb;
    for (uint32_t s = 0; s < nb; ++s) {
        const bool selected = mlm_age_selects(S, keys[3 * (size_t)s], keys[3 * (size_t)s + 1], keys[3 * (size_t)s + 2]);
        uint32_t cnt[8] = {};
        bool full = false;
        if (selected) {
            for (size_t i = (size_t)s * C; i < (size_t)(s + 1) * C; ++i) {
                float L = lo[i];
                uint8_t o = occ[i], b = infl[i];
                const uint32_t ev = mlm_age_voxel(A, L, o, b);
                full = full || !mlm_age_voxel_empty(L, o, b);
                for (int k = 0; k < 8; ++k) cnt[k] += (ev >> k) & 1u;
                if (!dry) {
                    if (ev & MLM_AGE_E_LO) lo[i] = L;
                    if (ev & MLM_AGE_E_OCC) occ[i] = o;
                    if (ev & MLM_AGE_E_INFL_ST) infl[i] = b;
                }
            }
        }
        state[s] = !selected ? MLM_AGE_B_UNSELECTED : full ? MLM_AGE_B_KEPT : MLM_AGE_B_EMPTY;
        if (want_rows) {
            int32_t *pb = &per_block[(size_t)s * MLM_AGE_PB];
            pb[0] = (int32_t)cnt[0], pb[1] = (int32_t)cnt[2], pb[2] = (int32_t)(cnt[5] + cnt[6]), pb[3] = (int32_t)state[s];
        }
        n_empty += state[s] == MLM_AGE_B_EMPTY;
        sum[1] += selected;
        for (int k = 0; k < 8; ++k) sum[4 + k] += cnt[k];
    }
    sum[2] = drop ? n_empty : 0, sum[3] = (int64_t)nb - sum[2];
    if (!drop || dry) return finish(0, 0);

    // the empty selected blocks counted per chunk, the chunk counts scanned, every slot ranked round by round and wave by wave
    auto drop_of = [&](uint32_t s) { return state[s] == MLM_AGE_B_EMPTY; };
    const uint32_t chunks = (nb + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    std::vector<uint32_t> chunk_cnt(chunks, 0);
    for (uint32_t s = 0; s < nb; ++s) chunk_cnt[s / MLM_CROP_SLOTS_PER_CHUNK] += drop_of(s);
    uint32_t D = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t v = chunk_cnt[c];
        chunk_cnt[c] = D, D += v;
    }
    if (D != n_empty) return 4;
    const uint32_t K = nb - D;
    std::vector<uint32_t> list(nb, 0xFFFFFFFFu);
    uint32_t H = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        uint32_t base = chunk_cnt[c];
        for (uint32_t r = 0; r < MLM_CROP_SLOTS_PER_CHUNK; r += kWorkgroup) {
            uint32_t total = 0;
            for (int w = 0; w < kWorkgroup / kWave; ++w) {
                uint32_t lanes_before = 0;
                for (int l = 0; l < kWave; ++l) {
                    const uint64_t s = (uint64_t)c * MLM_CROP_SLOTS_PER_CHUNK + r + w * kWave + l;
                    if (s >= nb) continue;
                    const bool dr = drop_of((uint32_t)s);
                    const uint32_t d = base + total + lanes_before;
                    const uint32_t at = mlm_crop_list_pos((uint32_t)s, d, dr, D);
                    if (at >= nb || list[at] != 0xFFFFFFFFu) return 4; // (the list is a permutation)
                    list[at] = (uint32_t)s;
                    if ((uint32_t)s == K) H = d;
                    lanes_before += dr ? 1u : 0u;
                }
                total += lanes_before;
            }
            base += total;
        }
    }
    if (D) {
        // the move, the last pair first (the rule has no order among the pairs), then the free tail back at alloc_pool's values
        for (uint32_t j = H; j-- > 0;) {
            const size_t dst = list[mlm_crop_hole_at(j)], src = list[mlm_crop_filler_at(j, D, K, H)];
            if (dst >= K || src < K || src >= nb) return 5;
            memcpy(&keys[3 * dst], &keys[3 * src], 12);
            memcpy(&lo[dst * C], &lo[src * C], C * 4), memcpy(&occ[dst * C], &occ[src * C], C), memcpy(&infl[dst * C], &infl[src * C], C);
        }
        for (size_t v = (size_t)K * C; v < (size_t)nb * C; ++v) lo[v] = 0.0f, occ[v] = 'u', infl[v] = 'u';
        nb_after = K;
    }
    return finish(0, 0);
}
