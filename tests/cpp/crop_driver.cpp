// CPU driver of mlm_crop.h (tests/test_crop_plan.py): the header's argument check, predicate, list positions, pair rule and shrink rule,
// executed over plain arrays the way the device phases of mlm_kernels_crop.h run them — flags counted per chunk, the chunk counts
// scanned, every slot ranked inside its chunk round by round and wave by wave, the page-out, the move by (hole, filler) pairs in a
// shuffled order, the tail reset.
//   crop_driver args  (has_box lo3 dims3 flags cap)...   -> a line per case: the check's code
//   crop_driver shrink (c0 capacity K)...                -> a line per case: the target
//   crop_driver run in.bin out.bin
//     in:  int64 {nb, cells, lo3, dims3, flags, cap, want_out, seed}, int32 keys [nb*3], float log_odds [nb*cells], u8 occ, u8 infl, u8 collapsed [nb]
//     out: int64 {status, nb, K, D, written, H}, then the pool after the call (same arrays, nb slots), then the output rows (D of each)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_crop.h"

namespace {
constexpr int kWorkgroup = 256, kWave = 64;

template <class T> void put(FILE *f, const std::vector<T> &v, size_t n) {
    if (n && fwrite(v.data(), sizeof(T), n, f) != n) exit(3);
}
template <class T> void get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(3);
}

int run(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 2;
    int64_t hd[12];
    if (fread(hd, sizeof(int64_t), 12, f) != 12) return 3;
    const uint32_t nb = (uint32_t)hd[0];
    const size_t C = (size_t)hd[1];
    const int32_t lo[3] = {(int32_t)hd[2], (int32_t)hd[3], (int32_t)hd[4]}, dims[3] = {(int32_t)hd[5], (int32_t)hd[6], (int32_t)hd[7]};
    const int flags = (int)hd[8];
    const long long cap = hd[9];
    const bool want_out = hd[10] != 0;
    uint64_t rng = (uint64_t)hd[11] * 2862933555777941757ull + 3037000493ull;
    std::vector<int32_t> keys;
    std::vector<float> lod;
    std::vector<uint8_t> occ, infl, col;
    get(f, keys, (size_t)nb * 3), get(f, lod, nb * C), get(f, occ, nb * C), get(f, infl, nb * C), get(f, col, nb);
    fclose(f);

    int64_t res[6] = {0, nb, nb, 0, 0, 0};
    std::vector<int32_t> o_keys;
    std::vector<float> o_lod;
    std::vector<uint8_t> o_occ, o_infl, o_col;
    MlmCropBox B{};
    const int bad = mlm_crop_check(lo, dims, flags, cap, B);
    if (bad) {
        res[0] = -1;
    } else {
        auto drop_of = [&](uint32_t s) { return mlm_crop_drops(B, keys[3 * (size_t)s], keys[3 * (size_t)s + 1], keys[3 * (size_t)s + 2]); };
        // phase 1: dropped slots per chunk
        const uint32_t chunks = (nb + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
        std::vector<uint32_t> chunk_cnt(chunks, 0);
        for (uint32_t c = 0; c < chunks; ++c)
            for (uint64_t s = (uint64_t)c * MLM_CROP_SLOTS_PER_CHUNK; s < (uint64_t)(c + 1) * MLM_CROP_SLOTS_PER_CHUNK; ++s)
                if (s < nb && drop_of((uint32_t)s)) chunk_cnt[c]++;
        // phase 2: exclusive scan of the chunk counts in place; the total is D
        uint32_t D = 0;
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t v = chunk_cnt[c];
            chunk_cnt[c] = D;
            D += v;
        }
        const uint32_t K = nb - D;
        // phase 3: every slot's d(s) from its chunk's base, the rounds before it, the waves before it and the lanes before it
        std::vector<uint32_t> list(nb, 0xFFFFFFFFu);
        uint32_t H = 0;
        for (uint32_t c = 0; c < chunks; ++c) {
            uint32_t base = chunk_cnt[c];
            for (uint32_t r = 0; r < MLM_CROP_SLOTS_PER_CHUNK; r += kWorkgroup) {
                uint32_t wave_cnt[kWorkgroup / kWave] = {};
                for (int t = 0; t < kWorkgroup; ++t) {
                    const uint64_t s = (uint64_t)c * MLM_CROP_SLOTS_PER_CHUNK + r + t;
                    if (s < nb && drop_of((uint32_t)s)) wave_cnt[t / kWave]++;
                }
                uint32_t total = 0;
                for (int w = 0; w < kWorkgroup / kWave; ++w) {
                    uint32_t lanes_before = 0;
                    for (int l = 0; l < kWave; ++l) {
                        const uint64_t s = (uint64_t)c * MLM_CROP_SLOTS_PER_CHUNK + r + w * kWave + l;
                        if (s >= nb) continue;
                        const bool drop = drop_of((uint32_t)s);
                        const uint32_t d = base + total + lanes_before;
                        const uint32_t at = mlm_crop_list_pos((uint32_t)s, d, drop, D);
                        if (at >= nb || list[at] != 0xFFFFFFFFu) return 4; // (the list is a permutation)
                        list[at] = (uint32_t)s;
                        if ((uint32_t)s == K) H = d;
                        lanes_before += drop ? 1u : 0u;
                    }
                    total += wave_cnt[w];
                }
                base += total;
            }
        }
        res[2] = K, res[3] = D, res[5] = H;
        if (want_out && cap < (long long)D) {
            res[0] = -3;
        } else if (!(flags & MLM_CROP_F_DRY) && D) {
            if (want_out) { // the page-out, before the move
                o_keys.resize((size_t)D * 3), o_lod.resize(D * C), o_occ.resize(D * C), o_infl.resize(D * C), o_col.resize(D);
                for (uint32_t r = 0; r < D; ++r) {
                    const size_t s = list[r];
                    memcpy(&o_keys[3 * (size_t)r], &keys[3 * s], 12);
                    memcpy(&o_lod[r * C], &lod[s * C], C * 4), memcpy(&o_occ[r * C], &occ[s * C], C), memcpy(&o_infl[r * C], &infl[s * C], C);
                    o_col[r] = col[s];
                }
                res[4] = D;
            }
            // the move, pair by pair in an arbitrary order (the rule has no order among the pairs)
            std::vector<uint32_t> pairs(H);
            for (uint32_t j = 0; j < H; ++j) pairs[j] = j;
            for (uint32_t j = H; j > 1; --j) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(pairs[j - 1], pairs[(size_t)((rng >> 33) % j)]);
            }
            for (uint32_t j : pairs) {
                const size_t dst = list[mlm_crop_hole_at(j)], src = list[mlm_crop_filler_at(j, D, K, H)];
                if (dst >= K || src < K || src >= nb) return 5;
                memcpy(&keys[3 * dst], &keys[3 * src], 12);
                memcpy(&lod[dst * C], &lod[src * C], C * 4), memcpy(&occ[dst * C], &occ[src * C], C), memcpy(&infl[dst * C], &infl[src * C], C);
                col[dst] = col[src];
            }
            // the free tail [K, nb) back at alloc_pool's values
            for (size_t v = (size_t)K * C; v < (size_t)nb * C; ++v) lod[v] = 0.0f, occ[v] = 'u', infl[v] = 'u';
            for (size_t s = K; s < nb; ++s) col[s] = 0;
        }
    }
    f = fopen(out_path, "wb");
    if (!f) return 2;
    if (fwrite(res, sizeof(int64_t), 6, f) != 6) return 3;
    put(f, keys, (size_t)nb * 3), put(f, lod, nb * C), put(f, occ, nb * C), put(f, infl, nb * C), put(f, col, nb);
    put(f, o_keys, o_keys.size()), put(f, o_lod, o_lod.size()), put(f, o_occ, o_occ.size()), put(f, o_infl, o_infl.size()), put(f, o_col, o_col.size());
    fclose(f);
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "args")) {
        for (int i = 2; i + 8 < argc; i += 9) {
            int32_t lo[3], dims[3];
            for (int a = 0; a < 3; ++a) lo[a] = (int32_t)atoll(argv[i + 1 + a]), dims[a] = (int32_t)atoll(argv[i + 4 + a]);
            const bool has = atoll(argv[i]) != 0;
            MlmCropBox B{};
            const int bad = mlm_crop_check(has ? lo : nullptr, has ? dims : nullptr, (int)atoll(argv[i + 7]), atoll(argv[i + 8]), B);
            printf("%d %s\n", bad, bad ? mlm_crop_check_text(bad) : "ok");
        }
        return 0;
    }
    if (!strcmp(argv[1], "shrink")) {
        for (int i = 2; i + 2 < argc; i += 3) printf("%lld\n", mlm_crop_shrink_target(atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2])));
        return 0;
    }
    if (!strcmp(argv[1], "widths")) {
        for (int i = 2; i < argc; ++i) printf("%d %d\n", mlm_crop_float_width(atoi(argv[i])), mlm_crop_byte_width(atoi(argv[i])));
        return 0;
    }
    if (!strcmp(argv[1], "run") && argc == 4) return run(argv[2], argv[3]);
    return 2;
}
