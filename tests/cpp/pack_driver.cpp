// pack_driver.cpp — mlm_pack_blocks / mlm_unpack_blocks on the CPU: mlmapping_amd/csrc/mlm_pack.h run in the device's phases (pack:
// pass 1 per row — codes, presence, counts, size —, the prefix, the capacity check, pass 2 with its guards; unpack: the header, the
// validator per block with the verdict of its successor's offset, the smallest (block, check), the cap check, the writer) over plain
// host arrays.  Built by tests/test_pack_plan.py with -fsanitize=address,undefined and held byte for byte to tests/pack_ref.py.  The
// stream of an unpack lives in a heap block of exactly `bytes` bytes: a read beyond it ends the program.
//
// in:  int64 [24]: mode (0 pack, 1 unpack), subbox_n, then
//        pack:   n, flags, bits of lo_min, bits of lo_max, cap_bytes, stream given, keys given, log_odds given, occ given, infl given,
//                key_lo given, key_dims given, key_lo [3], key_dims [3], the stream is misaligned device memory, 0...;
//                keys [n][3], log_odds, occ, infl [n][C] (each only if given and n > 0), released [n]
//        unpack: bytes, flags, cap, outputs given (1 keys | 2 log_odds | 4 occ | 8 infl), stream given, misaligned, 0...; the stream
// out: int64 [12]: status, check code, row / block (-1: none), summary [8], 0; the check's text (96 bytes, zero padded); then
//        pack:   the stream at its cap, every byte 7 where nothing was written
//        unpack: keys, log_odds, occ, infl at their cap, every byte 7 where nothing was written
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mlm_pack.h"

namespace {
template <class T> std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "pack_driver: short input\n");
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

int64_t out[12] = {};
char text[96] = {};

int finish(const char *path, int status, int code, long long where, const char *msg, bool with_summary, std::initializer_list<std::pair<const void *, size_t>> bufs) {
    out[0] = status, out[1] = code, out[2] = where;
    if (!with_summary) memset(out + 3, 0, MLM_PACK_SUMS * sizeof(int64_t));
    if (msg) snprintf(text, sizeof(text), "%s", msg);
    FILE *g = fopen(path, "wb");
    if (!g) return 3;
    put(g, out, 12);
    put(g, text, sizeof(text));
    for (const auto &b : bufs) put(g, (const uint8_t *)b.first, b.second);
    fclose(g);
    return 0;
}

int run_pack(FILE *f, const std::vector<int64_t> &head, const char *path) {
    const uint32_t subbox_n = (uint32_t)head[1], C = subbox_n * subbox_n * subbox_n, W = mlm_pack_words(C);
    const long long n_arg = head[2];
    const int flags = (int)head[3];
    const uint32_t min_bits = (uint32_t)head[4], max_bits = (uint32_t)head[5];
    const size_t cap_bytes = (size_t)head[6];
    const bool stream_given = head[7], keys_given = head[8], lo_given = head[9], occ_given = head[10], infl_given = head[11];
    const int32_t key_lo[3] = {(int32_t)head[14], (int32_t)head[15], (int32_t)head[16]}, key_dims[3] = {(int32_t)head[17], (int32_t)head[18], (int32_t)head[19]};
    const size_t n = keys_given && n_arg > 0 ? (size_t)n_arg : 0; // (no keys: the live map, which this driver holds empty)
    const std::vector<int32_t> keys = take<int32_t>(f, keys_given ? 3 * n : 0);
    const std::vector<uint32_t> lo = take<uint32_t>(f, lo_given ? n * C : 0);
    const std::vector<uint8_t> occ = take<uint8_t>(f, occ_given ? n * C : 0), infl = take<uint8_t>(f, infl_given ? n * C : 0), released = take<uint8_t>(f, n);
    std::vector<uint8_t> stream = sevens<uint8_t>(cap_bytes);
    int64_t *const sum = out + 3;
    auto done = [&](int status, int code, long long where, const char *msg, bool with_summary) {
        return finish(path, status, code, where, msg, with_summary, {{stream.data(), stream.size()}});
    };
    MlmAgeSel S{};
    const int bad = mlm_pack_check(head[12] ? key_lo : nullptr, head[13] ? key_dims : nullptr, n_arg, keys_given ? (const void *)&head : nullptr,
                                   lo_given ? (const void *)&head : nullptr, occ_given ? (const void *)&head : nullptr, flags, head[20] != 0, head[20] ? 4ull : 0ull, S);
    if (bad) return done(-1, bad, -1, mlm_pack_check_text(bad), false);
    const bool no_infl = (flags & MLM_PACK_F_NO_INFL) != 0;

    // the view of a cell, as mlm_kernels_pack.h's mlm_pack_cell reads it
    auto cell = [&](size_t r, uint32_t c, uint32_t &bits, uint32_t &co, uint32_t &ci, uint32_t &cv) {
        bits = co = ci = cv = 0u;
        if (c >= C) return true;
        const size_t at = r * C + (released[r] ? 0 : c);
        bits = lo[at];
        co = mlm_pack_class_code(occ[at]);
        ci = infl_given && !no_infl && !released[r] ? mlm_pack_class_code(infl[at]) : 0u;
        cv = mlm_pack_val_code(bits, min_bits, max_bits);
        const bool ok = co != 3u && ci != 3u;
        if (co == 3u) co = 0u;
        if (ci == 3u) ci = 0u;
        return ok;
    };
    // a step's ballots: the six plane words and the literal mask of cells 64 j .. 64 j + 63
    auto step = [&](size_t r, uint32_t j, unsigned long long b[6], uint32_t bits[64], unsigned long long &m_min, unsigned long long &m_max) {
        bool ok = true;
        for (int k = 0; k < 6; ++k) b[k] = 0ull;
        m_min = m_max = 0ull;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t co, ci, cv;
            ok = cell(r, 64u * j + lane, bits[lane], co, ci, cv) && ok;
            const uint32_t code[6] = {co & 1u, co >> 1, ci & 1u, ci >> 1, cv & 1u, cv >> 1};
            for (int k = 0; k < 6; ++k) b[k] |= (unsigned long long)code[k] << lane;
            m_min |= (unsigned long long)(cv == 1u) << lane, m_max |= (unsigned long long)(cv == 2u) << lane;
        }
        return ok;
    };

    // pass 1
    std::vector<MlmPackRow> rows(n);
    for (size_t r = 0; r < n; ++r) {
        MlmPackRow R{};
        bool okr = true;
        for (uint32_t j = 0; j < W; ++j) {
            unsigned long long b[6], m_min, m_max;
            uint32_t bits[64];
            okr = step(r, j, b, bits, m_min, m_max) && okr;
            for (int k = 0; k < 6; ++k) R.presence |= b[k] ? 1u << k : 0u;
            R.n_lit += (uint32_t)__builtin_popcountll(b[4] & b[5]), R.n_min += (uint32_t)__builtin_popcountll(m_min), R.n_max += (uint32_t)__builtin_popcountll(m_max);
        }
        R.units = (uint32_t)(mlm_pack_record_bytes(W, R.presence, R.n_lit) / 8ull), R.err = okr ? 0u : 1u, R.pad0 = 1u;
        rows[r] = R;
    }
    // the prefix and the totals
    std::vector<unsigned long long> off(n);
    unsigned long long units = 0, blank = 0, lits = 0, mins = 0, maxs = 0, key = ~0ull;
    for (size_t r = 0; r < n; ++r) {
        off[r] = units;
        units += rows[r].units, blank += rows[r].units == 1u, lits += rows[r].n_lit, mins += rows[r].n_min, maxs += rows[r].n_max;
        const unsigned long long k = mlm_pack_verdict_key((uint32_t)r, rows[r].err, 0u);
        if (k < key) key = k;
    }
    if (key != ~0ull) return done(-1, 9, (long long)(key >> 8), mlm_pack_check_text(9), false);
    const unsigned long long front = mlm_pack_front_bytes(n), total = front + 8ull * units;
    sum[0] = (int64_t)n, sum[1] = (int64_t)total, sum[2] = (int64_t)mlm_pack_raw_bytes(n, C), sum[3] = (int64_t)blank, sum[4] = (int64_t)lits, sum[5] = (int64_t)mins,
    sum[6] = (int64_t)maxs;
    const bool writes = stream_given && !(flags & MLM_PACK_F_DRY);
    if (front / 8ull + units > MLM_PACK_MAX_UNITS) return done(-3, 0, -1, nullptr, true);
    if (writes && total > cap_bytes) return done(-3, 0, -1, nullptr, true);
    if (!writes) return done(0, 0, -1, nullptr, true);

    // pass 2 into a block of exactly `total` bytes: a store outside a record ends the program
    std::unique_ptr<uint8_t[]> dst(new uint8_t[total]);
    memset(dst.get(), 7, total);
    const MlmPackHeader H{C, subbox_n, (uint32_t)n, no_infl ? 1u : 0u, min_bits, max_bits, total, lits};
    mlm_pack_header_write(H, dst.get());
    for (size_t r = 0; r < n; ++r) {
        const MlmPackRow R = rows[r];
        const unsigned long long o = front / 8ull + off[r];
        uint8_t *rec = dst.get() + 8ull * o, *dir = dst.get() + MLM_PACK_HEADER + MLM_PACK_DIR * r;
        for (int a = 0; a < 3; ++a) mlm_pack_put32(dir + 4 * a, (uint32_t)keys[3 * r + a]);
        mlm_pack_put32(dir + 12, (uint32_t)o);
        mlm_pack_put32(rec, R.presence), mlm_pack_put32(rec + 4, R.n_lit);
        uint8_t *planes = rec + 8, *lit_at = rec + 8 + 8ull * W * (unsigned long long)__builtin_popcount(R.presence);
        uint32_t base = 0;
        for (uint32_t j = 0; j < W; ++j) {
            unsigned long long b[6], m_min, m_max;
            uint32_t bits[64];
            step(r, j, b, bits, m_min, m_max);
            for (uint32_t k = 0; k < 6; ++k)
                if (R.presence >> k & 1u) {
                    uint8_t *w = planes + 8ull * ((size_t)__builtin_popcount(R.presence & ((1u << k) - 1u)) * W + j);
                    mlm_pack_put32(w, (uint32_t)b[k]), mlm_pack_put32(w + 4, (uint32_t)(b[k] >> 32));
                }
            const unsigned long long lit = b[4] & b[5];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t rank = base + (uint32_t)__builtin_popcountll(lit & (lane ? ~0ull >> (64 - lane) : 0ull));
                if ((lit >> lane & 1ull) && rank < R.n_lit) mlm_pack_put32(lit_at + 4ull * rank, bits[lane]);
            }
            base += (uint32_t)__builtin_popcountll(lit);
        }
        if (R.n_lit & 1u) mlm_pack_put32(lit_at + 4ull * R.n_lit, 0u);
    }
    memcpy(stream.data(), dst.get(), total);
    sum[7] = (int64_t)total;
    return done(0, 0, -1, nullptr, true);
}

int run_unpack(FILE *f, const std::vector<int64_t> &head, const char *path) {
    const uint32_t subbox_n = (uint32_t)head[1], C = subbox_n * subbox_n * subbox_n, W = mlm_pack_words(C);
    const size_t bytes = (size_t)head[2];
    const int flags = (int)head[3];
    const long long cap = head[4];
    const bool keys_out = head[5] & 1, lo_out = head[5] & 2, occ_out = head[5] & 4, infl_out = head[5] & 8;
    std::unique_ptr<uint8_t[]> heap(new uint8_t[bytes]); // (exactly `bytes`: the sanitizer guards both ends)
    if (bytes && fread(heap.get(), 1, bytes, f) != bytes) return 2;
    const uint8_t *s = heap.get();
    const size_t rows_cap = cap > 0 ? (size_t)cap : 0;
    std::vector<int32_t> keys = sevens<int32_t>(3 * rows_cap);
    std::vector<uint32_t> lo = sevens<uint32_t>(rows_cap * C);
    std::vector<uint8_t> occ = sevens<uint8_t>(rows_cap * C), infl = sevens<uint8_t>(rows_cap * C);
    int64_t *const sum = out + 3;
    auto done = [&](int status, int code, long long where, bool with_summary) {
        return finish(path, status, code, where, code ? mlm_unpack_check_text(code) : nullptr, with_summary,
                      {{keys.data(), keys.size() * 4}, {lo.data(), lo.size() * 4}, {occ.data(), occ.size()}, {infl.data(), infl.size()}});
    };
    int bad = mlm_unpack_check(head[6] ? (const void *)s : nullptr, flags, cap, head[7] != 0, head[7] ? 4ull : 0ull);
    if (bad) return done(-1, bad, -1, false);
    MlmPackHeader H{};
    if ((bad = mlm_pack_header_check(s, bytes, C, subbox_n, H))) return done(-1, bad, -1, false);
    const uint32_t n = H.n;

    // the validator: a row and a verdict on the successor per block, then the smallest key
    std::vector<MlmPackRow> rows(n);
    std::vector<uint32_t> next_err(n, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        unsigned long long o, size;
        uint32_t pres, n_lit, fl = 0, c_lit = 0, c_min = 0, c_max = 0;
        const int opened = mlm_pack_block_open(s, H.total, W, n, i, o, pres, n_lit, size);
        if (opened == 0)
            for (uint32_t j = 0; j < W; ++j) {
                unsigned long long w[6];
                mlm_pack_block_words(s, o, W, pres, j, w);
                fl |= mlm_pack_word_check(w, C, j, c_lit, c_min, c_max);
            }
        int next = 0;
        const int own = mlm_pack_block_close(s, H.total, n, i, opened, o, size, fl, n_lit, c_lit, next);
        MlmPackRow R{};
        R.units = (uint32_t)(size / 8ull), R.n_lit = c_lit, R.n_min = c_min, R.n_max = c_max, R.presence = pres, R.err = (uint32_t)own, R.pad0 = 1u;
        rows[i] = R;
        if (i + 1u < n) next_err[i + 1u] = (uint32_t)next;
    }
    unsigned long long key = ~0ull, blank = 0, lits = 0, mins = 0, maxs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long k = mlm_pack_verdict_key(i, rows[i].err, next_err[i]);
        if (k < key) key = k;
        blank += rows[i].units == 1u, lits += rows[i].n_lit, mins += rows[i].n_min, maxs += rows[i].n_max;
    }
    if (key != ~0ull) return done(-1, (int)(key & 0xFFull), (long long)(key >> 8), false);
    sum[0] = n, sum[1] = (int64_t)H.total, sum[2] = (int64_t)mlm_pack_raw_bytes(n, C), sum[3] = (int64_t)blank, sum[4] = (int64_t)lits, sum[5] = (int64_t)mins, sum[6] = (int64_t)maxs;
    const bool writes = keys_out || lo_out || occ_out || infl_out;
    if (writes && (unsigned long long)cap < n) return done(-3, 0, -1, true);
    if (!writes) return done(0, 0, -1, true);

    // the writer
    for (uint32_t i = 0; i < n; ++i) {
        unsigned long long o, size;
        uint32_t pres, n_lit;
        if (mlm_pack_block_open(s, H.total, W, n, i, o, pres, n_lit, size) != 0) return 4; // (never: validated)
        if (keys_out)
            for (int a = 0; a < 3; ++a) keys[3 * (size_t)i + a] = (int32_t)mlm_pack_u32(s + MLM_PACK_HEADER + MLM_PACK_DIR * (unsigned long long)i + 4 * a);
        const uint8_t *lit_at = s + 8ull * o + 8ull + 8ull * W * (unsigned long long)__builtin_popcount(pres);
        uint32_t base = 0;
        for (uint32_t j = 0; j < W; ++j) {
            unsigned long long w[6];
            mlm_pack_block_words(s, o, W, pres, j, w);
            const unsigned long long lit = w[4] & w[5];
            for (uint32_t lane = 0; lane < 64 && 64u * j + lane < C; ++lane) {
                const uint32_t co = (uint32_t)(w[0] >> lane & 1ull) | (uint32_t)(w[1] >> lane & 1ull) << 1, ci = (uint32_t)(w[2] >> lane & 1ull) | (uint32_t)(w[3] >> lane & 1ull) << 1,
                               cv = (uint32_t)(w[4] >> lane & 1ull) | (uint32_t)(w[5] >> lane & 1ull) << 1;
                const uint32_t rank = base + (uint32_t)__builtin_popcountll(lit & (lane ? ~0ull >> (64 - lane) : 0ull));
                const uint32_t literal = cv == 3u && rank < n_lit ? mlm_pack_u32(lit_at + 4ull * rank) : 0u;
                const size_t at = (size_t)i * C + 64u * j + lane;
                if (lo_out) lo[at] = mlm_pack_val_bits(cv, H.min_bits, H.max_bits, literal);
                if (occ_out) occ[at] = mlm_pack_class_byte(co);
                if (infl_out) infl[at] = mlm_pack_class_byte(ci);
            }
            base += (uint32_t)__builtin_popcountll(lit);
        }
    }
    sum[7] = (int64_t)n * (int64_t)((keys_out ? 12 : 0) + (lo_out ? 4 * (int64_t)C : 0) + (occ_out ? (int64_t)C : 0) + (infl_out ? (int64_t)C : 0));
    return done(0, 0, -1, true);
}
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = take<int64_t>(f, 24);
    const int rc = head[0] == 0 ? run_pack(f, head, argv[2]) : run_unpack(f, head, argv[2]);
    fclose(f);
    return rc;
}
