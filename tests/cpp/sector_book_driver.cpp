// k_sector's booking (mlm_sector_book.h) both ways on the CPU, into plain array tables:
//   record-wise   every record books on every target of its centre's spread (mlm_book_record: what the kernel did before centres were reduced)
//   centre-wise   every record books on its centre's entry only (target 0, mlm_book_record_centre; the kind bit once per centre); then every
//                 centre's totals are taken from its entry
//                 (mlm_book_centre, all of them before any spread) and booked once on the other targets (mlm_book_centre_target)
// and compares every field of every entry: tmin, the kinds, the whole cnt word (count and strength sum mod 2^11), the rows field of every
// entry that is not flagged as wrapped, and the set of flagged entries; the number of flags of the centre-wise form never exceeds the
// record-wise one's.  The packed target lists are checked against the spread they were made from.
// A spread is synthetic — any function of the centre alone will do: 1 + 2 d targets with d = centre % 5 (up to nine, so that lists
// overflow), target keys centre +- step, kinds 0, 2 d - 1, 2 d as mlm_sec_targets numbers them, a strength 0..3 per (target, kind).
// Record sets: random centres out of few (3 to 60 records per centre), lane masks of every density, first items up to 2^21; some
// sets feed one centre thousands of full masks so that reference counts wrap (rows > 2 047), with and without a second wrapping centre
// that shares its targets.  Prints one line of counters; the test asserts on them.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "mlm_sector_book.h"

struct Cell {
    uint32_t tmin = 0xFFFFFFFFu, kg = 0, cnt = 0;
};
struct Table {
    std::vector<Cell> c;
    std::multiset<int> flagged;
    explicit Table(size_t n) : c(n) {}
    void min_t(int e, uint32_t t) { c[(size_t)e].tmin = std::min(c[(size_t)e].tmin, t); }
    void or_kg(int e, uint32_t bits) { c[(size_t)e].kg |= bits; }
    void add_cnt(int e, uint32_t amount) { c[(size_t)e].cnt += amount; }
    uint32_t add_kg(int e, uint32_t amount) {
        const uint32_t old = c[(size_t)e].kg;
        c[(size_t)e].kg += amount;
        return old;
    }
    void rows_wrapped(int e) { flagged.insert(e); }
};
struct Rec {
    int centre;
    uint32_t i_first, cnt, rows;
};

static const int N_KEYS = 400, PAD = 8; // centres 0 .. N_KEYS - 1 live at entries PAD .. ; targets reach PAD cells to either side
static uint32_t strength_of(int e, uint32_t sub) { return ((uint32_t)e * 7u + sub * 3u) & 3u; }
template <class F> static void spread(int centre, F &&f) {
    f(centre + PAD, 0u);
    const int dmax = centre % 5;
    for (int d = 1; d <= dmax; ++d) {
        f(centre + PAD + d, (uint32_t)(2 * d - 1));
        if ((centre + d) % 3) f(centre + PAD - d, (uint32_t)(2 * d)); // (some spreads are one-sided, as at the map's edge)
    }
}
static uint32_t mask_rows(unsigned long long m) {
    uint32_t n = 0;
    for (int r = 0; r < 8; ++r) n += ((m >> (8 * r)) & 0xFFu) != 0;
    return n;
}

int main() {
    unsigned long long n_sets = 0, n_records = 0, n_centres = 0, n_entries = 0, bad_fields = 0, bad_flags = 0, more_flags = 0, n_wrapped = 0, n_lists = 0,
                       n_list_more = 0, bad_lists = 0;
    std::mt19937_64 rng(20240611);
    for (int set = 0; set < 400; ++set) {
        std::vector<Rec> recs;
        const int n_cent = 1 + (int)(rng() % 40);
        const int wrap_mode = set % 8 == 7 ? 1 + (set / 8) % 2 : 0; // 1: one centre wraps; 2: two wrapping centres share targets
        std::vector<int> centres;
        for (int i = 0; i < n_cent; ++i) centres.push_back((int)(rng() % N_KEYS));
        const int density = set % 4;
        for (int c : centres) {
            const int n = 3 + (int)(rng() % 58);
            for (int i = 0; i < n; ++i) {
                unsigned long long m = rng();
                if (density == 1) m &= rng() & rng();
                if (density == 2) m &= 0xFFull << (8 * (rng() % 8));
                if (density == 3) m = ~0ull;
                if (!m) m = 1ull << (rng() % 64);
                recs.push_back(Rec{c, (uint32_t)(rng() % (1u << 21)), (uint32_t)__builtin_popcountll(m), mask_rows(m)});
            }
        }
        if (wrap_mode) {
            const int c0 = 4 + 5 * (int)(rng() % 70); // (c % 5 == 4: the widest spread)
            const int n = 260 + (int)(rng() % 400); // 8 rows each: 2 080 rows and more
            for (int i = 0; i < n; ++i) recs.push_back(Rec{c0, (uint32_t)(rng() % (1u << 21)), 64u, 8u});
            if (wrap_mode == 2)
                for (int i = 0; i < 300; ++i) recs.push_back(Rec{c0 >= 9 ? c0 - 5 : c0 + 5, (uint32_t)(rng() % (1u << 21)), 64u, 8u}); // (the same spread, four cells shared)
        }
        std::shuffle(recs.begin(), recs.end(), rng);
        // ---- record by record
        Table A((size_t)N_KEYS + 2 * PAD);
        for (const Rec &r : recs)
            spread(r.centre, [&](int e, uint32_t sub) { mlm_book_record(A, e, sub, r.i_first, r.cnt, r.rows, strength_of(e, sub)); });
        // ---- centre by centre
        Table B((size_t)N_KEYS + 2 * PAD);
        for (const Rec &r : recs) mlm_book_record_centre(B, r.centre + PAD, r.i_first, r.cnt, r.rows, strength_of(r.centre + PAD, 0u));
        std::vector<std::pair<int, MlmBookCentre>> cen;
        for (int e = 0; e < (int)B.c.size(); ++e)
            if (B.c[(size_t)e].tmin != 0xFFFFFFFFu) B.c[(size_t)e].kg = mlm_book_centre_kind(B.c[(size_t)e].kg); // (every entry that exists is a centre)
        for (int e = 0; e < (int)B.c.size(); ++e)
            if (B.c[(size_t)e].kg & 1u) cen.push_back({e - PAD, mlm_book_centre(B.c[(size_t)e].tmin, B.c[(size_t)e].kg, B.c[(size_t)e].cnt, B.flagged.count(e) != 0)});
        std::shuffle(cen.begin(), cen.end(), rng);
        for (const auto &c : cen) {
            unsigned long long list = 0;
            uint32_t nt = 0;
            std::vector<uint32_t> want;
            bool wide = false;
            spread(c.first, [&](int e, uint32_t sub) {
                if (sub == 0) return;
                list = mlm_book_list_add(list, nt++, e, sub);
                want.push_back((uint32_t)e | sub << 12);
                wide = wide || sub > 15u;
                mlm_book_centre_target(B, e, sub, c.second, strength_of(e, sub));
            });
            ++n_lists;
            if (want.size() > 4 || wide) {
                ++n_list_more;
                bad_lists += list != MLM_BOOK_LIST_MORE;
            } else {
                bad_lists += list == MLM_BOOK_LIST_MORE || mlm_book_list_count(list) != want.size();
                for (size_t i = 0; i < want.size(); ++i) bad_lists += ((list >> (16 * i)) & 0xFFFFu) != want[i];
            }
        }
        // ---- every field of every entry
        for (size_t e = 0; e < A.c.size(); ++e) {
            const Cell &a = A.c[e], &b = B.c[e];
            const bool fa = A.flagged.count((int)e) != 0, fb = B.flagged.count((int)e) != 0;
            bad_flags += fa != fb;
            more_flags += B.flagged.count((int)e) > A.flagged.count((int)e);
            n_wrapped += fa;
            bad_fields += a.tmin != b.tmin;
            bad_fields += (a.kg & ((1u << MLM_BOOK_KIND_BITS) - 1u)) != (b.kg & ((1u << MLM_BOOK_KIND_BITS) - 1u));
            bad_fields += a.cnt != b.cnt;
            if (!fa) bad_fields += (a.kg >> MLM_BOOK_KIND_BITS) != (b.kg >> MLM_BOOK_KIND_BITS);
            n_entries += a.kg != 0;
        }
        ++n_sets;
        n_records += recs.size();
        n_centres += cen.size();
    }
    std::printf("n_sets %llu n_records %llu n_centres %llu n_entries %llu bad_fields %llu bad_flags %llu more_flags %llu n_wrapped %llu n_lists %llu n_list_more %llu "
                "bad_lists %llu\n",
                n_sets, n_records, n_centres, n_entries, bad_fields, bad_flags, more_flags, n_wrapped, n_lists, n_list_more, bad_lists);
    return 0;
}
