// mlm_sector_book.h — the integer forms of k_sector's booking (mlm_kernels_sector.h): what a hit record adds to its centre cell, what
// the spread pass takes back from that cell as the centre's totals, what it adds to every other target of the centre's spread, and how
// a centre's targets are packed for the reference pass.  Plain integer code shared by the kernel and the CPU test driver
// (tests/cpp/sector_book_driver.cpp), which books record sets both ways — record by record and centre by centre — and compares the tables.
//
// A table is reached through a visitor T (the kernel's works on LDS atomics, the driver's on a plain array):
//   void min_t(int e, uint32_t t)              MlmSecCell::tmin = min(tmin, t)
//   uint32_t add_kg(int e, uint32_t amount)    MlmSecCell::kg += amount, returns the old word
//   void or_kg(int e, uint32_t bits)           MlmSecCell::kg |= bits
//   void add_cnt(int e, uint32_t amount)       MlmSecCell::cnt += amount
//   void rows_wrapped(int e)                   the entry's reference count has wrapped
//
// Why booking a centre's totals once gives the bits that booking its records one by one gives.  Per target (centre, sub) a record r adds
//   tmin   min with i_first_r * MLM_TIME_SLOTS + sub        min_r(i_first_r * 21 + sub) = (min_r i_first_r) * 21 + sub
//   kinds  OR of 1 << sub                                   OR
//   cnt    + cnt_r                                          the sum of the records' counts
//   strength field (kept mod 2^11)  + cnt_r * s             sum_r(cnt_r * s) = (sum_r cnt_r) * s  (mod 2^11), s depends on (centre, sub) only
//   reference rows  + rows_r                                sums only grow: "some add crossed 2 047" = "the final sum exceeds 2 047": the same cells
//                                                           are flagged
// What may differ: how many times a wrapped cell is flagged (there are fewer adds, and every flag of the centre-wise form stands for a
// multiple of 2 048 that some record's add of the record-wise form crosses): a column gives up for "more than eight flags" less often
// than record by record, never more often.  The rows field of a flagged cell (its sum mod 2^11) is not used by anything.
#pragma once
#include <stdint.h>

#ifndef MLM_TIME_SLOTS
#define MLM_TIME_SLOTS 21 // (as mlm_types.h has it: the CPU drivers include this header on its own)
#endif
#ifndef MLM_SEC_CNT_BITS
#define MLM_SEC_CNT_BITS 21 // (as mlm_host.h has it)
#endif
#define MLM_BOOK_KIND_BITS 21 // (MLM_SEC_KIND_BITS of mlm_kernels_sector.h; the kernel asserts they are one value)
#define MLM_BOOK_ROWS_MAX (0xFFFFFFFFu >> MLM_BOOK_KIND_BITS)

#ifdef __HIPCC__
#define MLM_SB_HD __host__ __device__ __forceinline__
#else
#define MLM_SB_HD inline
#endif

// ---- the amounts of one target
MLM_SB_HD uint32_t mlm_book_time(uint32_t i_first, uint32_t sub) { return i_first * MLM_TIME_SLOTS + sub; }
// contributions, and above them (mod 2^11) the sum of their strengths
MLM_SB_HD uint32_t mlm_book_cnt_amount(uint32_t cnt, uint32_t strength) { return cnt | ((cnt * strength) << MLM_SEC_CNT_BITS); }
MLM_SB_HD uint32_t mlm_book_rows_amount(uint32_t rows) { return rows << MLM_BOOK_KIND_BITS; }
// did the add of `rows` to a kg word that was `old_kg` carry out of the rows field?
MLM_SB_HD bool mlm_book_rows_carry(uint32_t old_kg, uint32_t rows) { return (old_kg >> MLM_BOOK_KIND_BITS) + rows > MLM_BOOK_ROWS_MAX; }

// One record on one target: the record-wise form (what every target got before centres were reduced), and what a record still does on its
// CENTRE's entry (target sub = 0 of its own spread).  strength: of (rho of the target, sub).
template <class T> MLM_SB_HD void mlm_book_record(T &tab, int e, uint32_t sub, uint32_t i_first, uint32_t cnt, uint32_t rows, uint32_t strength) {
    tab.min_t(e, mlm_book_time(i_first, sub));
    tab.or_kg(e, 1u << sub);
    tab.add_cnt(e, mlm_book_cnt_amount(cnt, strength));
    if (mlm_book_rows_carry(tab.add_kg(e, mlm_book_rows_amount(rows)), rows)) tab.rows_wrapped(e);
}

// The same on the record's centre less the kind bit: every entry that exists when the records are through is a centre, and the spread
// pass sets bit 0 of its kinds once (mlm_book_centre_kind) instead of once per record.
template <class T> MLM_SB_HD void mlm_book_record_centre(T &tab, int e, uint32_t i_first, uint32_t cnt, uint32_t rows, uint32_t strength) {
    tab.min_t(e, mlm_book_time(i_first, 0u));
    tab.add_cnt(e, mlm_book_cnt_amount(cnt, strength));
    if (mlm_book_rows_carry(tab.add_kg(e, mlm_book_rows_amount(rows)), rows)) tab.rows_wrapped(e);
}
MLM_SB_HD uint32_t mlm_book_centre_kind(uint32_t kg) { return kg | 1u; }

// ---- a centre's totals.  While only centre contributions have been booked, the centre's own entry IS the accumulator: its tmin is
// (min i_first) * MLM_TIME_SLOTS + 0, the low bits of its cnt the sum of the counts, the rows field of its kg the sum of the rows (mod
// 2^11; `wrapped`: the entry was flagged, the sum exceeds 2 047 — all that matters of it).  The spread pass takes them before any other
// target is booked:
//   t0   bits 0-30 (min i_first) * MLM_TIME_SLOTS, bit 31 the rows sum has wrapped
//   cr   bits 0-20 the count, bits 21-31 the rows (mod 2^11)
struct MlmBookCentre {
    uint32_t t0, cr;
};
#define MLM_BOOK_WRAPPED 0x80000000u
MLM_SB_HD MlmBookCentre mlm_book_centre(uint32_t tmin, uint32_t kg, uint32_t cnt, bool wrapped) {
    MlmBookCentre c;
    c.t0 = tmin | (wrapped ? MLM_BOOK_WRAPPED : 0u);
    c.cr = (cnt & ((1u << MLM_SEC_CNT_BITS) - 1u)) | (kg & ~((1u << MLM_BOOK_KIND_BITS) - 1u));
    return c;
}
static_assert(MLM_SEC_CNT_BITS == MLM_BOOK_KIND_BITS, "a centre's count and rows share one word");
// the centre's totals on one OTHER target of its spread (sub >= 1)
template <class T> MLM_SB_HD void mlm_book_centre_target(T &tab, int e, uint32_t sub, MlmBookCentre c, uint32_t strength) {
    const uint32_t cnt = c.cr & ((1u << MLM_SEC_CNT_BITS) - 1u), rows = c.cr >> MLM_BOOK_KIND_BITS;
    tab.min_t(e, (c.t0 & ~MLM_BOOK_WRAPPED) + sub);
    tab.or_kg(e, 1u << sub);
    tab.add_cnt(e, mlm_book_cnt_amount(cnt, strength));
    const uint32_t old = tab.add_kg(e, mlm_book_rows_amount(rows));
    // (a centre whose own sum wrapped flags every target once, whatever the add of its remainder does)
    if ((c.t0 & MLM_BOOK_WRAPPED) || mlm_book_rows_carry(old, rows)) tab.rows_wrapped(e);
}

// ---- a centre's other targets as the reference pass wants them: (table entry | sub << 12) in 16 bits each, four at most, filled from
// bit 0 (a target other than the centre has sub >= 1: no field of a target is zero).  MLM_BOOK_LIST_MORE: more than four, or a sub above
// 15 — the reference pass runs the spread again for the centre's records.
#define MLM_BOOK_LIST_MORE 1ull // (entry 1 with sub 0: no target's field)
MLM_SB_HD unsigned long long mlm_book_list_add(unsigned long long list, uint32_t n, int e, uint32_t sub) {
    if (list == MLM_BOOK_LIST_MORE || n >= 4u || sub > 15u) return MLM_BOOK_LIST_MORE;
    return list | (unsigned long long)((uint32_t)e | (sub << 12)) << (16u * n);
}
MLM_SB_HD uint32_t mlm_book_list_count(unsigned long long list) { // (list != MLM_BOOK_LIST_MORE)
    return list ? 4u - ((uint32_t)__builtin_clzll(list) >> 4) : 0u;
}
