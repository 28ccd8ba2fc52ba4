// mlm_sector_ray.h — the integer walk of one lane's share of a ray of k_sector (mlm_kernels_sector.h), shared with the CPU test driver
// (tests/cpp/sector_ray_driver.cpp).  No LDS or HIP types: the caller's visitor books what the walk finds.
//
// The ray of a hit-centre cell (rho, z) runs radially inwards (map_awareness.cpp:243-274): step k = 1 .. rho-1 is the cell rho - k in row
// z' = round(z - k (z - zc) / rho).  With N_k = 2 (z rho - k (z - zc)) + rho, z' = floor(N_k / 2 rho) unless N_k is a multiple of 2 rho:
// the exact value is then a half-integer — a TIE — and only the reference's own FP64 sequence (mlm_sray_row_fp64) says which way it goes;
// everywhere else that sequence is at most ~1e-12 away from the exact value, which is at least 1 / (2 rho) away from the next half-integer.
// N_k is followed as N_k = q 2 rho + rem: per step rem -= fr, q -= sq (2 (z - zc) = sq 2 rho + fr), one borrow when rem goes negative.
//
//   mask mode      visit(row, word, bits): the cells rho-k of consecutive steps that share a row and a 32-cell word of the miss mask, merged
//                  in a register, as the bits of that word.  Step by step: the bit is carried by rotation, the word by its borrow, the row's
//                  range test is one unsigned compare.  (A form that went from one change of the row or word to the next with one exact
//                  division per run was built and measured: it issued 48 k MORE vector instructions per config-2 frame than this one —
//                  a lane's share is ten steps in three or four runs, and lanes of unequal slope diverge — profiles/r10a_ab.txt.)
//   frontier mode  visit(row, cell, step): every cell needs its time.
// Ties are not visited: the walk returns them as a bit mask (bit k - k_lo) for the caller to resolve with the FP64 sequence under one
// wave-wide test, so that no FP64 code sits in the loop; a call therefore covers at most 64 steps (the caller cuts a longer share — rho above
// 256 with four lanes — into pieces: MLM_SRAY_MAX_STEPS).  Rows outside [0, nZ) are not visited.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_SRAY_HD __host__ __device__ __forceinline__
#else
#define MLM_SRAY_HD inline
#endif
#define MLM_SRAY_MAX_STEPS 64

// a = quo * d + r, 0 <= r < d (|a| < 2^24, 0 < d < 2^24: the float quotient is off by one at most)
MLM_SRAY_HD void mlm_sray_floor_div(int a, int d, int &quo, int &r) {
    quo = (int)floorf((float)a / (float)d);
    r = a - quo * d;
    if (r < 0) {
        r += d;
        --quo;
    } else if (r >= d) {
        r -= d;
        ++quo;
    }
}

// the reference's own sequence for step k (slope rounded, k * slope rounded, z - .. rounded, round half away)
MLM_SRAY_HD int mlm_sray_row_fp64(int rho, int z, int zc, int k) {
    const double slope = (rho > 0) ? (z - zc) / (rho * 1.0) : 0.0;
    return (int)round(z - (k * slope));
}

// steps [k_lo, k_hi) of lane `lane` of the 1 << sh lanes that share the ray's steps 1 .. rho-1
MLM_SRAY_HD void mlm_sray_share(int rho, uint32_t lane, uint32_t sh, int &k_lo, int &k_hi) {
    const int seg = (rho + (int)(1u << sh) - 2) >> sh;
    k_lo = 1 + (int)lane * seg;
    k_hi = rho < k_lo + seg ? rho : k_lo + seg;
}

template <bool FRONTIER, class Visit>
MLM_SRAY_HD unsigned long long mlm_sray_walk(int rho, int z, int zc, int nZ, int k_lo, int k_hi, Visit &&visit) {
    unsigned long long ties = 0;
    if (k_lo >= k_hi) return ties;
    const int dz = z - zc, two_rho = 2 * rho;
    int sq, fr, q, rem;
    mlm_sray_floor_div(2 * dz, two_rho, sq, fr);
    mlm_sray_floor_div(rho * (2 * z + 1) - (k_lo - 1) * 2 * dz, two_rho, q, rem); // N at k_lo - 1
    int k = k_lo;
    // one step of N; true: the step is a tie, which the caller resolves (not to be visited)
    auto step = [&](int &row) {
        rem -= fr;
        q -= sq;
        if (rem < 0) {
            rem += two_rho;
            --q;
        }
        row = q;
        if (rem != 0) return false;
        ties |= 1ull << ((k - k_lo) & 63); // (k - k_lo < MLM_SRAY_MAX_STEPS)
        return true;
    };
    if (FRONTIER) {
        for (; k < k_hi; ++k) {
            int row;
            if (!step(row) && (unsigned)row < (unsigned)nZ) visit(row, rho - k, k);
        }
        return ties;
    }
    // consecutive steps in one row and word are merged in a register (key = row << 4 | word: at most 16 words, rho <= 512)
    int cur = -1;
    uint32_t cur_bits = 0, bit = 1u << ((rho - k) & 31);
    int word = (rho - k) >> 5;
    for (; k < k_hi; ++k) {
        int row;
        if (!step(row)) {
            const int key = (unsigned)row < (unsigned)nZ ? (row << 4) | word : -1;
            if (key != cur) {
                if (cur >= 0) visit(cur >> 4, cur & 15, cur_bits);
                cur = key;
                cur_bits = 0;
            }
            cur_bits |= bit;
        }
        bit = (bit >> 1) | (bit << 31); // (the next cell: one lower)
        word -= (int)(bit >> 31);
    }
    if (cur >= 0) visit(cur >> 4, cur & 15, cur_bits);
    return ties;
}
