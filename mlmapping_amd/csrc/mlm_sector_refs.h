// mlm_sector_refs.h — the integer forms of k_sector's reference pass (mlm_kernels_sector.h): how a reference of a multi-kind cell is
// packed, what the pass keeps of a cell (its origin, once per cell instead of once per (record, cell) pair) and of a record (the flags
// of its non-empty mask rows, taken one by one with a find-first-bit).  Plain integer code shared by the kernel and the CPU test
// driver (tests/cpp/sector_refs_driver.cpp), which holds every form here to the straightforward one.
#pragma once
#include <stdint.h>

#ifndef MLM_TIME_SLOTS
#define MLM_TIME_SLOTS 21 // (as mlm_types.h has it: the CPU drivers include this header on its own)
#endif

#ifdef __HIPCC__
#define MLM_SR_HD __host__ __device__ __forceinline__
#else
#define MLM_SR_HD inline
#endif

// A reference of a multi-kind cell = one non-empty row of the 8x8 lane mask of one contribution group, 4 bytes:
//   bits 0-7 the row's byte of the mask, 8-12 the kind, 13-31 where the row's first lane lies relative to the cell's FIRST pixel
//   (its earliest contribution, MlmSecCell::tmin: no contribution lies in a row above it):
//     dense images   (rows below the first pixel's) << 8 | 128 + (tile column - the first pixel's tile column)   11 + 8 bits
//     lists          (64-item rows below the first item's) << 3 | mask row      16 + 3 bits (2^22 items)
#define MLM_REF_DY_DENSE 2047u
#define MLM_REF_DY_LIST 65535u
// (xrel: the row's tile column relative to the tile column of the cell's first pixel, + MLM_REF_XREL0: an image may be any width, a cell's
// contributions lie within 1 016 pixels of its first one's column — else the frame gives the sector path up)
#define MLM_REF_XREL0 128u
MLM_SR_HD uint32_t mlm_ref_pack(uint32_t bits, uint32_t kind, bool dense, uint32_t dy0, uint32_t row, uint32_t xrel) {
    const uint32_t pos = dense ? ((dy0 + row) << 8) | xrel : (dy0 << 3) | row;
    return bits | (kind << 8) | (pos << 13);
}
// The same word from what a group's rows share: base = mlm_ref_pack(0, kind, dense, dy0, 0, xrel), then per row
// base + (row << shift) + bits.  The fields below the position do not overlap (bits < 256, kind < 32, xrel < 256, row < 8), and the
// row enters the position as a sum in both layouts, so the sums are the packed word (mod 2^32, as mlm_ref_pack's shifts are).
MLM_SR_HD uint32_t mlm_ref_row_shift(bool dense) { return dense ? 21u : 13u; }
MLM_SR_HD uint32_t mlm_ref_repack(uint32_t base, uint32_t shift, uint32_t row, uint32_t bits) { return base + (row << shift) + bits; }

// ---- a cell's origin: what its references are relative to, from its first-touch time tmin = first pixel * MLM_TIME_SLOTS + kind.
//   dense images   (row of the first pixel) << osh | its tile column (column >> 3), osh = bits of the image's last tile column:
//                  row * width <= pixel and 2^osh <= max(1, width / 4), so the packed word is at most a quarter of the pixel index:
//                  exact for every image (tile columns have 13 bits at most, MLM_SEC_MAX_WIDTH)
//   lists          first item >> 6 (its 64-item row)
// row_m, row_s: exact division by the image width (mlm_host.h: div_magic, pixels below 2^27).
MLM_SR_HD uint32_t mlm_sec_origin_shift(int tile_w) {
    const uint32_t last = tile_w > 0 ? ((uint32_t)tile_w - 1u) >> 3 : 0u;
    return last ? 32u - (uint32_t)__builtin_clz(last) : 0u;
}
MLM_SR_HD uint32_t mlm_sec_origin(uint32_t tmin, int tile_w, uint32_t osh, unsigned long long row_m, int row_s) {
    const uint32_t pix0 = tmin / MLM_TIME_SLOTS;
    if (tile_w <= 0) return pix0 >> 6;
    const uint32_t y0c = (uint32_t)(((unsigned long long)pix0 * row_m) >> row_s);
    return (y0c << osh) | ((pix0 - y0c * (uint32_t)tile_w) >> 3);
}
MLM_SR_HD uint32_t mlm_sec_origin_row(uint32_t origin, bool dense, uint32_t osh) { return dense ? origin >> osh : origin; }
MLM_SR_HD uint32_t mlm_sec_origin_xt(uint32_t origin, uint32_t osh) { return origin & ((1u << osh) - 1u); }

// ---- a record's non-empty mask rows (bytes of its 8x8 lane mask) as flags in one word: row r at bit 8 (r & 3) + 4 (r >> 2).
// (per half of the mask: a byte is non-zero iff its low seven bits carry into bit 7 or bit 7 is set)
MLM_SR_HD uint32_t mlm_sec_row_flags(unsigned long long mask) {
    const uint32_t lo = (uint32_t)mask, hi = (uint32_t)(mask >> 32);
    const uint32_t flo = (((lo & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | lo) & 0x80808080u;
    const uint32_t fhi = (((hi & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | hi) & 0x80808080u;
    return (flo >> 7) | (fhi >> 3);
}
// the lowest flag's row and its byte of the mask (flags != 0); the caller clears it with flags &= flags - 1
MLM_SR_HD void mlm_sec_row_take(uint32_t flags, unsigned long long mask, uint32_t &row, uint32_t &bits) {
    const uint32_t b = (uint32_t)__builtin_ctz(flags);
    row = (b >> 3) | (b & 4u);
    bits = (((b & 4u) ? (uint32_t)(mask >> 32) : (uint32_t)mask) >> (b & 24u)) & 0xFFu;
}
