// mlm_boxgrow.h — the box growth of mlm_query_boxes (include/mlmap_hip.h): validity, the limit arithmetic, the round and face loop and
// the counters, once, for the kernel (mlm_kernels_boxes.h), the host mirror (MapView::boxes, mlm_mapview.h) and the CPU test driver
// (tests/cpp/box_driver.cpp), so that all three run the very same control flow.  No reference counterpart: the reference has no
// volume query; the classes of the voxels are those of its point queries (what mlm_export_window's occ / infl channels return).
//
// Faces: 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z (axis = face >> 1, outward direction = face & 1).  A box is lo[3], hi[3], inclusive.
//
// The voxels come from a callable
//     void scan(const int32_t lo[3], const int32_t hi[3], int flags, bool full, long long &n_unknown, long long &n_obstacle)
// that ADDS to n_unknown the voxels of the box lo..hi whose occ class is UNKNOWN and to n_obstacle those with (bits & flags) != 0,
// bits being the MLM_BOX_* classes (1 getOccupancy == OCCUPIED, 2 getInflateOccupancy == OCCUPIED, 4 getOccupancy == UNKNOWN).
// With full == false it may return as soon as n_obstacle != 0 (both counts are then discarded: a rejected slab); with full == true
// it counts every voxel (the blocked start reports its obstacle voxels in full).  On the device the callable is run by a whole wave and
// returns the same counts in every lane, so everything below is wave-uniform.
//
// All coordinates that can leave int32 (the next layer of a face, extents, volumes) are 64-bit.  A side is at most 2^15 + 2 * 4096,
// so a slab has fewer than 40 960^2 < 2^31 voxels and a box fewer than 2^46.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_BG_HD __host__ __device__ __forceinline__
#define MLM_BG_UNROLL _Pragma("unroll") // (the per-axis and per-face arrays live in registers: no loop over them may stay a loop)
#else
#define MLM_BG_HD inline
#define MLM_BG_UNROLL
#endif

#define MLM_BOX_MAX_GROW 4096
#define MLM_BOX_MAX_SIDE (1 << 15) // b - a >= this on an axis: an invalid item

struct MlmBoxLimits {
    int32_t grow[6];         // most layers per face, 0 .. MLM_BOX_MAX_GROW
    int32_t on;              // a limit window is given:
    int32_t wlo[3], whi[3];  // its first and last voxel per axis (inclusive)
};

struct MlmBoxResult {
    int status;        // 1 grown, 0 blocked start, -1 invalid
    int32_t box[6];    // the final box, lo then hi
    uint32_t closed;   // bit c: face c was closed by an obstacle
    long long row[4];  // voxels of the final box, of those UNKNOWN, of those with O, slabs absorbed
};

MLM_BG_HD bool mlm_box_valid(const int32_t b[6], const MlmBoxLimits &L) {
    bool ok = true;
    MLM_BG_UNROLL
    for (int a = 0; a < 3; ++a) {
        const long long lo = b[a], hi = b[3 + a];
        ok = ok && lo <= hi && hi - lo < MLM_BOX_MAX_SIDE;
        if (L.on) ok = ok && lo >= L.wlo[a] && hi <= L.whi[a];
    }
    return ok;
}

MLM_BG_HD long long mlm_box_volume(const int32_t lo[3], const int32_t hi[3]) {
    long long v = 1;
    MLM_BG_UNROLL
    for (int a = 0; a < 3; ++a) v *= (long long)hi[a] - lo[a] + 1;
    return v;
}

// Most voxels the final box of a valid item can have (the mirror's work bound): B0 plus max_grow per face, cut to the window.
MLM_BG_HD long long mlm_box_limit_volume(const int32_t b[6], const MlmBoxLimits &L) {
    long long v = 1;
    MLM_BG_UNROLL
    for (int a = 0; a < 3; ++a) {
        long long lo = (long long)b[a] - L.grow[2 * a], hi = (long long)b[3 + a] + L.grow[2 * a + 1];
        if (L.on) {
            lo = lo < L.wlo[a] ? L.wlo[a] : lo;
            hi = hi > L.whi[a] ? L.whi[a] : hi;
        }
        v *= hi - lo + 1;
    }
    return v;
}

// The whole contract for one item.
template <class Scan> MLM_BG_HD void mlm_box_grow(const int32_t b6[6], int flags, const MlmBoxLimits &L, Scan &scan, MlmBoxResult &o) {
    MLM_BG_UNROLL
    for (int k = 0; k < 6; ++k) o.box[k] = b6[k];
    o.closed = 0;
    o.row[0] = o.row[1] = o.row[2] = o.row[3] = 0;
    if (!mlm_box_valid(b6, L)) {
        o.status = -1;
        return;
    }
    int32_t lo[3], hi[3];
    MLM_BG_UNROLL
    for (int a = 0; a < 3; ++a) {
        lo[a] = b6[a];
        hi[a] = b6[3 + a];
    }
    long long unk = 0, obs = 0;
    scan(lo, hi, flags, true, unk, obs);
    o.row[0] = mlm_box_volume(lo, hi);
    o.row[1] = unk;
    o.row[2] = obs;
    if (obs) {
        o.status = 0;
        return;
    }
    o.status = 1;
    int32_t grown[6] = {0, 0, 0, 0, 0, 0};
    uint32_t open = 63u, closed = 0;
    long long slabs = 0;
    while (open) {
        for (int c = 0; c < 6; ++c) {
            const uint32_t bit = 1u << c;
            if (!(open & bit)) continue;
            const int ax = c >> 1;
            const bool up = (c & 1) != 0;
            // the face's next layer, its count so far and its limits (selected without indexing the arrays by a variable)
            long long next = 0, wl = 0, wh = 0;
            int32_t done = 0, most = 0;
            MLM_BG_UNROLL
            for (int a = 0; a < 3; ++a)
                if (a == ax) {
                    next = up ? (long long)hi[a] + 1 : (long long)lo[a] - 1;
                    wl = L.wlo[a];
                    wh = L.whi[a];
                }
            MLM_BG_UNROLL
            for (int k = 0; k < 6; ++k)
                if (k == c) {
                    done = grown[k];
                    most = L.grow[k];
                }
            if (done >= most || next > 2147483647ll || next < -2147483648ll || (L.on && (next < wl || next > wh))) {
                open &= ~bit; // closed by limit
                continue;
            }
            int32_t slo[3], shi[3];
            MLM_BG_UNROLL
            for (int a = 0; a < 3; ++a) {
                slo[a] = a == ax ? (int32_t)next : lo[a];
                shi[a] = a == ax ? (int32_t)next : hi[a];
            }
            long long su = 0, so = 0;
            scan(slo, shi, flags, false, su, so);
            if (so) {
                open &= ~bit; // closed by obstacle
                closed |= bit;
                continue;
            }
            MLM_BG_UNROLL
            for (int a = 0; a < 3; ++a)
                if (a == ax) {
                    if (up) hi[a] = (int32_t)next;
                    else lo[a] = (int32_t)next;
                }
            MLM_BG_UNROLL
            for (int k = 0; k < 6; ++k)
                if (k == c) grown[k] = done + 1;
            unk += su; // (counters are committed only when the slab is absorbed)
            ++slabs;
        }
    }
    MLM_BG_UNROLL
    for (int a = 0; a < 3; ++a) {
        o.box[a] = lo[a];
        o.box[3 + a] = hi[a];
    }
    o.closed = closed;
    o.row[0] = mlm_box_volume(lo, hi);
    o.row[1] = unk;
    o.row[3] = slabs;
}
