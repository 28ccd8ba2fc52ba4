// mlm_views.h — everything of mlm_query_views (include/mlmap_hip.h) that is not a launch: pure integer code shared by the kernels
// (mlm_kernels_views.h), the host driver (mlmap_hip.hip) and the CPU test driver (tests/cpp/view_driver.cpp), so that all of them
// run the very same arithmetic.  No reference counterpart: the reference has no view query; the classes are those of its point
// queries, the paths are the walk of mlm_raywalk.h, unchanged.
//
// A view is a group of rays.  Its answer is a set cardinality: the distinct voxels on the union of its rays' paths, counted by
// class.  The set is kept as one bit per voxel of the view's bounding box — the box spanned by the start and end voxels of its
// valid rays (a path is monotone per axis, so every voxel of it, the stop voxel included, lies in that box), cut to the caller's
// box B — and a voxel is accounted by whoever sets its bit first (the atomic OR returns the word as it was), so the counters have
// one value whatever the schedule.  The stop predicate is a function of the voxel alone: a voxel is a traversed voxel for every
// ray that meets it or the stop voxel of every such ray, never both, and one bit per voxel is enough.
#pragma once
#include <limits.h>
#include <stddef.h>

#include <vector>

#include "mlm_raywalk.h"

// the box spanned by start and end voxels (inclusive bounds); empty: lo > hi
struct MlmViewBox {
    int lo[3], hi[3];
};
MLM_RW_HD void mlm_view_box_reset(MlmViewBox &b) {
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = INT_MAX;
        b.hi[a] = INT_MIN;
    }
}
// start and end voxel of a ray that mlm_ray_setup accepted, added to the box
MLM_RW_HD void mlm_view_box_add(MlmViewBox &b, const MlmRayState &S, int n) {
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        const int v = S.g[a] * n + S.c[a], e = v + S.s[a] * S.r[a];
        const int l = v < e ? v : e, h = v < e ? e : v;
        b.lo[a] = l < b.lo[a] ? l : b.lo[a];
        b.hi[a] = h > b.hi[a] ? h : b.hi[a];
    }
}

// the caller's box B (lo, dims as mlm_export_window's; on = 0: all voxels)
struct MlmViewWindow {
    int on;
    int lo[3], d[3];
};

// a view's bounding box cut to B: origin, edges (0: empty) and bits; refused: more than 2^31 - 1 of them
struct MlmViewClip {
    int lo[3], d[3];
    long long bits;
    int refused;
};
MLM_RW_HD void mlm_view_clip(const MlmViewBox &raw, const MlmViewWindow &B, MlmViewClip &C) {
    bool empty = false;
    long long bits = 1;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        long long l = raw.lo[a], h = raw.hi[a];
        if (B.on) {
            const long long bl = B.lo[a], bh = bl + B.d[a] - 1; // (lo + dims fits an int32)
            l = l > bl ? l : bl;
            h = h < bh ? h : bh;
        }
        empty = empty || l > h;
        const long long d = l > h ? 0 : h - l + 1; // (|v| <= 2^30: at most 2^31 + 1)
        C.lo[a] = l > h ? 0 : (int)l;
        C.d[a] = (int)(d > INT_MAX ? INT_MAX : d);
        // (a product of three edges <= 2^31 + 1 overflows 64 bits: saturate as soon as it is past the limit)
        bits = bits > 0x7FFFFFFFll ? bits : bits * d;
    }
    C.refused = !empty && bits > 0x7FFFFFFFll;
    C.bits = (empty || C.refused) ? 0 : bits;
    if (empty || C.refused) C.d[0] = C.d[1] = C.d[2] = 0;
}
// the bit of voxel v in the view's box; -1: outside (not accounted)
MLM_RW_HD int mlm_view_bit(const MlmViewClip &C, int vx, int vy, int vz) {
    const unsigned int x = (unsigned int)vx - (unsigned int)C.lo[0], y = (unsigned int)vy - (unsigned int)C.lo[1],
                       z = (unsigned int)vz - (unsigned int)C.lo[2];
    if (x >= (unsigned int)C.d[0] || y >= (unsigned int)C.d[1] || z >= (unsigned int)C.d[2]) return -1;
    return (int)((z * (unsigned int)C.d[1] + y) * (unsigned int)C.d[0] + x); // (< bits <= 2^31 - 1)
}
// the element of voxel v in the window layout of B (exclude / mark); v lies in B
MLM_RW_HD size_t mlm_view_at(const MlmViewWindow &B, int vx, int vy, int vz) {
    return ((size_t)(vz - B.lo[2]) * (size_t)B.d[1] + (size_t)(vy - B.lo[1])) * (size_t)B.d[0] + (size_t)(vx - B.lo[0]);
}

// Was the bit clear in the word the atomic OR returned?  (MLM_VIEWS_NO_DEDUP: an experiment build that counts every visit, what
// summing per-ray counts amounts to — it must fail the value comparisons of the tests.)
MLM_RW_HD bool mlm_view_new(unsigned int old_word, unsigned int mask) {
#ifdef MLM_VIEWS_NO_DEDUP
    (void)old_word, (void)mask;
    return true;
#else
    return (old_word & mask) == 0;
#endif
}
// The accounting of a voxel seen for the first time in its view: class bits as MlmRayClasses returns them (1 occ OCCUPIED,
// 2 inflated OCCUPIED, 4 occ UNKNOWN; neither 1 nor 4: FREE), stop: it is a stop voxel, excluded: its exclude byte is non-zero.
// Table words [0] traversed, [1] of those UNKNOWN, [2] of those FREE, [3] stop voxels.
MLM_RW_HD void mlm_view_account(int bits, bool stop, bool excluded, unsigned int &n_trav, unsigned int &n_unknown, unsigned int &n_free,
                                unsigned int &n_stop) {
    // (no branch on stop: with one, the compiler keeps n_trav / n_stop in a stack slot it indexes by stop)
    const unsigned int s = !excluded && stop ? 1u : 0u, t = !excluded && !stop ? 1u : 0u;
    n_stop += s;
    n_trav += t;
    n_unknown += t & ((unsigned int)(bits >> 2) & 1u);
    n_free += t & ((bits & 5) == 0 ? 1u : 0u);
}
MLM_RW_HD unsigned char mlm_view_mark_bits(bool stop) { return stop ? 2 : 1; }

// One ray of a view: mlm_ray_walk's loop with a visitor in place of the count — visit(vx, vy, vz, class bits, stop) for path
// indices 0 .. k-1 (stop = false) and for the stop voxel at index k.  Returns the status (1 stopped, 0 reached the end, -1 invalid:
// nothing visited); n_steps as mlm_query_rays.
template <class Cls, class Visit>
MLM_RW_HD int mlm_view_walk(const double p0[3], const double p1[3], double d, int n, int flags, Cls &cls, Visit &visit, int &n_steps) {
    MlmRayState S;
    n_steps = 0;
    if (!mlm_ray_setup(p0, p1, d, n, S)) return -1;
    int k = 0, m_in = 0, d_in = 1;
    bool nb = true;
    for (;;) {
        const int bits = cls(S.g, S.c, nb);
        const bool stop = (bits & flags) != 0;
        visit(S.g[0] * n + S.c[0], S.g[1] * n + S.c[1], S.g[2] * n + S.c[2], bits, stop);
        if (stop) {
            n_steps = k;
            return 1;
        }
        ++k;
        if ((S.r[0] | S.r[1] | S.r[2]) == 0) break;
        nb = mlm_ray_step(S, n, m_in, d_in);
    }
    n_steps = k;
    return 0;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
// A view whose bitset has at most `lds_bits` bits (knob "view_lds_bits", default and most kViewLdsBits) gets one workgroup with the
// bitset in LDS; the launch of a size class reserves that class's bytes, so that small views do not run at the occupancy of the
// largest: 8, 16, 32, 48 and 64 KiB (the last less the 64 bytes of the workgroup's counters: a launch stays within 64 KiB) leave 20,
// 10, 5, 3 and 2 workgroups of kViewLdsThreads lanes room in a CU's 160 KiB (how many of them run is then up to the kernel's
// registers: DESIGN.md).  A 64 x 48 fan of 4 m at d = 0.1 needs 10-46 KiB, depending on how it lies to the axes.
// Every other view keeps its bitset in global scratch and is walked by several workgroups, one per kViewGlobalThreads rays, at most
// kViewMaxParts; global views run in batches whose bitsets together stay within kViewScratchWords (a launch is as wide as its batch:
// the budget is what keeps the machine filled when the views are sparse fans in large boxes).
constexpr int kViewRow = 8; // MLM_VIEW_ROW
constexpr int kViewLdsClasses = 5;
constexpr int kViewGlobal = kViewLdsClasses; // the class of the global path
constexpr int kViewLdsThreads = 512, kViewGlobalThreads = 256, kViewMaxParts = 256;
constexpr long long kViewLdsBits = (64 * 1024 - 64) * 8;
constexpr long long kViewScratchWords = 1ll << 26; // 256 MiB: the largest view that is not refused; 512 views of 0.5 MiB a launch
constexpr int kViewBoxRays = 4096;                 // rays of a workgroup of the bounding-box pass
MLM_RW_HD int mlm_view_class_bytes(int cls) { return cls == 0 ? 8192 : cls == 1 ? 16384 : cls == 2 ? 32768 : cls == 3 ? 49152 : 65472; }
MLM_RW_HD long long mlm_view_words(long long bits) { return (bits + 31) >> 5; }
MLM_RW_HD int mlm_view_class(long long bits, long long lds_bits) {
    if (bits > lds_bits || bits > kViewLdsBits) return kViewGlobal;
    int cls = 0;
    while (mlm_view_class_bytes(cls) < mlm_view_words(bits) * 4) ++cls;
    return cls;
}
MLM_RW_HD int mlm_view_parts(long long rays) {
    const long long p = (rays + kViewGlobalThreads - 1) / kViewGlobalThreads;
    return (int)(p < 1 ? 1 : p > kViewMaxParts ? kViewMaxParts : p);
}

// What a workgroup is given: a view (index within the call's chunk of views), its rays (indices within the chunk's rays), and on
// the global path its share (rays ray0 + part * threads + lane, stride parts * threads) and where the view's bitset starts.
struct MlmViewJob {
    int view, ray0, ray1;
    int part, parts, pad;
    long long word_off;
};

// Views of a chunk by path.  begin[k] .. begin[k + 1]: the rays of view k, relative to the chunk.
struct MlmViewPlan {
    std::vector<MlmViewJob> lds[kViewLdsClasses]; // one job per view
    std::vector<MlmViewJob> global;               // parts of a view in a row, views in batch order
    struct Batch {
        size_t job0, job1; // of `global`
        long long words;   // scratch words the batch's bitsets take
    };
    std::vector<Batch> batches;
    std::vector<int> refused;
    long long scratch_words = 0; // the largest batch
};
inline MlmViewPlan mlm_view_plan(const MlmViewBox *raw, const long long *begin, int n_views, const MlmViewWindow &B, long long lds_bits) {
    MlmViewPlan P;
    long long used = 0;
    for (int k = 0; k < n_views; ++k) {
        MlmViewClip C;
        mlm_view_clip(raw[k], B, C);
        if (C.refused) {
            P.refused.push_back(k);
            continue;
        }
        const int cls = mlm_view_class(C.bits, lds_bits);
        MlmViewJob j{k, (int)begin[k], (int)begin[k + 1], 0, 1, 0, 0};
        if (cls < kViewGlobal) {
            P.lds[cls].push_back(j);
            continue;
        }
        const long long w = mlm_view_words(C.bits);
        if (P.batches.empty() || used + w > kViewScratchWords) {
            P.batches.push_back({P.global.size(), P.global.size(), 0});
            used = 0;
        }
        j.word_off = used;
        j.parts = mlm_view_parts(begin[k + 1] - begin[k]);
        for (j.part = 0; j.part < j.parts; ++j.part) P.global.push_back(j);
        used += w;
        P.batches.back().job1 = P.global.size();
        P.batches.back().words = used;
        P.scratch_words = used > P.scratch_words ? used : P.scratch_words;
    }
    return P;
}
