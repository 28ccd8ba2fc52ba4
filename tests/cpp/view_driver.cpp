// Test driver for the accounting of mlm_query_views on the host: the rules of mlmapping_amd/csrc/mlm_views.h (bounding box, clipping,
// bit index, accounting of a newly seen voxel, the plan) over the walk of mlm_raywalk.h and the classes of MapView::RayClasses
// (mlm_mapview.h) — the code the kernels of mlm_kernels_views.h run too — built by tests/test_view_plan.py with g++
// -fsanitize=address,undefined (no HIP, no GPU).  Views are processed in the plan's order and with the plan's buffers: a view of an
// LDS class in a bitset of that class's bytes, the global path's views batch by batch in one scratch at their offsets.
// Input blob: d_sub f64; lds_bits i64; n, n_blocks, n_rays, n_views, flags, has_box, has_exclude, has_mark i32; lo, dims [3] i32;
// keys [n_blocks*3] i32; collapsed [n_blocks] u8; occ, infl [n_blocks*cells] u8; p0, p1 [n_rays*3] f64; view_begin [n_views+1] i32;
// exclude, mark [voxels of the box] u8 when present.  Output file: table [n_views*8] i64; class per view [n_views] i32 (0.. LDS class,
// 5 global, -1 refused); mark [voxels of the box] u8 when present.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mlm_mapview.h"
#include "mlm_views.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

struct Visit {
    const MlmViewWindow &B;
    const MlmViewClip &C;
    uint32_t *bits;
    size_t words; // of the buffer the plan gave the view
    const uint8_t *exclude;
    uint8_t *mark;
    unsigned int n[4] = {0, 0, 0, 0};
    void operator()(int vx, int vy, int vz, int cls, bool stop) {
        const int idx = mlm_view_bit(C, vx, vy, vz);
        if (idx < 0) return;
        if ((size_t)(idx >> 5) >= words) std::abort(); // (the plan's buffer holds the view's box)
        const unsigned int m = 1u << (idx & 31), old = bits[idx >> 5];
        bits[idx >> 5] = old | m;
        if (!mlm_view_new(old, m)) return;
        bool excluded = false;
        if (B.on) {
            const size_t at = mlm_view_at(B, vx, vy, vz);
            if (exclude) excluded = exclude[at] != 0;
            if (mark) mark[at] |= mlm_view_mark_bits(stop);
        }
        mlm_view_account(cls, stop, excluded, n[0], n[1], n[2], n[3]);
    }
};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double d_sub;
    long long lds_bits;
    int32_t hdr[8], box[6];
    if (!rd(f, &d_sub, 8) || !rd(f, &lds_bits, 8) || !rd(f, hdr, sizeof hdr) || !rd(f, box, sizeof box)) return 2;
    const int n = hdr[0], nb = hdr[1], nr = hdr[2], nv = hdr[3], flags = hdr[4], C = n * n * n;
    MlmViewWindow B{};
    size_t nvox = 0;
    if (hdr[5]) {
        B.on = 1;
        nvox = 1;
        for (int a = 0; a < 3; ++a) {
            B.lo[a] = box[a];
            B.d[a] = box[3 + a];
            nvox *= (size_t)box[3 + a];
        }
    }
    std::vector<int32_t> keys((size_t)nb * 3), vb((size_t)nv + 1);
    std::vector<uint8_t> col((size_t)nb), occ((size_t)nb * C), infl((size_t)nb * C), exclude(hdr[6] ? nvox : 0), mark(hdr[7] ? nvox : 0);
    std::vector<double> p0((size_t)nr * 3), p1((size_t)nr * 3);
    if (!rd(f, keys.data(), keys.size() * 4) || !rd(f, col.data(), col.size()) || !rd(f, occ.data(), occ.size()) || !rd(f, infl.data(), infl.size()) ||
        !rd(f, p0.data(), p0.size() * 8) || !rd(f, p1.data(), p1.size() * 8) || !rd(f, vb.data(), vb.size() * 4) ||
        !rd(f, exclude.data(), exclude.size()) || !rd(f, mark.data(), mark.size()))
        return 2;
    std::fclose(f);
    mlm_host::MapView v;
    v.d_sub = d_sub;
    v.n = n;
    v.cells = C;
    v.d_glb = d_sub * n;
    v.d_sub_half = d_sub * 0.5;
    v.occ = occ.data(), v.infl = infl.data(), v.col = col.data();
    v.table_reset((size_t)nb);
    for (int b = 0; b < nb; ++b) v.table_insert(keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2], b);

    // the bounding boxes, the plan
    std::vector<MlmViewBox> raw((size_t)nv);
    std::vector<long long> begin((size_t)nv + 1);
    for (int k = 0; k <= nv; ++k) begin[(size_t)k] = vb[(size_t)k];
    for (int k = 0; k < nv; ++k) {
        mlm_view_box_reset(raw[(size_t)k]);
        for (long long i = begin[(size_t)k]; i < begin[(size_t)k + 1]; ++i) {
            MlmRayState S;
            if (mlm_ray_setup(&p0[3 * (size_t)i], &p1[3 * (size_t)i], d_sub, n, S)) mlm_view_box_add(raw[(size_t)k], S, n);
        }
    }
    const MlmViewPlan plan = mlm_view_plan(raw.data(), begin.data(), nv, B, lds_bits);
    std::vector<int64_t> table((size_t)nv * kViewRow, 0);
    std::vector<int32_t> cls_of((size_t)nv, -2);

    auto run = [&](const MlmViewJob &J, uint32_t *bits, size_t words) {
        MlmViewClip clip;
        mlm_view_clip(raw[(size_t)J.view], B, clip);
        Visit visit{B, clip, bits, words, exclude.empty() ? nullptr : exclude.data(), mark.empty() ? nullptr : mark.data()};
        mlm_host::MapView::RayClasses rc{v};
        int64_t *row = &table[(size_t)J.view * kViewRow];
        for (long long i = (long long)J.ray0 + J.part; i < J.ray1; i += J.parts) { // (a part's share; the lane stride is the kernel's)
            int k_steps;
            const int st = mlm_view_walk(&p0[3 * (size_t)i], &p1[3 * (size_t)i], d_sub, n, flags, rc, visit, k_steps);
            if (st < 0) {
                row[5] += 1;
            } else {
                row[4] += st;
                row[6] += k_steps;
            }
        }
        for (int c = 0; c < 4; ++c) row[c] += visit.n[c];
    };
    for (int c = 0; c < kViewLdsClasses; ++c) {
        const size_t words = (size_t)mlm_view_class_bytes(c) / 4;
        std::vector<uint32_t> bits(words);
        for (const MlmViewJob &J : plan.lds[c]) {
            MlmViewClip clip;
            mlm_view_clip(raw[(size_t)J.view], B, clip);
            if ((size_t)mlm_view_words(clip.bits) > words || cls_of[(size_t)J.view] != -2) return 5;
            cls_of[(size_t)J.view] = c;
            for (size_t w = 0; w < (size_t)mlm_view_words(clip.bits); ++w) bits[w] = 0u; // (what the kernel clears)
            run(J, bits.data(), words);
        }
    }
    std::vector<uint32_t> scratch((size_t)plan.scratch_words);
    for (const MlmViewPlan::Batch &b : plan.batches) {
        if (b.words > plan.scratch_words || (b.words > kViewScratchWords && plan.global[b.job1 - 1].view != plan.global[b.job0].view)) return 5;
        for (size_t w = 0; w < (size_t)b.words; ++w) scratch[w] = 0u;
        for (size_t j = b.job0; j < b.job1; ++j) {
            const MlmViewJob &J = plan.global[j];
            MlmViewClip clip;
            mlm_view_clip(raw[(size_t)J.view], B, clip);
            if (J.word_off + mlm_view_words(clip.bits) > b.words) return 5;
            if (J.part == 0 && cls_of[(size_t)J.view] != -2) return 5;
            cls_of[(size_t)J.view] = kViewGlobal;
            run(J, scratch.data() + J.word_off, (size_t)mlm_view_words(clip.bits));
        }
    }
    for (int k : plan.refused) {
        if (cls_of[(size_t)k] != -2) return 5;
        cls_of[(size_t)k] = -1;
        table[(size_t)k * kViewRow + 7] = 1;
    }
    for (int k = 0; k < nv; ++k)
        if (cls_of[(size_t)k] == -2) return 5; // (every view is on exactly one path)
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(table.data(), 8, table.size(), o);
    std::fwrite(cls_of.data(), 4, cls_of.size(), o);
    if (!mark.empty()) std::fwrite(mark.data(), 1, mark.size(), o);
    std::fclose(o);
    return 0;
}
