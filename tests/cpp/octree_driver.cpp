// Test driver for mlm_export_octree's host arithmetic and rules, built by tests/test_octree_plan.py with g++ -fsanitize=address,undefined.
//   octree_driver plan LO0 LO1 LO2 D0 D1 D2 DEPTH ...   mlm_oct_plan (mlmapping_amd/csrc/mlm_octree.h) of the cases given (7 numbers each);
//                                      one line per case: why, T, bricks, cells, lab_bytes, cnt_bytes, the five offsets, scratch bytes,
//                                      then off[T .. depth + 1]
//   octree_driver args FLAGS CAPN ANYN CAPM ANYM SUMMARY ...   mlm_oct_args of the cases given (6 numbers each), one result per line
//   octree_driver run IN OUT           the tree of one box by the rules of mlm_octree.h, driven in the device's phase order — bricks up
//                                      (with the counters), the levels above them up, the root, down to the bricks, then per range of
//                                      rows the cells above the bricks and the wanted bricks rebuilt and walked down — only sequentially.
//     IN:  int64 D0 D1 D2 LO0 LO1 LO2 DEPTH FLAGS CAPN CAPM WHICH STEP (WHICH: bit 0 words, 1 inner4, 2 skip, 3 leaf4, 4 leaf_class
//          wanted; STEP: rows per range, 0: one range), then the occ classes and the infl classes of the box, D0 D1 D2 int8 each
//     OUT: int64 summary[40]; then words [CAPN] uint16, inner4 [CAPN][4] int32, skip [CAPN] int32, leaf4 [CAPM][4] int32,
//          leaf_class [CAPM] int8 — every byte 0x77 where the rules wrote nothing
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mlm_octree.h"

static int plan_mode(int argc, char **argv) {
    if ((argc - 2) % 7 != 0) return 2;
    for (int i = 2; i + 6 < argc; i += 7) {
        const long long lo[3] = {atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2])}, D[3] = {atoll(argv[i + 3]), atoll(argv[i + 4]), atoll(argv[i + 5])};
        const int depth = atoi(argv[i + 6]);
        const MlmOctPlan p = mlm_oct_plan(lo, D, depth);
        printf("%d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", p.why, p.T, p.bricks, p.cells, p.lab_bytes, p.cnt_bytes, p.off_icnt, p.off_lcnt,
               p.off_ib, p.off_lb, p.off_ctrl, p.scratch_bytes);
        if (!p.why)
            for (int l = p.T; l <= depth + 1; ++l) printf(" %lld", p.off[l]);
        printf("\n");
    }
    return 0;
}

static int args_mode(int argc, char **argv) {
    if ((argc - 2) % 6 != 0) return 2;
    for (int i = 2; i + 5 < argc; i += 6)
        printf("%d\n", mlm_oct_args(atoi(argv[i]), atoll(argv[i + 1]), atoi(argv[i + 2]) != 0, atoll(argv[i + 3]), atoi(argv[i + 4]) != 0,
                                    atoi(argv[i + 5]) != 0));
    return 0;
}

// the labels of the voxels of brick cb, as mlm_oct_brick_load leaves them
static void brick_load(const MlmOctGeo &G, const long long cb[3], const int8_t *occ, const int8_t *infl, MlmOctBrick &B) {
    const int T = G.T, side = 1 << T;
    for (int j = 0; j < (1 << (3 * T)); ++j) {
        const long long v[3] = {(cb[0] << T) - G.half + (j & (side - 1)), (cb[1] << T) - G.half + ((j >> T) & (side - 1)), (cb[2] << T) - G.half + (j >> (2 * T))};
        int label = MLM_OCT_NONE;
        if (v[0] >= G.lo[0] && v[0] < G.lo[0] + G.D[0] && v[1] >= G.lo[1] && v[1] < G.lo[1] + G.D[1] && v[2] >= G.lo[2] && v[2] < G.lo[2] + G.D[2]) {
            const size_t at = (size_t)(((v[2] - G.lo[2]) * G.D[1] + (v[1] - G.lo[1])) * G.D[0] + (v[0] - G.lo[0]));
            label = mlm_oct_class(occ[at], infl[at], G.flags);
        }
        B.lab[j] = (uint8_t)label;
    }
}
static void brick_reduce(MlmOctBrick &B, int T, unsigned *cnt) {
    for (int l = 1; l <= T; ++l)
        for (int j = 0; j < (1 << (3 * (T - l))); ++j) mlm_oct_brick_up(B, T, l, j, cnt);
}

static int run_mode(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 3;
    long long hd[12];
    if (fread(hd, 8, 12, f) != 12) return 3;
    const long long D[3] = {hd[0], hd[1], hd[2]}, lo[3] = {hd[3], hd[4], hd[5]};
    const int depth = (int)hd[6], flags = (int)hd[7], which = (int)hd[10];
    const long long cap_n = hd[8], cap_m = hd[9], step = hd[11];
    const MlmOctPlan p = mlm_oct_plan(lo, D, depth);
    if (p.why || mlm_oct_args(flags, cap_n, cap_n > 0, cap_m, cap_m > 0, true)) return 4;
    const size_t nvox = (size_t)(D[0] * D[1] * D[2]);
    std::vector<int8_t> occ(nvox), infl(nvox);
    if (fread(occ.data(), 1, nvox, f) != nvox || fread(infl.data(), 1, nvox, f) != nvox) return 3;
    fclose(f);
    const MlmOctGeo G = mlm_oct_geo(lo, D, depth, flags, p);
    std::vector<unsigned char> scratch((size_t)p.scratch_bytes, 0x11); // (nothing may rely on zeroed scratch but the control block)
    const MlmOctUpper U = mlm_oct_upper(scratch.data(), p);
    memset(U.ctrl, 0, (size_t)kOctCtrlBytes);
    auto B = std::make_unique<MlmOctBrick>();
    const int T = G.T;

    // up: the bricks
    for (long long b = 0; b < p.bricks; ++b) {
        long long cb[3];
        mlm_oct_cell_at(G, T, b, cb);
        memset(B.get(), 0x11, sizeof(MlmOctBrick));
        brick_load(G, cb, occ.data(), infl.data(), *B);
        unsigned cnt[10] = {0};
        brick_reduce(*B, T, cnt);
        U.lab[G.off[T] + b] = B->lab[mlm_oct_lab_at(T)];
        U.icnt[G.off[T] + b] = B->icnt[mlm_oct_cnt_at(T)];
        U.lcnt[G.off[T] + b] = B->lcnt[mlm_oct_cnt_at(T)];
        for (int i = 0; i < 4; ++i) {
            U.ctrl[kOctCtrlOccLeaves + i] += cnt[i];
            U.ctrl[kOctCtrlFreeLeaves + i] += cnt[4 + i];
        }
        U.ctrl[kOctCtrlOccVox] += cnt[8];
        U.ctrl[kOctCtrlFreeVox] += cnt[9];
    }
    // up: the levels above; the root; down to the bricks
    for (int l = T + 1; l <= depth; ++l)
        for (long long j = 0; j < G.off[l + 1] - G.off[l]; ++j) mlm_oct_upper_up(G, U, l, j);
    mlm_oct_root(G, U);
    for (int l = depth; l > T; --l)
        for (long long j = 0; j < G.off[l + 1] - G.off[l]; ++j) mlm_oct_upper_down(G, U, l, j);
    int64_t sm[MLM_OCT_ROW_I64];
    mlm_oct_summary(U.ctrl, sm);

    // rows, range by range
    std::vector<uint16_t> words((size_t)cap_n, 0x7777);
    std::vector<int32_t> inner4((size_t)cap_n * 4, 0x77777777), skip((size_t)cap_n, 0x77777777), leaf4((size_t)cap_m * 4, 0x77777777);
    std::vector<int8_t> leaf_class((size_t)cap_m, 0x77);
    const long long nN = std::min<long long>(sm[0], cap_n), nM = std::min<long long>(sm[1], cap_m);
    const long long nstep = step > 0 ? std::min(nN, step) : nN, mstep = step > 0 ? std::min(nM, step) : nM;
    for (long long n0 = 0, m0 = 0; n0 < nN || m0 < nM;) {
        const long long n1 = std::min(nN, n0 + nstep), m1 = std::min(nM, m0 + mstep);
        MlmOctOut O{};
        if (n1 > n0) {
            O.words = (which & 1) ? words.data() + n0 : nullptr;
            O.inner4 = (which & 2) ? inner4.data() + 4 * n0 : nullptr;
            O.skip = (which & 4) ? skip.data() + n0 : nullptr;
        }
        if (m1 > m0) {
            O.leaf4 = (which & 8) ? leaf4.data() + 4 * m0 : nullptr;
            O.leaf_class = (which & 16) ? leaf_class.data() + m0 : nullptr;
        }
        O.n0 = n0, O.n1 = n1, O.m0 = m0, O.m1 = m1;
        mlm_oct_root_emit(G, U, O);
        for (long long j = G.off[T + 1]; j < G.off[depth + 1]; ++j) {
            const int l = mlm_oct_level_of(G, j);
            mlm_oct_upper_emit(G, U, O, l, j - G.off[l]);
        }
        for (long long b = 0; b < p.bricks; ++b) {
            if (!mlm_oct_brick_wanted(G, U, O, b)) continue;
            long long cb[3];
            mlm_oct_cell_at(G, T, b, cb);
            memset(B.get(), 0x11, sizeof(MlmOctBrick));
            brick_load(G, cb, occ.data(), infl.data(), *B);
            brick_reduce(*B, T, nullptr);
            B->ib[mlm_oct_cnt_at(T)] = U.ib[G.off[T] + b];
            B->lb[mlm_oct_cnt_at(T)] = U.lb[G.off[T] + b];
            const long long kb[3] = {cb[0] << T, cb[1] << T, cb[2] << T};
            for (int l = T; l >= 1; --l)
                for (int j = 0; j < (1 << (3 * (T - l))); ++j) mlm_oct_brick_down(*B, G, O, kb, l, j);
        }
        n0 = n1;
        m0 = m1;
    }
    f = fopen(out_path, "wb");
    if (!f) return 3;
    fwrite(sm, 8, MLM_OCT_ROW_I64, f);
    if (cap_n) {
        fwrite(words.data(), 2, words.size(), f);
        fwrite(inner4.data(), 4, inner4.size(), f);
        fwrite(skip.data(), 4, skip.size(), f);
    }
    if (cap_m) {
        fwrite(leaf4.data(), 4, leaf4.size(), f);
        fwrite(leaf_class.data(), 1, leaf_class.size(), f);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "args")) return args_mode(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "run")) return run_mode(argv[2], argv[3]);
    return 2;
}
