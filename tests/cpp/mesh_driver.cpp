// Test driver for mlm_export_mesh's host arithmetic and rules, built by tests/test_mesh_plan.py with g++ -fsanitize=address,undefined.
//   mesh_driver plan D0 D1 D2 ...      mlm_mesh_plan (mlmapping_amd/csrc/mlm_mesh.h) of the boxes given (3 numbers each); one line per
//                                      box: the inputs, why, voxels, lattice, grown, words, fchunks, vchunks, the six part sizes, the
//                                      six offsets, scratch bytes
//   mesh_driver args FLAGS CAPF ANYF CAPV ANYV SUMMARY ...   mlm_mesh_args of the cases given (6 numbers each), one result per line
//   mesh_driver div                    mlm_mesh_div against the machine's division on divisors and dividends around every edge;
//                                      prints the number of disagreements
//   mesh_driver run IN OUT             the mesh of one box by the rules of mlm_mesh.h, driven in the device's phase order — states,
//                                      masks and bits (with the summary counters), chunk counts, scan, word bases, rows — only
//                                      sequentially.
//     IN:  int64 D0 D1 D2 FLAGS CAPF CAPV LO0 LO1 LO2 N WHICH 0 (WHICH: bit 0 quads, 1 face4, 2 vert3, 3 xyz, 4 n3 wanted), double
//          D_SUB, then the occ classes and the infl classes of the grown box, (D0 + 2)(D1 + 2)(D2 + 2) int8 each
//     OUT: int64 summary[12]; then quads [CAPF][4] int32, face4 [CAPF][4] int32, vert3 [CAPV][3] int32, xyz [CAPV][3] float,
//          n3 [CAPV][3] int8 — every byte 0x77 where the rules wrote nothing
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_mesh.h"

static int plan_mode(int argc, char **argv) {
    if ((argc - 2) % 3 != 0) return 2;
    for (int i = 2; i + 2 < argc; i += 3) {
        const long long D[3] = {atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2])};
        const MlmMeshPlan p = mlm_mesh_plan(D);
        printf("%lld %lld %lld %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", D[0], D[1], D[2], p.why,
               p.voxels, p.lattice, p.grown, p.words, p.fchunks, p.vchunks, p.state_bytes, p.fmask_bytes, p.bits_bytes, p.wbase_bytes, p.fchunk_bytes,
               p.vchunk_bytes, p.off_fmask, p.off_bits, p.off_wbase, p.off_fchunk, p.off_vchunk, p.off_ctrl, p.scratch_bytes);
    }
    return 0;
}

static int args_mode(int argc, char **argv) {
    if ((argc - 2) % 6 != 0) return 2;
    for (int i = 2; i + 5 < argc; i += 6)
        printf("%d\n", mlm_mesh_args(atoi(argv[i]), atoll(argv[i + 1]), atoi(argv[i + 2]) != 0, atoll(argv[i + 3]), atoi(argv[i + 4]) != 0,
                                     atoi(argv[i + 5]) != 0));
    return 0;
}

static int div_mode() {
    const uint32_t ds[] = {1u, 2u, 3u, 5u, 7u, 10u, 63u, 64u, 65u, 1000u, 65535u, 65536u, 65537u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFFu};
    long long bad = 0, n = 0;
    for (uint32_t d : ds) {
        const MlmMeshDiv v = mlm_mesh_div_by(d);
        auto check = [&](unsigned long long i) {
            if (i > 0xFFFFFFFFull) return;
            ++n;
            bad += mlm_mesh_div((uint32_t)i, v) != (uint32_t)i / d;
        };
        for (unsigned long long q : {0ull, 1ull, 2ull, 1000ull, 0xFFFFFFFFull / d - 1, 0xFFFFFFFFull / d, 0x7FFFFFFFull / d})
            for (long long e = -3; e <= 3; ++e)
                if ((long long)(q * d) + e >= 0) check((unsigned long long)((long long)(q * d) + e));
        for (unsigned long long i = 0; i < 5000; ++i) check(i * 858993ull + 7);
        for (unsigned long long i = 0xFFFFFFFFull - 2000; i <= 0xFFFFFFFFull; ++i) check(i);
    }
    printf("%lld %lld\n", bad, n);
    return 0;
}

static int run_mode(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 3;
    long long hd[12];
    double d_sub;
    if (fread(hd, 8, 12, f) != 12 || fread(&d_sub, 8, 1, f) != 1) return 3;
    const long long D[3] = {hd[0], hd[1], hd[2]}, lo[3] = {hd[6], hd[7], hd[8]};
    const int flags = (int)hd[3], n = (int)hd[9], which = (int)hd[10];
    const long long cap_f = hd[4], cap_v = hd[5];
    const MlmMeshPlan p = mlm_mesh_plan(D);
    if (p.why || mlm_mesh_args(flags, cap_f, cap_f > 0, cap_v, cap_v > 0, true) || n < 1) return 4;
    std::vector<int8_t> occ((size_t)p.grown), infl((size_t)p.grown);
    if (fread(occ.data(), 1, occ.size(), f) != occ.size() || fread(infl.data(), 1, infl.size(), f) != infl.size()) return 3;
    fclose(f);
    const MlmMeshGeo G = mlm_mesh_geo(D, lo, n, d_sub, d_sub * n, flags);
    const size_t gy = (size_t)G.gy, gz = (size_t)G.gz;

    // states of the grown box
    std::vector<uint8_t> state((size_t)p.grown);
    for (long long z = 0; z < D[2] + 2; ++z)
        for (long long y = 0; y < D[1] + 2; ++y)
            for (long long x = 0; x < D[0] + 2; ++x) {
                const size_t g = (size_t)z * gz + (size_t)y * gy + (size_t)x;
                const bool inside = x >= 1 && x <= D[0] && y >= 1 && y <= D[1] && z >= 1 && z <= D[2];
                state[g] = mlm_mesh_state(occ[g], infl[g], flags, inside);
            }
    // masks and bits, the summary counters
    long long sm[MLM_MESH_ROW_I64] = {0};
    std::vector<uint8_t> fmask((size_t)p.voxels);
    std::vector<unsigned long long> bits((size_t)p.words, 0ull);
    for (long long j = 0; j < p.voxels; ++j) {
        uint32_t x, y, z;
        mlm_mesh_split((uint32_t)j, G.by_d0, G.by_d1, x, y, z);
        const size_t g = (size_t)(z + 1) * gz + (size_t)(y + 1) * gy + (size_t)(x + 1);
        const unsigned m = mlm_mesh_faces(state.data(), g, gy, gz);
        fmask[(size_t)j] = (uint8_t)m;
        sm[2] += state[g] & 1;
        sm[3] += m != 0;
        for (int a = 0; a < 6; ++a) sm[4 + a] += (m >> a) & 1u;
        sm[10] += __builtin_popcount(m & mlm_mesh_rim(x, y, z, G.D));
    }
    for (long long L = 0; L < p.lattice; ++L) {
        uint32_t k0, k1, k2;
        mlm_mesh_split((uint32_t)L, G.by_l0, G.by_l1, k0, k1, k2);
        int nrm[3];
        if (mlm_mesh_vertex(state.data(), (size_t)k2 * gz + (size_t)k1 * gy + (size_t)k0, gy, gz, nrm)) bits[(size_t)(L >> 6)] |= 1ull << (L & 63);
    }
    // chunk counts, scan (one entry more: the total)
    std::vector<unsigned long long> fchunk((size_t)p.fchunks + 1, 0ull), vchunk((size_t)p.vchunks + 1, 0ull);
    for (long long j = 0; j < p.voxels; ++j) fchunk[(size_t)(j / kMeshChunk)] += (unsigned)__builtin_popcount(fmask[(size_t)j]);
    for (long long w = 0; w < p.words; ++w) vchunk[(size_t)(w / (kMeshChunk / 64))] += (unsigned)__builtin_popcountll(bits[(size_t)w]);
    auto scan = [](std::vector<unsigned long long> &v) {
        unsigned long long carry = 0;
        for (auto &e : v) {
            const unsigned long long c = e;
            e = carry;
            carry += c;
        }
    };
    scan(fchunk);
    scan(vchunk);
    sm[0] = (long long)fchunk.back();
    sm[1] = (long long)vchunk.back();
    // word bases
    std::vector<uint32_t> wbase((size_t)p.words);
    for (long long c = 0; c < p.vchunks; ++c) {
        uint32_t before = (uint32_t)vchunk[(size_t)c];
        for (long long w = c * (kMeshChunk / 64); w < std::min(p.words, (c + 1) * (kMeshChunk / 64)); ++w) {
            wbase[(size_t)w] = before;
            before += (uint32_t)__builtin_popcountll(bits[(size_t)w]);
        }
    }
    // rows
    std::vector<int32_t> quads((size_t)cap_f * 4, 0x77777777), face4((size_t)cap_f * 4, 0x77777777), vert3((size_t)cap_v * 3, 0x77777777);
    std::vector<float> xyz((size_t)cap_v * 3);
    if (!xyz.empty()) memset(xyz.data(), 0x77, xyz.size() * sizeof(float));
    std::vector<int8_t> n3((size_t)cap_v * 3, 0x77);
    for (long long L = 0; L < p.lattice; ++L) {
        if (!((bits[(size_t)(L >> 6)] >> (L & 63)) & 1ull)) continue;
        const long long k = mlm_mesh_vertex_number(bits.data(), wbase.data(), (uint32_t)L);
        if (k >= cap_v) continue;
        mlm_mesh_vertex_row(G, state.data(), (uint32_t)L, (which & 4) ? vert3.data() + k * 3 : nullptr, (which & 8) ? xyz.data() + k * 3 : nullptr,
                            (which & 16) ? n3.data() + k * 3 : nullptr);
    }
    for (long long c = 0; c < p.fchunks; ++c) {
        long long fnum = (long long)fchunk[(size_t)c];
        for (long long j = c * kMeshChunk; j < std::min(p.voxels, (c + 1) * kMeshChunk); ++j) {
            const unsigned m = fmask[(size_t)j];
            if (!m) continue;
            uint32_t x, y, z;
            mlm_mesh_split((uint32_t)j, G.by_d0, G.by_d1, x, y, z);
            for (int a = 0; a < 6; ++a) {
                if (!((m >> a) & 1u)) continue;
                if (fnum < cap_f)
                    mlm_mesh_face_row(G, x, y, z, a, bits.data(), wbase.data(), (which & 1) ? quads.data() + fnum * 4 : nullptr,
                                      (which & 2) ? face4.data() + fnum * 4 : nullptr);
                ++fnum;
            }
        }
    }
    f = fopen(out_path, "wb");
    if (!f) return 3;
    fwrite(sm, 8, MLM_MESH_ROW_I64, f);
    if (cap_f) {
        fwrite(quads.data(), 4, quads.size(), f);
        fwrite(face4.data(), 4, face4.size(), f);
    }
    if (cap_v) {
        fwrite(vert3.data(), 4, vert3.size(), f);
        fwrite(xyz.data(), 4, xyz.size(), f);
        fwrite(n3.data(), 1, n3.size(), f);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "args")) return args_mode(argc, argv);
    if (argc == 2 && !strcmp(argv[1], "div")) return div_mode();
    if (argc == 4 && !strcmp(argv[1], "run")) return run_mode(argv[2], argv[3]);
    return 2;
}
