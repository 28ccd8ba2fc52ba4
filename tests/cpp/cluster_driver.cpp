// Test driver for mlm_export_clusters' host arithmetic and per-voxel rules, built by tests/test_cluster_plan.py with
// g++ -fsanitize=address,undefined.
//   cluster_driver plan D0 D1 D2 TILE FRONTIER CAP ...   mlm_cluster_plan (mlmapping_amd/csrc/mlm_host.h) of the cases given (6
//                                                        numbers each); one line per case: the inputs, ok, T, n, tiles, voxels,
//                                                        chunks, the six part sizes, the six offsets, scratch bytes
//   cluster_driver run IN OUT                            the components of one box by the rules of mlmapping_amd/csrc/mlm_cluster.h,
//                                                        driven in the device's phase order — local tile by tile, merge over
//                                                        the pairs a tile border separates, flatten and sizes, chunk counts,
//                                                        scan, ranks and row starts, labels and row updates — only sequentially.
//     IN:  int64 D0 D1 D2 TILE CONNECTIVITY MIN_SIZE CAP LO0 LO1 LO2, then D0*D1*D2 bytes (1: in S)
//     OUT: int64 summary[6], tiles, unions issued; then int32 labels per voxel; then CAP rows of 16 int64 (rows from K on: zero)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_host.h"
#include "mlm_cluster.h"

static int plan_mode(int argc, char **argv) {
    if ((argc - 2) % 6 != 0) return 2;
    for (int i = 2; i + 5 < argc; i += 6) {
        const long long D[3] = {atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2])};
        const long long tile = atoll(argv[i + 3]), fr = atoll(argv[i + 4]), cap = atoll(argv[i + 5]);
        const MlmClusterPlan p = mlm_cluster_plan(D, tile, fr != 0, cap);
        printf("%lld %lld %lld %lld %lld %lld %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld "
               "%lld\n",
               D[0], D[1], D[2], tile, fr, cap, p.ok ? 1 : 0, p.T[0], p.T[1], p.T[2], p.n[0], p.n[1], p.n[2], p.tiles, p.voxels, p.chunks,
               p.field_bytes, p.num_bytes, p.mask_bytes, p.grown_bytes, p.chunk_bytes, p.table_bytes, p.off_num, p.off_mask, p.off_grown,
               p.off_chunk, p.off_table, p.off_ctrl, p.scratch_bytes);
    }
    return 0;
}

static int run_mode(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 3;
    long long hd[10];
    if (fread(hd, 8, 10, f) != 10) return 3;
    const long long D[3] = {hd[0], hd[1], hd[2]}, lo[3] = {hd[7], hd[8], hd[9]};
    const long long cap = hd[6];
    const uint32_t min_size = (uint32_t)hd[5];
    const int nfwd = mlm_cluster_nfwd((int)hd[4]);
    const MlmClusterPlan p = mlm_cluster_plan(D, hd[3], false, cap);
    if (!p.ok || !nfwd) return 4;
    std::vector<uint8_t> mask((size_t)p.voxels);
    if (fread(mask.data(), 1, mask.size(), f) != mask.size()) return 3;
    fclose(f);
    const long long sy = D[0], sz = D[0] * D[1];
    std::vector<uint32_t> field((size_t)p.voxels), num((size_t)p.voxels, 0);
    long long cnt[8] = {0, 0, 0, 0, 0, 0, p.tiles, 0};
    const int T[3] = {(int)p.T[0], (int)p.T[1], (int)p.T[2]};

    // local
    for (long long t = 0; t < p.tiles; ++t) {
        const long long t0 = t % p.n[0], t1 = (t / p.n[0]) % p.n[1], t2 = t / (p.n[0] * p.n[1]);
        const long long o[3] = {t0 * p.T[0], t1 * p.T[1], t2 * p.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)std::min(p.T[a], D[a] - o[a]);
        const int nv = td[0] * td[1] * td[2], tz = td[0] * td[1];
        std::vector<uint32_t> s((size_t)nv);
        auto box = [&](int i) { return (size_t)(((o[2] + i / tz) * D[1] + o[1] + (i / td[0]) % td[1]) * D[0] + o[0] + i % td[0]); };
        bool any = false;
        for (int i = 0; i < nv; ++i) {
            const bool in = mask[box(i)] != 0;
            s[(size_t)i] = in ? (uint32_t)i : MLM_CLUSTER_OFF;
            any |= in;
        }
        long long passes = 0;
        for (bool more = any; more; ++passes) {
            more = false;
            for (int i = 0; i < nv; ++i) {
                const uint32_t w = mlm_cluster_local_step(s.data(), i % td[0], (i / td[0]) % td[1], i / tz, td, nfwd);
                if (w != s[(size_t)i]) {
                    s[(size_t)i] = w;
                    more = true;
                }
            }
        }
        cnt[5] = std::max(cnt[5], passes);
        for (int i = 0; i < nv; ++i) field[box(i)] = s[(size_t)i] == MLM_CLUSTER_OFF ? MLM_CLUSTER_OFF : (uint32_t)box((int)s[(size_t)i]);
    }
    // merge
    auto ld = [&](uint32_t i) { return field[i]; };
    auto amin = [&](uint32_t i, uint32_t v) {
        const uint32_t old = field[i];
        if (v < old) field[i] = v;
        return old;
    };
    for (long long j = 0; j < p.voxels; ++j) {
        if (field[(size_t)j] == MLM_CLUSTER_OFF) continue;
        const long long x = j % sy, y = (j / sy) % D[1], z = j / sz;
        for (int k = 0; k < nfwd; ++k) {
            int dx, dy, dz;
            mlm_cluster_fwd(k, dx, dy, dz);
            if (!mlm_cluster_leaves((int)(x % T[0]), (int)(y % T[1]), (int)(z % T[2]), dx, dy, dz, T)) continue;
            const long long ux = x + dx, uy = y + dy, uz = z + dz;
            if (ux < 0 || ux >= D[0] || uy < 0 || uy >= D[1] || uz >= D[2]) continue;
            const long long u = j + dx + dy * sy + dz * sz;
            if (field[(size_t)u] == MLM_CLUSTER_OFF) continue;
            cnt[7] += mlm_cluster_union(ld, amin, (uint32_t)j, (uint32_t)u);
        }
    }
    // flatten and sizes
    for (long long j = 0; j < p.voxels; ++j) {
        if (field[(size_t)j] == MLM_CLUSTER_OFF) continue;
        const uint32_t root = mlm_cluster_find(ld, (uint32_t)j);
        field[(size_t)j] = root;
        ++num[root];
        ++cnt[0];
    }
    // chunk counts, scan, ranks and row starts
    std::vector<uint32_t> chunk_cnt((size_t)p.chunks, 0);
    for (long long j = 0; j < p.voxels; ++j) {
        if (field[(size_t)j] != (uint32_t)j) continue;
        const uint32_t size = num[(size_t)j];
        ++cnt[1];
        cnt[4] = std::max<long long>(cnt[4], size);
        if (size >= min_size) {
            ++chunk_cnt[(size_t)(j / kClusterChunk)];
            cnt[3] += size;
        }
    }
    for (long long c = 0; c < p.chunks; ++c) {
        const uint32_t v = chunk_cnt[(size_t)c];
        chunk_cnt[(size_t)c] = (uint32_t)cnt[2];
        cnt[2] += v;
    }
    std::vector<int64_t> table((size_t)(cap * MLM_CLUSTER_ROW_I64), 0);
    for (long long c = 0; c < p.chunks; ++c) {
        uint32_t k = chunk_cnt[(size_t)c];
        for (long long j = c * kClusterChunk; j < std::min(p.voxels, (c + 1) * kClusterChunk); ++j) {
            if (field[(size_t)j] != (uint32_t)j) continue;
            const uint32_t size = num[(size_t)j];
            const bool kept = size >= min_size;
            num[(size_t)j] = kept ? k : MLM_CLUSTER_OFF;
            if (kept && k < cap) {
                const long long r[3] = {j % sy, (j / sy) % D[1], j / sz};
                mlm_cluster_row_init(table.data() + (size_t)k * MLM_CLUSTER_ROW_I64, size, r, lo);
            }
            k += kept;
        }
    }
    // labels and rows
    std::vector<int32_t> labels((size_t)p.voxels);
    auto add = [](int64_t *q, int64_t v) { *q += v; };
    auto mn = [](int64_t *q, int64_t v) { *q = std::min(*q, v); };
    auto mx = [](int64_t *q, int64_t v) { *q = std::max(*q, v); };
    auto orr = [](int64_t *q, int64_t v) { *q |= v; };
    for (long long j = 0; j < p.voxels; ++j) {
        const uint32_t root = field[(size_t)j];
        const int32_t lab = mlm_cluster_label(root, root == MLM_CLUSTER_OFF ? MLM_CLUSTER_OFF : num[root]);
        labels[(size_t)j] = lab;
        if (lab < 0 || lab >= cap) continue;
        const long long v[3] = {j % sy, (j / sy) % D[1], j / sz};
        mlm_cluster_row_update(table.data() + (size_t)lab * MLM_CLUSTER_ROW_I64, v, v, v, mlm_cluster_faces(v[0], v[1], v[2], D), lo, add, mn, mx, orr);
    }
    f = fopen(out_path, "wb");
    if (!f) return 3;
    fwrite(cnt, 8, 8, f);
    fwrite(labels.data(), 4, labels.size(), f);
    if (!table.empty()) fwrite(table.data(), 8, table.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "run")) return run_mode(argv[2], argv[3]);
    return 2;
}
