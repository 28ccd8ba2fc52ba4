// Test driver for mlm_export_route's host arithmetic and per-voxel rules, built by tests/test_route_plan.py with
// g++ -fsanitize=address,undefined.
//   route_driver plan D0 D1 D2 TILE SEEDS ...   mlm_route_plan (mlmapping_amd/csrc/mlm_host.h) of the cases given (5 numbers each); one
//                                               line per case: the inputs, ok, T, n, tiles, voxels, field / class / dirty / seed
//                                               bytes, the four offsets, scratch bytes, LDS bytes, cap
//   route_driver run IN OUT                     the field of one box by the rules of mlmapping_amd/csrc/mlm_route.h, driven as the
//                                               device drives them: class bytes from D_out, tile by tile against a full
//                                               one-voxel halo, dirty arrays that swap roles from sweep to sweep, stop at the
//                                               first sweep that marks nothing — only sequentially.
//     IN:  int64 D0 D1 D2 TILE MAX_COST SEEDS CONNECTIVITY W0 W1 W2 CLEARANCE NPEN, then NPEN int32 penalties, SEEDS x 3 int32
//          (relative to the box), then D0*D1*D2 uint16 D_out
//     OUT: int64 traversable, reached, largest cost, sweeps, cap, tiles; then int32 cost, uint8 parent and uint8 class per voxel
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_host.h"
#include "mlm_route.h"

static int plan_mode(int argc, char **argv) {
    if ((argc - 2) % 5 != 0) return 2;
    for (int i = 2; i + 4 < argc; i += 5) {
        const long long D[3] = {atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2])};
        const long long tile = atoll(argv[i + 3]), seeds = atoll(argv[i + 4]);
        const MlmRoutePlan p = mlm_route_plan(D, tile, seeds);
        printf("%lld %lld %lld %lld %lld %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", D[0], D[1],
               D[2], tile, seeds, p.ok ? 1 : 0, p.T[0], p.T[1], p.T[2], p.n[0], p.n[1], p.n[2], p.tiles, p.voxels, p.field_bytes, p.class_bytes,
               p.dirty_bytes, p.seed_bytes, p.off_class, p.off_dirty, p.off_ctrl, p.off_seeds, p.scratch_bytes, p.lds_bytes, p.cap);
    }
    return 0;
}

struct Box {
    long long D[3];
    std::vector<uint32_t> field;
    uint32_t at(long long x, long long y, long long z) const {
        if (x < 0 || x >= D[0] || y < 0 || y >= D[1] || z < 0 || z >= D[2]) return MLM_REACH_BLOCKED;
        return field[(size_t)((z * D[1] + y) * D[0] + x)];
    }
};

struct Rules {
    int connectivity;
    uint32_t move_cost[3], max_cost;
    uint32_t pen[64];
};

template <int CONN>
static uint32_t relax(const std::vector<uint32_t> &s, size_t c, int sy, int sz, uint32_t pen, const Rules &r) {
    return mlm_route_relax<CONN>(s[c], pen, r.move_cost, r.max_cost,
                                 [&](int dx, int dy, int dz) { return s[(size_t)((long long)c + dx + dy * sy + dz * sz)]; });
}

// one tile of one sweep: stage, relax to the tile's fixpoint, write back, mark the tiles whose halo holds a lowered voxel
static bool sweep_tile(Box &B, const std::vector<uint8_t> &cls, const MlmRoutePlan &p, long long t, const Rules &r, std::vector<uint8_t> &next) {
    const long long t0 = t % p.n[0], t1 = (t / p.n[0]) % p.n[1], t2 = t / (p.n[0] * p.n[1]);
    const long long o[3] = {t0 * p.T[0], t1 * p.T[1], t2 * p.T[2]};
    int td[3];
    for (int a = 0; a < 3; ++a) td[a] = (int)std::min(p.T[a], B.D[a] - o[a]);
    const int sy = td[0] + 2, sz = sy * (td[1] + 2), hv = sz * (td[2] + 2);
    std::vector<uint32_t> s((size_t)hv);
    for (int i = 0; i < hv; ++i) s[(size_t)i] = B.at(o[0] + i % sy - 1, o[1] + (i / sy) % (td[1] + 2) - 1, o[2] + i / sz - 1);
    bool more = true;
    while (more) {
        more = false;
        for (int iz = 0; iz < td[2]; ++iz)
            for (int iy = 0; iy < td[1]; ++iy)
                for (int ix = 0; ix < td[0]; ++ix) {
                    const size_t c = (size_t)((iz + 1) * sz + (iy + 1) * sy + ix + 1);
                    const uint32_t pen = mlm_route_pen(r.pen, cls[(size_t)(((o[2] + iz) * B.D[1] + o[1] + iy) * B.D[0] + o[0] + ix)]);
                    const uint32_t v = s[c], w = r.connectivity == 6    ? relax<6>(s, c, sy, sz, pen, r)
                                                 : r.connectivity == 18 ? relax<18>(s, c, sy, sz, pen, r)
                                                                        : relax<26>(s, c, sy, sz, pen, r);
                    if (w != v) {
                        s[c] = w;
                        more = true;
                    }
                }
    }
    uint32_t mask = 0;
    for (int iz = 0; iz < td[2]; ++iz)
        for (int iy = 0; iy < td[1]; ++iy)
            for (int ix = 0; ix < td[0]; ++ix) {
                const uint32_t v = s[(size_t)((iz + 1) * sz + (iy + 1) * sy + ix + 1)];
                uint32_t &g = B.field[(size_t)(((o[2] + iz) * B.D[1] + o[1] + iy) * B.D[0] + o[0] + ix)];
                if (v < g) {
                    g = v;
                    mask |= mlm_route_dirty_mask(mlm_reach_faces(ix, iy, iz, td), r.connectivity);
                }
            }
    bool marked = false;
    for (int k = 0; k < 27; ++k)
        if ((mask >> k) & 1u) {
            const long long nt = mlm_route_tile_at(t0, t1, t2, p.n, k);
            if (nt >= 0) {
                next[(size_t)nt] = 1;
                marked = true;
            }
        }
    return marked;
}

static int run_mode(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 3;
    long long hd[12];
    if (fread(hd, 8, 12, f) != 12) return 3;
    Box B;
    for (int a = 0; a < 3; ++a) B.D[a] = hd[a];
    const MlmRoutePlan p = mlm_route_plan(B.D, hd[3], hd[5]);
    const int clearance = (int)hd[10], n_pen = (int)hd[11];
    if (!p.ok || !mlm_route_connectivity_ok((int)hd[6]) || n_pen < 0 || clearance < 0 || clearance + n_pen > 63) return 4;
    Rules r{};
    r.connectivity = (int)hd[6];
    r.max_cost = (uint32_t)hd[4];
    for (int k = 0; k < 3; ++k) r.move_cost[k] = (uint32_t)hd[7 + k];
    std::vector<int32_t> pens((size_t)n_pen), seeds((size_t)hd[5] * 3);
    std::vector<uint16_t> d_out((size_t)p.voxels);
    if (fread(pens.data(), 4, pens.size(), f) != pens.size() || fread(seeds.data(), 4, seeds.size(), f) != seeds.size() ||
        fread(d_out.data(), 2, d_out.size(), f) != d_out.size())
        return 3;
    fclose(f);
    for (int k = 0; k < n_pen; ++k) r.pen[k] = (uint32_t)pens[(size_t)k];
    std::vector<uint8_t> cls((size_t)p.voxels);
    B.field.resize((size_t)p.voxels);
    for (size_t j = 0; j < cls.size(); ++j) {
        cls[j] = mlm_route_class(d_out[j], clearance, n_pen);
        B.field[j] = (int)cls[j] > n_pen ? MLM_REACH_BLOCKED : MLM_REACH_FAR;
    }
    std::vector<uint8_t> dirty[2] = {std::vector<uint8_t>((size_t)p.tiles, 0), std::vector<uint8_t>((size_t)p.tiles, 0)};
    for (long long i = 0; i < hd[5]; ++i) {
        const long long x = seeds[(size_t)(3 * i)], y = seeds[(size_t)(3 * i + 1)], z = seeds[(size_t)(3 * i + 2)];
        if (B.at(x, y, z) == MLM_REACH_BLOCKED) continue;
        B.field[(size_t)((z * B.D[1] + y) * B.D[0] + x)] = 0;
        // a seed is a lowered voxel: its own tile is dirty, and so is every tile whose halo holds it
        const long long t[3] = {x / p.T[0], y / p.T[1], z / p.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)std::min(p.T[a], B.D[a] - t[a] * p.T[a]);
        dirty[0][(size_t)((t[2] * p.n[1] + t[1]) * p.n[0] + t[0])] = 1;
        const uint32_t m =
            mlm_route_dirty_mask(mlm_reach_faces((int)(x - t[0] * p.T[0]), (int)(y - t[1] * p.T[1]), (int)(z - t[2] * p.T[2]), td), r.connectivity);
        for (int k = 0; k < 27; ++k) {
            const long long nt = ((m >> k) & 1u) ? mlm_route_tile_at(t[0], t[1], t[2], p.n, k) : -1;
            if (nt >= 0) dirty[0][(size_t)nt] = 1;
        }
    }
    long long sweeps = 0;
    for (bool marked = true; marked; ++sweeps) {
        if (sweeps >= p.cap) return 5; // the schedule did not stop by itself
        marked = false;
        std::vector<uint8_t> &cur = dirty[sweeps & 1], &next = dirty[(sweeps & 1) ^ 1];
        for (long long t = 0; t < p.tiles; ++t) {
            if (!cur[(size_t)t]) continue;
            cur[(size_t)t] = 0;
            marked |= sweep_tile(B, cls, p, t, r, next);
        }
    }
    std::vector<int32_t> cost((size_t)p.voxels);
    std::vector<uint8_t> parent((size_t)p.voxels);
    long long out[6] = {0, 0, -1, sweeps, p.cap, p.tiles};
    for (long long z = 0; z < B.D[2]; ++z)
        for (long long y = 0; y < B.D[1]; ++y)
            for (long long x = 0; x < B.D[0]; ++x) {
                const size_t j = (size_t)((z * B.D[1] + y) * B.D[0] + x);
                const uint32_t v = B.field[j];
                cost[j] = mlm_route_cost(v);
                parent[j] = mlm_route_parent(v, mlm_route_pen(r.pen, cls[j]), r.move_cost, r.connectivity,
                                             [&](int dx, int dy, int dz) { return B.at(x + dx, y + dy, z + dz); });
                out[0] += v != MLM_REACH_BLOCKED;
                out[1] += v < MLM_REACH_FAR;
                if (v < MLM_REACH_FAR && (long long)v > out[2]) out[2] = v;
            }
    f = fopen(out_path, "wb");
    if (!f) return 3;
    fwrite(out, 8, 6, f);
    fwrite(cost.data(), 4, cost.size(), f);
    fwrite(parent.data(), 1, parent.size(), f);
    fwrite(cls.data(), 1, cls.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "run")) return run_mode(argv[2], argv[3]);
    return 2;
}
