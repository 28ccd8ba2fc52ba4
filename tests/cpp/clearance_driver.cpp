// Test driver for mlm_query_clearance on the host: the rule of mlmapping_amd/csrc/mlm_clearance.h (the control flow the kernels
// k_clearance / k_clearance_groups and the entry point's host branch run too) — built by tests/test_clearance_plan.py with
// g++ -fsanitize=address,undefined (no HIP, no GPU).  Input blob: d_sub f64; n, n_groups (-1: no groups), sq_stop, sq_cap, flags i32;
// lo[3], dims[3] i32; p0, p1 [n*3] f64; group_begin [n_groups + 1] i32; sqdist [dims2*dims1*dims0] i32.  The field is copied into an
// allocation of exactly its size, so a read beside it is reported.  Output file: status [n] i8, voxel3 [n*3] i32, t [n] f64, n_steps,
// min_sq [n] i32, min3 [n*3] i32, cost [n] i64, n_near [n] i32, table [n_groups*8] i64 — of the walk without look-ahead; the walk with
// a look-ahead of 2, 4 and 5 must give the same bytes (exit status 4 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlm_clearance.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }

struct Out {
    std::vector<int8_t> status;
    std::vector<int32_t> voxel, n_steps, min_sq, min3, n_near;
    std::vector<double> t;
    std::vector<int64_t> cost, table;
};

template <int K> static void run(const std::vector<double> &p0, const std::vector<double> &p1, int n, double d, const MlmClearField &F,
                                 const std::vector<int32_t> &gb, int ng, Out &o) {
    const size_t N = (size_t)n;
    o.status.assign(N, 0), o.voxel.assign(3 * N, 0), o.n_steps.assign(N, 0), o.min_sq.assign(N, 0), o.min3.assign(3 * N, 0);
    o.n_near.assign(N, 0), o.t.assign(N, 0.0), o.cost.assign(N, 0), o.table.assign(ng > 0 ? (size_t)ng * MLM_CLEAR_WORDS : 0, -7);
    for (int i = 0; i < n; ++i) {
        MlmClearResult r;
        mlm_clear_walk<K>(&p0[3 * (size_t)i], &p1[3 * (size_t)i], d, F, r);
        o.status[i] = (int8_t)r.status;
        o.t[i] = r.t;
        o.n_steps[i] = r.n_steps, o.min_sq[i] = r.min_sq, o.n_near[i] = r.n_near, o.cost[i] = (int64_t)r.cost;
        for (int a = 0; a < 3; ++a) o.voxel[3 * (size_t)i + a] = r.voxel[a], o.min3[3 * (size_t)i + a] = r.min3[a];
    }
    for (int g = 0; g < ng; ++g)
        mlm_clear_group(gb[(size_t)g], gb[(size_t)g + 1], o.status.data(), o.min_sq.data(), o.cost.data(), o.n_steps.data(), o.n_near.data(),
                        &o.table[(size_t)g * MLM_CLEAR_WORDS]);
}

static bool same(const Out &a, const Out &b) {
    return a.status == b.status && a.voxel == b.voxel && a.n_steps == b.n_steps && a.min_sq == b.min_sq && a.min3 == b.min3 && a.n_near == b.n_near &&
           a.cost == b.cost && a.table == b.table && a.t.size() == b.t.size() &&
           (a.t.empty() || std::memcmp(a.t.data(), b.t.data(), a.t.size() * sizeof(double)) == 0);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double d_sub;
    int32_t hdr[5], box[6]; // n, n_groups, sq_stop, sq_cap, flags; lo, dims
    if (!rd(f, &d_sub, 8) || !rd(f, hdr, sizeof hdr) || !rd(f, box, sizeof box)) return 2;
    const int n = hdr[0], ng = hdr[1];
    const size_t nvox = (size_t)box[3] * box[4] * box[5];
    std::vector<double> p0((size_t)n * 3), p1((size_t)n * 3);
    std::vector<int32_t> gb(ng >= 0 ? (size_t)ng + 1 : 0);
    int32_t *field = (int32_t *)std::malloc(nvox * sizeof(int32_t));
    if (!field || !rd(f, p0.data(), p0.size() * 8) || !rd(f, p1.data(), p1.size() * 8) || !rd(f, gb.data(), gb.size() * 4) || !rd(f, field, nvox * 4))
        return 2;
    std::fclose(f);
    MlmClearField F{};
    F.sqdist = field;
    for (int a = 0; a < 3; ++a) F.lo[a] = box[a], F.dims[a] = box[3 + a];
    F.sq_stop = hdr[2], F.sq_cap = hdr[3], F.outside_pass = hdr[4] & 1;
    Out o1, o2, o4, o5;
    run<1>(p0, p1, n, d_sub, F, gb, ng, o1);
    run<2>(p0, p1, n, d_sub, F, gb, ng, o2);
    run<4>(p0, p1, n, d_sub, F, gb, ng, o4);
    run<5>(p0, p1, n, d_sub, F, gb, ng, o5);
    std::free(field);
    if (!same(o1, o2) || !same(o1, o4) || !same(o1, o5)) return 4;
    FILE *g = std::fopen(argv[2], "wb");
    if (!g) return 2;
    const size_t N = (size_t)n;
    const bool ok = wr(g, o1.status.data(), N) && wr(g, o1.voxel.data(), 12 * N) && wr(g, o1.t.data(), 8 * N) && wr(g, o1.n_steps.data(), 4 * N) &&
                    wr(g, o1.min_sq.data(), 4 * N) && wr(g, o1.min3.data(), 12 * N) && wr(g, o1.cost.data(), 8 * N) && wr(g, o1.n_near.data(), 4 * N) &&
                    wr(g, o1.table.data(), 8 * o1.table.size());
    return std::fclose(g) == 0 && ok ? 0 : 2;
}
