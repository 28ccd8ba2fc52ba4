// mlm_path.h — the rule of mlm_query_paths (include/mlmap_hip.h): the trace along the parent codes of mlm_export_reach /
// mlm_export_route, the integer visibility test, the shortening loop, the table words and the length sum, once, in plain integer
// C++, for the kernel (mlm_kernels_path.h), the host branch of the entry point and the CPU test driver (tests/cpp/path_driver.cpp),
// so that all three run the very same control flow.  No reference counterpart: the reference has no cost field and no path query;
// the move codes and their offsets are mlm_route.h's (mlm_route_offset; the first six are mlm_reach.h's).
//
// Nothing here trusts the field: a voxel is OPEN iff it lies in the box and its byte is <= M (M = 6 for a reach field, 26 for a route
// field; M itself is a seed), every step is taken only onto an open voxel of the box, the trace ends after max_moves moves, a
// visibility walk ends after at most n_x + n_y + n_z <= 3 * lookahead steps, and the shortening always accepts the next path voxel.
//
// The path of one goal lives in a scratch of three int32 arrays of max_moves + 1 entries (x, y, z of u_0 .. u_K, relative to the
// box: no linear indices, so nobody divides); who writes it and who tests which candidates is the executor's business:
//   X.put(k, x, y, z)        record u_k (called for k = 0, 1, .. in order)
//   X.sync(K)                u_0 .. u_K are complete: make them readable through X.at
//   X.at(k, v)               read u_k
//   X.pick(F, i, hi)         the largest j in (i + 1, hi] with vis(u_i, u_j), or i + 1 if there is none (hi >= i + 1)
//   X.uni(v)                 v, which has the same value in every thread of the executor, marked as such
//   X.leader()               does this thread write results?
// MlmPathSerial below is the plain one (one thread, candidates from the far end down); the kernel's runs a wave per goal.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mlm_route.h"

#ifdef __HIPCC__
#define MLM_PATH_NOUNROLL _Pragma("nounroll")
#else
#define MLM_PATH_NOUNROLL
#endif
#define MLM_PATH_KIND_REACH 0
#define MLM_PATH_KIND_ROUTE 1
#define MLM_PATH_WORDS 8              // words of a table row (MLM_PATH_ROW)
#define MLM_PATH_MAX_LOOKAHEAD 4096   // so every factor of a crossing comparison is at most 2 * 4096 + 1 < 2^14 and a product fits an int
#define MLM_PATH_MAX_MOVES (1 << 20)

// the field of a call: the bytes of the box [D[2]][D[1]][D[0]] and the seed code M
struct MlmPathField {
    const uint8_t *parent;
    int32_t D[3];
    int M;
};

MLM_RE_HD int mlm_path_seed_code(int kind) { return kind == MLM_PATH_KIND_REACH ? 6 : MLM_ROUTE_CODES; }
MLM_RE_HD bool mlm_path_inside(const MlmPathField &F, long long x, long long y, long long z) {
    return x >= 0 && x < F.D[0] && y >= 0 && y < F.D[1] && z >= 0 && z < F.D[2];
}
// the byte of a voxel inside the box
MLM_RE_HD int mlm_path_code(const MlmPathField &F, int x, int y, int z) {
    return F.parent[((size_t)z * (size_t)F.D[1] + (size_t)y) * (size_t)F.D[0] + (size_t)x];
}
MLM_RE_HD bool mlm_path_open(const MlmPathField &F, int x, int y, int z) {
    return mlm_path_inside(F, x, y, z) && mlm_path_code(F, x, y, z) <= F.M;
}

// vis(a, b) for open voxels a, b with |b - a| <= MLM_PATH_MAX_LOOKAHEAD per axis: the walk from a to b over the crossings
// (2 k + 1) / (2 n) of each axis in ascending order; at a tie of the axes T every voxel c + (a non-empty subset of T's steps) must be
// open.  `ties` (optional): bit 0 / 1 set if a tie group of two / of three axes occurred before the answer was known.
MLM_RE_HD bool mlm_path_vis(const MlmPathField &F, const int a[3], const int b[3], int *ties = nullptr) {
    int n[3], s[3], k[3] = {0, 0, 0}, c[3];
    MLM_ROUTE_UNROLL
    for (int x = 0; x < 3; ++x) {
        const int d = b[x] - a[x];
        n[x] = d < 0 ? -d : d;
        s[x] = d > 0 ? 1 : d < 0 ? -1 : 0;
        c[x] = a[x];
    }
    while (k[0] < n[0] || k[1] < n[1] || k[2] < n[2]) {
        int best = -1, T = 0;
        MLM_ROUTE_UNROLL
        for (int x = 0; x < 3; ++x) {
            if (k[x] >= n[x]) continue;
            if (best < 0) {
                best = x;
                T = 1 << x;
                continue;
            }
            // (2 k_x + 1) / (2 n_x) against (2 k_best + 1) / (2 n_best), cross-multiplied
            const int l = (2 * k[x] + 1) * n[best], r = (2 * k[best] + 1) * n[x];
            if (l < r) {
                best = x;
                T = 1 << x;
            } else if (l == r)
                T |= 1 << x;
        }
        if (ties && (T & (T - 1))) *ties |= T == 7 ? 2 : 1;
        MLM_PATH_NOUNROLL
        for (int S = 1; S < 8; ++S) {
            if ((S & T) != S) continue;
            if (!mlm_path_open(F, c[0] + ((S & 1) ? s[0] : 0), c[1] + ((S & 2) ? s[1] : 0), c[2] + ((S & 4) ? s[2] : 0))) return false;
        }
        MLM_ROUTE_UNROLL
        for (int x = 0; x < 3; ++x)
            if (T >> x & 1) {
                c[x] += s[x];
                ++k[x];
            }
    }
    return true;
}

// one leg of the polyline: acc + d * sqrt(sq) as three IEEE double operations (the library is built without contraction)
MLM_RE_HD double mlm_path_add_leg(double acc, double d, const int a[3], const int b[3]) {
    long long sq = 0;
    MLM_ROUTE_UNROLL
    for (int x = 0; x < 3; ++x) sq += (long long)(b[x] - a[x]) * (b[x] - a[x]);
    const double root = sqrt((double)sq);
    const double leg = d * root;
    return acc + leg;
}

// where the results of one goal go; any pointer may be null
struct MlmPathOut {
    int8_t *status;    // this goal's
    int32_t *way3;     // this goal's [cap][3]
    double *length;    // this goal's
    int64_t *table;    // this goal's [MLM_PATH_WORDS]
};

// The whole contract for one goal.  goal: absolute voxel; lo: the box's first voxel; d = (double)(float)subbox_d_xyz.  Returns the
// status.  Every thread of an executor calls this with the same arguments; only X.leader() stores.
template <class Exec>
MLM_RE_HD int mlm_path_goal(const MlmPathField &F, const int32_t lo[3], const int32_t goal[3], int L, int max_moves, int cap, double d, Exec &X,
                            const MlmPathOut &o) {
    // the table words: K, W, face / edge / corner moves, the longest leg, the candidates beyond the chosen ones
    int K = 0, W = 0, faces = 0, edges = 0, corners = 0, longest = 0;
    long long beyond = 0;
    double length = -1.0;
    int status = 0;
    const long long g[3] = {(long long)goal[0] - lo[0], (long long)goal[1] - lo[1], (long long)goal[2] - lo[2]};
    if (mlm_path_inside(F, g[0], g[1], g[2]) && mlm_path_code(F, (int)g[0], (int)g[1], (int)g[2]) <= F.M) {
        // ---- trace
        int u[3] = {(int)g[0], (int)g[1], (int)g[2]};
        int c = X.uni(mlm_path_code(F, u[0], u[1], u[2])); // (the byte of u_K: every voxel's is read once)
        for (;;) {
            X.put(K, u[0], u[1], u[2]);
            if (c == F.M) {
                status = 1;
                break;
            }
            if (K == max_moves) {
                status = -1;
                break;
            }
            int dx, dy, dz;
            mlm_route_offset(c, dx, dy, dz);
            const int v[3] = {u[0] + dx, u[1] + dy, u[2] + dz};
            const int cv = mlm_path_inside(F, v[0], v[1], v[2]) ? X.uni(mlm_path_code(F, v[0], v[1], v[2])) : 255;
            if (cv > F.M) {
                status = -2;
                break;
            }
            const int kind = mlm_route_kind(c);
            faces += kind == 0, edges += kind == 1, corners += kind == 2;
            u[0] = v[0], u[1] = v[1], u[2] = v[2];
            c = cv;
            ++K;
        }
        if (status == 1) {
            X.sync(K);
            // ---- shortening
            int i = 0, a[3];
            W = 1;
            double acc = 0.0;
            X.at(0, a);
            const bool lead = X.leader();
            if (lead && o.way3 && cap > 0) {
                MLM_ROUTE_UNROLL
                for (int x = 0; x < 3; ++x) o.way3[x] = a[x] + lo[x];
            }
            while (i < K) {
                const int hi = K - i < L ? K : i + L;
                const int j = X.pick(F, i, hi);
                int b[3];
                X.at(j, b);
                acc = mlm_path_add_leg(acc, d, a, b);
                beyond += hi - j;
                longest = j - i > longest ? j - i : longest;
                if (lead && o.way3 && W < cap) {
                    MLM_ROUTE_UNROLL
                    for (int x = 0; x < 3; ++x) o.way3[3 * (size_t)W + x] = b[x] + lo[x];
                }
                ++W;
                i = j;
                MLM_ROUTE_UNROLL
                for (int x = 0; x < 3; ++x) a[x] = b[x];
            }
            length = acc;
        }
    }
    if (status != 1) faces = edges = corners = 0; // (counted along the way; reported for a whole path only)
    if (X.leader()) {
        if (o.status) *o.status = (int8_t)status;
        if (o.length) *o.length = length;
        if (o.table) {
            MLM_ROUTE_UNROLL
            for (int w = 0; w < MLM_PATH_WORDS; ++w)
                o.table[w] = w == 0 ? K : w == 1 ? W : w == 2 ? faces : w == 3 ? edges : w == 4 ? corners : w == 5 ? longest : w == 6 ? beyond : 0;
        }
    }
    return status;
}

// the plain executor: one thread, the path in three arrays of at least max_moves + 1 entries each, candidates from the far end down
struct MlmPathSerial {
    int32_t *px, *py, *pz;
    MLM_RE_HD void put(int k, int x, int y, int z) { px[k] = x, py[k] = y, pz[k] = z; }
    MLM_RE_HD void sync(int) {}
    MLM_RE_HD void at(int k, int v[3]) const { v[0] = px[k], v[1] = py[k], v[2] = pz[k]; }
    MLM_RE_HD int uni(int v) const { return v; }
    MLM_RE_HD bool leader() const { return true; }
    MLM_RE_HD int pick(const MlmPathField &F, int i, int hi) const {
        int a[3], b[3];
        at(i, a);
        for (int j = hi; j > i + 1; --j) {
            at(j, b);
            if (mlm_path_vis(F, a, b)) return j;
        }
        return i + 1;
    }
};
