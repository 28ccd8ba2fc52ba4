// mlm_kernels_score.h — scan-to-map scores of candidate poses (mlm_score_poses; no reference counterpart: the reference takes its pose
// from an external odometry; the rule — transform, lattice, classes, field cost, the eight counters — is mlm_score.h's, which the host
// code and the CPU test run too).
//
// k_score<CLASSES, FIELD>: one lane per pose.  Workgroup (x, y) of the grid takes point chunk x and the MLM_BLOCK consecutive poses
// from y * MLM_BLOCK on; a lane keeps its pose's 12 doubles, its eight counters and the block of its previous point in registers.
// The chunk's points pass through LDS in tiles of MLM_SCORE_TILE (one coalesced load per workgroup); in the inner loop every lane
// reads the same point, an LDS broadcast.  There is no cross-lane reduction: a pose's row is the sum of its lane's counters over the
// chunks.  With one chunk a lane writes its row with plain stores; with more the host zeroes the rows first and every lane adds its
// non-zero words with atomicAdd — integer adds, so the row has one value whatever the order.  Consecutive lanes are consecutive
// poses: a correlative grid with x fastest gathers from neighbouring voxels of the field and of the class planes.  A lane probes
// the block table again only when its point leaves the block of its previous one (MlmRayClasses, mlm_kernels_rays.h); an absent or
// released block reads no class byte.  The field-only instantiation touches nothing of the map.
#pragma once
#include "mlm_kernels_rays.h"
#include "mlm_score.h"

#define MLM_SCORE_TILE 128 // points per LDS tile (3 KB); a chunk is a whole number of tiles

struct MlmScore {
    const double *pts; // [n_pts * 3], sensor frame
    const double *T;   // [n_poses * 12]
    int n_pts, n_poses;
    int chunk;         // points per chunk, a multiple of MLM_SCORE_TILE; gridDim.x chunks cover n_pts
    int atomic;        // more than one chunk: the rows are zeroed, add
    MlmScoreField F;
    unsigned long long *table; // [n_poses * 8]
};

template <bool CLASSES, bool FIELD> __global__ __launch_bounds__(MLM_BLOCK) void k_score(const MlmDev P, const MlmScore Q) {
    __shared__ double s_pts[MLM_SCORE_TILE * 3];
    const int k = (int)(blockIdx.y * MLM_BLOCK + threadIdx.x);
    const bool live = k < Q.n_poses;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = live ? Q.T[12 * (size_t)k + i] : 0.0;
    unsigned long long acc[MLM_SCORE_WORDS];
#pragma unroll
    for (int i = 0; i < MLM_SCORE_WORDS; ++i) acc[i] = 0;
    MlmScoreBlock B{};
    MlmRayClasses cls{P, -1, 4, true};
    MlmScoreNoClasses none;
    const long long p0 = (long long)blockIdx.x * Q.chunk;
    const int p1 = (int)min((long long)Q.n_pts, p0 + Q.chunk); // (wave-uniform: every lane of the workgroup meets every barrier)
    for (int t0 = (int)p0; t0 < p1; t0 += MLM_SCORE_TILE) {
        const int m = min(MLM_SCORE_TILE, p1 - t0);
        __syncthreads(); // (the previous tile has been read)
        for (int i = threadIdx.x; i < 3 * m; i += MLM_BLOCK) s_pts[i] = Q.pts[3 * (size_t)t0 + i];
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; ++j) {
            const double s[3] = {s_pts[3 * j], s_pts[3 * j + 1], s_pts[3 * j + 2]};
            if (CLASSES)
                mlm_score_pair<CLASSES, FIELD>(T, s, P.d_sub, P.n, Q.F, cls, B, acc);
            else
                mlm_score_pair<CLASSES, FIELD>(T, s, P.d_sub, P.n, Q.F, none, B, acc);
        }
    }
    if (!live) return;
    unsigned long long *row = Q.table + (size_t)k * MLM_SCORE_WORDS;
    if (!Q.atomic) {
#pragma unroll
        for (int i = 0; i < MLM_SCORE_WORDS; ++i) row[i] = acc[i];
    } else {
#pragma unroll
        for (int i = 0; i < MLM_SCORE_WORDS; ++i)
            if (acc[i]) atomicAdd(row + i, acc[i]);
    }
}
