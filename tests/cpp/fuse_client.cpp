// fuse_client.cpp — a C++ client of the facade's fuseBlocks member (include/mlmap_facade.hpp), compiled by tests/test_fuse_plan.py:
// a diff, then the fuse with per-row counts.
#include <cstdint>
#include <vector>

#include "mlmap_facade.hpp"

int64_t page_in(mlmap_hip::mlmap &map, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl) {
    int64_t summary[MLM_FUSE_ROW] = {};
    map.fuseBlocks(n, keys, log_odds, occ, nullptr, MLM_FUSE_ADD, MLM_FUSE_DRY, nullptr, summary);
    const int64_t conflicts = summary[7];
    std::vector<int32_t> per_row((size_t)n * MLM_FUSE_COLS);
    map.fuseBlocks(n, keys, log_odds, occ, infl, MLM_FUSE_FILL, 0, per_row.data(), summary);
    map.fuseBlocks(n, keys, log_odds, occ);
    return conflicts + summary[2] + per_row[3];
}
