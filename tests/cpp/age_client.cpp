// age_client.cpp — a C++ client of the facade's ageBlocks member (include/mlmap_facade.hpp), compiled by tests/test_age_plan.py:
// a dry count, the aging of everything outside a key box with per-block counts, and the call with every default.
#include <cstdint>
#include <vector>

#include "mlmap_facade.hpp"

int64_t forget_behind(mlmap_hip::mlmap &map, const int32_t key_lo[3], const int32_t key_dims[3], int blocks) {
    int64_t summary[MLM_AGE_ROW] = {};
    map.ageBlocks(key_lo, key_dims, MLM_AGE_SCALE, 0.9f, 0.1f, MLM_AGE_OUTSIDE | MLM_AGE_FORGET | MLM_AGE_DROP | MLM_AGE_DRY, nullptr, summary);
    const int64_t would_drop = summary[2];
    std::vector<int32_t> per_block((size_t)blocks * MLM_AGE_COLS);
    map.ageBlocks(key_lo, key_dims, MLM_AGE_STEP, 0.05f, 0.1f, MLM_AGE_OUTSIDE | MLM_AGE_FORGET | MLM_AGE_DROP | MLM_AGE_CLEAR_INFL, per_block.data(), summary);
    map.ageBlocks();
    return would_drop + summary[6] + (blocks ? per_block[3] : 0);
}
