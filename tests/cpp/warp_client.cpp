// warp_client.cpp — a C++ client of the facade's warpBlocks member (include/mlmap_facade.hpp), compiled by tests/test_warp_plan.py:
// a sizing call, the call into host arrays, the replacing call.
#include <cstdint>
#include <vector>

#include "mlmap_facade.hpp"

int64_t reanchor(mlmap_hip::mlmap &map, const double T_sd[12], int cells) {
    int64_t summary[MLM_WARP_ROW] = {};
    map.warpBlocks(T_sd, nullptr, nullptr, MLM_WARP_DRY, 0, nullptr, nullptr, nullptr, nullptr, summary);
    const int cap = (int)summary[2];
    std::vector<int32_t> keys((size_t)cap * 3);
    std::vector<float> log_odds((size_t)cap * cells);
    std::vector<uint8_t> occ((size_t)cap * cells), infl((size_t)cap * cells);
    map.warpBlocks(T_sd, nullptr, nullptr, MLM_WARP_SEEN, cap, keys.data(), log_odds.data(), occ.data(), infl.data(), summary);
    map.warpBlocks(T_sd, nullptr, nullptr, MLM_WARP_REPLACE);
    return summary[3];
}
