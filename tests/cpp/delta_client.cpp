// delta_client.cpp — a C++ client of the facade's deltaBlocks member (include/mlmap_facade.hpp), compiled by tests/test_delta_plan.py:
// a dry count that sizes the outputs, then the call that writes the new table, the emitted blocks and the gone keys.
#include <cstdint>
#include <vector>

#include "mlmap_facade.hpp"

int64_t what_changed(mlmap_hip::mlmap &map, std::vector<int32_t> &table_keys, std::vector<uint64_t> &table_digest, size_t cells) {
    int64_t summary[MLM_DELTA_ROW] = {};
    const int n_prev = (int)(table_keys.size() / 3);
    map.deltaBlocks(nullptr, nullptr, n_prev, table_keys.data(), table_digest.data(), MLM_DELTA_DRY, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                    nullptr, summary);
    const int S = (int)summary[1], E = (int)(summary[5] + summary[6]), G = (int)summary[7];
    std::vector<int32_t> cur_keys(3 * (size_t)S), keys(3 * (size_t)E), gone(3 * (size_t)G);
    std::vector<uint64_t> cur_digest(2 * (size_t)S);
    std::vector<float> log_odds((size_t)E * cells);
    std::vector<uint8_t> occ((size_t)E * cells), infl((size_t)E * cells), kind((size_t)E);
    map.deltaBlocks(nullptr, nullptr, n_prev, table_keys.data(), table_digest.data(), MLM_DELTA_NO_INFL, S, cur_keys.data(), cur_digest.data(), E, keys.data(),
                    log_odds.data(), occ.data(), infl.data(), kind.data(), G, gone.data(), summary);
    table_keys.swap(cur_keys), table_digest.swap(cur_digest);
    return summary[8] + summary[10];
}
