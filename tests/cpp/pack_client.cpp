// pack_client.cpp — a C++ client of the facade's packBlocks / unpackBlocks members (include/mlmap_facade.hpp), compiled by
// tests/test_pack_plan.py: a dry call that sizes the stream, the call that writes it, and the stream turned back into rows.
#include <cstdint>
#include <vector>

#include "mlmap_facade.hpp"

std::vector<uint8_t> whole_map(mlmap_hip::mlmap &map) {
    int64_t summary[MLM_PACK_ROW] = {};
    map.packBlocks(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, MLM_PACK_DRY, 0, nullptr, summary);
    std::vector<uint8_t> stream((size_t)summary[1]);
    map.packBlocks(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, MLM_PACK_NO_INFL, stream.size(), stream.data(), summary);
    return stream;
}

int64_t rows_of(mlmap_hip::mlmap &map, const std::vector<uint8_t> &stream, size_t cells, std::vector<int32_t> &keys, std::vector<float> &log_odds, std::vector<uint8_t> &occ) {
    int64_t summary[MLM_PACK_ROW] = {};
    map.unpackBlocks(stream.data(), stream.size(), 0, 0, nullptr, nullptr, nullptr, nullptr, summary);
    const size_t n = (size_t)summary[0];
    keys.resize(3 * n), log_odds.resize(n * cells), occ.resize(n * cells);
    map.unpackBlocks(stream.data(), stream.size(), 0, (int)n, keys.data(), log_odds.data(), occ.data(), nullptr, summary);
    return summary[7];
}
