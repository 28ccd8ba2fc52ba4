// logit_inv_scan.cpp — the hard cases of getOdd's narrowing (include/mlmap.h:40): for EVERY float L in [LO, HI] the host value
// (float)(p / (1 + p)), p = pow(10.0, (double)L) with glibc's pow, and the list of the L whose double quotient lies within K double
// ulps of a float rounding midpoint.  Those are the only inputs where a pow that is a few ulps off (the device's) can round to a
// different float — ASSUMING that pow's error stays below K/4 ulps: p then moves by less than K/4 ulps, 1 + p by less than that,
// and their quotient by less than K ulps.  For each listed L: whether glibc's pow is correctly rounded there (libquadmath's powq,
// 113 bits, as the yardstick).
//
// usage: logit_inv_scan LO HI K
// prints one line per hard case, in increasing L:  "L_bits f_bits m cr"  (hex float bits of L and of the host's odds; m: the
// quotient's signed distance to the midpoint in double ulps; cr: 1 if glibc's pow is correctly rounded at L), then
// "# scanned N hard M threads T".  Threads: min(16, OMP_NUM_THREADS or the hardware's).
#include <quadmath.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace {

uint32_t bits_of(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
float float_of(uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

struct Hard {
    float L;
    float f;
    long m;
    int cr;
};

} // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s LO HI K\n", argv[0]);
        return 2;
    }
    const float lo = std::strtof(argv[1], nullptr), hi = std::strtof(argv[2], nullptr);
    const long K = std::strtol(argv[3], nullptr, 10);
    // (the odds must stay normal floats, >= 2^-126, for the midpoints to sit 2^28 double ulps above a float)
    if (!(lo <= hi) || lo < -37.0f || K < 0 || K >= (1l << 28)) {
        std::fprintf(stderr, "need -37 <= LO <= HI and 0 <= K < 2^28\n");
        return 2;
    }
    // the floats of [lo, hi] as ranges of bit patterns (negative floats: the pattern grows as the value falls)
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    if (hi < 0.0f) ranges.push_back({bits_of(hi), bits_of(lo)});
    else if (lo < 0.0f) ranges.push_back({0x80000000u, bits_of(lo)}), ranges.push_back({0u, bits_of(hi)});
    else ranges.push_back({bits_of(lo), bits_of(hi)});
    constexpr uint64_t kChunk = 1u << 20;
    std::vector<std::pair<uint64_t, uint64_t>> chunks; // [first, last] patterns
    uint64_t total = 0;
    for (const auto &r : ranges) {
        total += (uint64_t)r.second - r.first + 1;
        for (uint64_t a = r.first; a <= r.second; a += kChunk) chunks.push_back({a, std::min<uint64_t>(r.second, a + kChunk - 1)});
    }
    unsigned int T = std::thread::hardware_concurrency();
    if (const char *e = std::getenv("OMP_NUM_THREADS"))
        if (std::atoi(e) > 0) T = (unsigned int)std::atoi(e);
    T = std::max(1u, std::min(16u, T));

    std::atomic<size_t> next{0};
    std::mutex mu;
    std::vector<Hard> hard;
    auto work = [&]() {
        std::vector<Hard> mine;
        for (size_t c; (c = next.fetch_add(1)) < chunks.size();)
            for (uint64_t u = chunks[c].first; u <= chunks[c].second; ++u) {
                const float L = float_of((uint32_t)u);
                const double p = std::pow(10.0, (double)L);
                const double q = p / (1 + p);
                uint64_t qb;
                std::memcpy(&qb, &q, 8);
                // the low 29 bits of q's significand: 2^28 is a float rounding midpoint (q < 1, a normal float's binade)
                const long m = (long)(qb & ((1ull << 29) - 1)) - (1l << 28);
                if (std::labs(m) > K) continue;
                const int cr = (double)powq((__float128)10, (__float128)L) == p;
                mine.push_back({L, (float)q, m, cr});
            }
        std::lock_guard<std::mutex> g(mu);
        hard.insert(hard.end(), mine.begin(), mine.end());
    };
    std::vector<std::thread> pool;
    for (unsigned int t = 0; t < T; ++t) pool.emplace_back(work);
    for (auto &t : pool) t.join();
    std::sort(hard.begin(), hard.end(), [](const Hard &a, const Hard &b) { return a.L < b.L; });
    for (const Hard &h : hard) std::printf("%08x %08x %ld %d\n", bits_of(h.L), bits_of(h.f), h.m, h.cr);
    std::printf("# scanned %llu hard %zu threads %u\n", (unsigned long long)total, hard.size(), T);
    return 0;
}
