// MlmBktMod (mlm_host.h): the two 32-bit forms k_sector takes a hit's bucket with — `code % n` for the sign-extended 32-bit hash code of
// VectorHasher and the emulated container's bucket count n — against unsigned __int128 arithmetic.
//   exhaustive: divisors 2, 3, 4 294 967 291 and 20 753 (where a config-2 stream's container settles), all 2^32 hash values each.  The
//               expected remainder is seeded with a 128-bit remainder at the start of every run of 2^16 consecutive codes, kept by
//               counting inside the run (consecutive codes, consecutive remainders: no division in the loop) and checked against a
//               128-bit remainder again at the run's end.
//   primes:     every bucket count libstdc++'s rehash policy can choose below 2^32 (its prime list, walked with _M_next_bkt): 2^16
//               strided hash values plus 0, +-1, INT_MIN and INT_MAX, each against a 128-bit remainder; and 2^64 mod n itself.
//   fall-back:  the list's first entry of 2^32 or more, 2^32 itself and 0 must not select the fast forms.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "mlm_host.h"

using namespace mlm_host;
typedef unsigned __int128 u128;

static inline unsigned long long code_of(uint32_t h) { return (unsigned long long)(long long)(int32_t)h; } // (mlm_hash_rpz's return)
static inline uint32_t ref_of(uint32_t h, unsigned long long n) { return (uint32_t)((u128)code_of(h) % (u128)n); }

static unsigned long long exhaustive(unsigned long long n, unsigned int n_threads) {
    const MlmBktMod B = bkt_mod(n);
    std::vector<unsigned long long> bad(n_threads, 0ull);
    std::vector<std::thread> pool;
    for (unsigned int t = 0; t < n_threads; ++t)
        pool.emplace_back([&, t]() {
            unsigned long long b = 0;
            for (uint32_t run = t; run < (1u << 16); run += n_threads) { // (a run never crosses the step from INT_MAX to INT_MIN)
                const uint32_t h0 = run << 16;
                uint32_t r = ref_of(h0, n);
                for (uint32_t i = 0; i < (1u << 16); ++i) {
                    b += mlm_bucket_fast(code_of(h0 + i), B) != r;
                    r = r + 1u == (uint32_t)n ? 0u : r + 1u;
                }
                b += r != (uint32_t)((u128)(ref_of(h0 + 0xFFFFu, n) + 1ull) % (u128)n); // (the count arrived where 128-bit arithmetic puts it)
            }
            bad[t] = b;
        });
    for (auto &th : pool) th.join();
    unsigned long long s = 0;
    for (auto b : bad) s += b;
    return s;
}

int main() {
    unsigned int n_threads = std::thread::hardware_concurrency();
    n_threads = n_threads < 1u ? 1u : (n_threads > 16u ? 16u : n_threads);
    unsigned long long checked = 0, bad = 0;
    for (unsigned long long n : {2ull, 3ull, 4294967291ull, 20753ull}) {
        if (!bkt_mod(n).fast) {
            std::printf("no fast form for %llu\n", n);
            return 1;
        }
        bad += exhaustive(n, n_threads);
        checked += 1ull << 32;
    }
    // libstdc++'s prime list below 2^32
    std::__detail::_Prime_rehash_policy pol;
    unsigned long long primes = 0, p_checked = 0, p_bad = 0, c_bad = 0, first_big = 0;
    for (size_t p = pol._M_next_bkt(2);; p = pol._M_next_bkt(p + 1)) {
        if (p >= (1ull << 32)) {
            first_big = p;
            break;
        }
        ++primes;
        const MlmBktMod B = bkt_mod(p);
        if (!B.fast) {
            std::printf("no fast form for %zu\n", p);
            return 1;
        }
        c_bad += B.c != (uint32_t)(((u128)1 << 64) % (u128)p);
        const uint32_t edge[5] = {0u, 1u, 0xFFFFFFFFu, (uint32_t)INT_MIN, (uint32_t)INT_MAX};
        for (uint32_t i = 0; i < (1u << 16) + 5u; ++i) {
            const uint32_t h = i < (1u << 16) ? (i << 16) | ((i * 40503u) & 0xFFFFu) : edge[i - (1u << 16)];
            p_bad += mlm_bucket_fast(code_of(h), B) != ref_of(h, p);
            ++p_checked;
        }
    }
    const int fallback = (bkt_mod(first_big).fast == 0u) + (bkt_mod(1ull << 32).fast == 0u) + (bkt_mod(0ull).fast == 0u);
    // (one bucket: every code lands in bucket 0 — the multiplier wraps to 0)
    const int one = bkt_mod(1).fast == 1u && mlm_bucket_fast(code_of(0x80000000u), bkt_mod(1)) == 0u && mlm_bucket_fast(code_of(12345u), bkt_mod(1)) == 0u;
    std::printf("checked %llu bad %llu primes %llu prime_checked %llu prime_bad %llu c_bad %llu fallback %d one %d first_big %llu\n", checked, bad, primes, p_checked,
                p_bad, c_bad, fallback, one, first_big);
    return 0;
}
