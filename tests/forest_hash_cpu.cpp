// Prints the counter hash of csrc/common.h and the seed derivation (nnd_seed_of, same header) for fixed arguments:
// tests/test_forest_reference_cpu.py pins the Python restatements (tests/search_reference.py, tests/forest_reference.py) to them.
// Host code only: nothing here touches a device.
#include <cstdio>

#include "common.h"

int main() {
    const uint32_t seeds[3] = {1u, 0x9E3779B9u, 0xFFFFFFFFu};
    const uint32_t as[4] = {0u, 1u, 131071u, 0xFFFFFFF0u};
    const uint32_t bs[3] = {0u, 7u, 401u};
    for (uint32_t s : seeds)
        for (uint32_t a : as) {
            printf("hash2 %u %u %u\n", s, a, nnd_hash2(s, a));
            for (uint32_t b : bs) printf("hash3 %u %u %u %u\n", s, a, b, nnd_hash3(s, a, b));
        }
    const int64_t states[3][3] = {{1, 2, 3}, {-2147483648LL, 2147483646LL, -1}, {1791095845LL, -12091157LL, 4282876139LL - 4294967296LL}};
    for (const auto &st : states) printf("seed %lld %lld %lld %u\n", (long long)st[0], (long long)st[1], (long long)st[2], nnd_seed_of(st));
    return 0;
}
