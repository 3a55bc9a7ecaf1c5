// Prints the counter hash of csrc/common.h for the arguments of a few pruning coins, the word that stands for (entry, compared
// entry) in that hash (nnd_prune_coin_word, same header), and how many different words the pairs below NND_WIDE_K give:
// tests/test_prune_reference_cpu.py pins tests/prune_reference.py to them.  Host code only: nothing here touches a device.
#include <cstdio>
#include <vector>

#include "common.h"

int main() {
    const uint32_t seeds[3] = {77u, 77u ^ 0x51ED270Bu, 0xFFFFFFFFu};
    const uint32_t rows[3] = {0u, 1201u, 36001u};
    const uint32_t pairs[5][2] = {{1u, 0u}, {14u, 13u}, {63u, 62u}, {64u, 0u}, {255u, 254u}};
    for (uint32_t s : seeds)
        for (uint32_t r : rows)
            for (const auto &p : pairs) {
                const uint32_t w = nnd_prune_coin_word(p[0], p[1]);
                printf("coin %u %u %u %u %u %u\n", s, r, p[0], p[1], w, nnd_hash3(s, r, w));
            }
    std::vector<unsigned char> seen((size_t)NND_WIDE_K * NND_WIDE_K * 4, 0);
    unsigned distinct = 0;
    for (uint32_t a = 0; a < NND_WIDE_K; a++)
        for (uint32_t b = 0; b < NND_WIDE_K; b++) {
            const uint32_t w = nnd_prune_coin_word(a, b);
            if (w < seen.size() && !seen[w]) { seen[w] = 1; distinct++; }
        }
    printf("distinct %u of %u\n", distinct, (unsigned)(NND_WIDE_K * NND_WIDE_K));
    return 0;
}
