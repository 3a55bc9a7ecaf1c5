// The index arithmetic of the typed-rows conversion (pynndescent_amd/csrc/convert_index.h) on a CPU, under a sanitizer: for
// every (rows, d, element size, vector width, misalignment of the source) of a sweep the work items are walked exactly as the
// kernel walks them, against a source and a destination buffer of exactly rows * d elements (so that an item that leaves the
// run is an out-of-bounds access the sanitizer reports), and it is checked that every element is written exactly once, that
// every vector item starts on a multiple of the vector size, and that scalar items are fewer than two vectors' worth.
// Usage: convert_index_cpu            prints "plans P elements E bad B", exit status 0 when B == 0
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "convert_index.h"

static long long g_bad = 0, g_plans = 0, g_elements = 0;

static void fail(const char *what, long long rows, int d, int es, int vec, int mis) {
    if (g_bad++ < 10) fprintf(stderr, "FAIL %s: rows %lld d %d elem_size %d vec %d misalignment %d\n", what, rows, d, es, vec, mis);
}

// elem_size bytes per source element, vec elements per vector, the source starting `mis` bytes past a 64-byte boundary
static void one_case(long long rows, int d, int es, int vec, int mis) {
    const int64_t count = rows * (int64_t)d;
    // exact-size heap blocks: the run ends where the block ends, and the sanitizer knows the bounds
    unsigned char *block = (unsigned char *)malloc((size_t)count * es + 1);
    float *dst = (float *)malloc(sizeof(float) * (size_t)count + 4);
    unsigned char *hits = (unsigned char *)calloc((size_t)count + 1, 1);
    for (int64_t i = 0; i < count * es; i++) block[i] = (unsigned char)(i * 31 + 7);
    const uint64_t addr = ((uint64_t)1 << 20) + (uint64_t)mis;  // the device address the plan is made for
    const nnd_conv_plan p = nnd_conv_make_plan(addr, es, vec, count);
    g_plans++;
    if (p.head < 0 || p.body < 0 || p.tail < 0 || p.head + p.body * vec + p.tail != count) fail("the parts do not add up", rows, d, es, vec, mis);
    if (mis % es == 0 && (p.head >= vec || p.tail >= vec) && p.body > 0) fail("a scalar part of a whole vector or more", rows, d, es, vec, mis);
    const int64_t items = nnd_conv_items(p);
    for (int64_t i = 0; i < items; i++) {
        int64_t first = -1;
        const int len = nnd_conv_item(p, i, &first);
        if (len != 1 && len != vec) fail("item length", rows, d, es, vec, mis);
        if (len == vec && (addr + (uint64_t)first * es) % ((uint64_t)es * vec) != 0) fail("a vector item is not aligned", rows, d, es, vec, mis);
        for (int c = 0; c < len; c++) {
            const int64_t e = first + c;
            unsigned char tmp[8];
            memcpy(tmp, block + e * es, (size_t)es);  // the read the kernel makes (out of the run: the sanitizer stops here)
            dst[e] = (float)tmp[0];
            hits[e]++;
        }
    }
    for (int64_t e = 0; e < count; e++)
        if (hits[e] != 1) { fail("an element is written zero or several times", rows, d, es, vec, mis); break; }
    for (int64_t e = 0; e < count; e++)
        if (dst[e] != (float)block[e * es]) { fail("an element landed in the wrong place", rows, d, es, vec, mis); break; }
    g_elements += count;
    free(block);
    free(dst);
    free(hits);
}

int main() {
    const long long rows_set[] = {0, 1, 2, 3, 7, 64, 257, 2001};
    const int d_set[] = {1, 2, 3, 5, 7, 8, 16, 23, 24, 31, 33, 128, 130};
    const struct { int es, vec; } types[] = {{2, 8}, {8, 4}, {4, 4}};  // float16 / bfloat16, float64, float32
    for (long long rows : rows_set)
        for (int d : d_set)
            for (auto t : types)
                for (int mis = 0; mis < 64; mis += (rows > 300 ? 6 : 1)) one_case(rows, d, t.es, t.vec, mis);
    // a count beyond 2^31 elements: the arithmetic alone (no buffers)
    {
        const int64_t count = ((int64_t)1 << 33) + 8;  // head 5, tail 3
        const nnd_conv_plan p = nnd_conv_make_plan(4096 + 6, 2, 8, count);
        int64_t first = -1;
        const int64_t items = nnd_conv_items(p);
        if (p.head != 5 || p.tail != 3 || p.head + p.body * 8 + p.tail != count) fail("large count: parts", count, 1, 2, 8, 6);
        if (nnd_conv_item(p, p.body - 1, &first) != 8 || first != p.head + (p.body - 1) * 8) fail("large count: last vector", count, 1, 2, 8, 6);
        if (nnd_conv_item(p, items - 1, &first) != 1 || first != count - 1) fail("large count: last item", count, 1, 2, 8, 6);
        g_plans++;
    }
    printf("plans %lld elements %lld bad %lld\n", g_plans, g_elements, g_bad);
    return g_bad ? 1 : 0;
}
