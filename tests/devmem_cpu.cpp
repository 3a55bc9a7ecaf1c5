// devmem_cpu.cpp -- the ownership policy of pynndescent_amd/csrc/devmem.h on a CPU (driven by test_devmem_cpu.py): the header is
// compiled with a counting allocator in place of the device's, under AddressSanitizer.  `devmem_cpu <case>` exits 0 when the
// case holds; a failed CHECK prints its line and exits 1; a double free is ASan's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

static std::vector<std::pair<void *, int>> g_blocks;  // every block ever handed out, and the times it was given back
static int g_live = 0, g_calls = 0, g_fail_at = 0;  // g_fail_at = N: the N-th allocation from now fails (0: none)

static bool fake_alloc(void **p, size_t bytes) {
    g_calls++;
    if (g_fail_at > 0 && --g_fail_at == 0) return false;
    *p = malloc(bytes);
    g_blocks.push_back({*p, 0});
    g_live++;
    return true;
}
static void fake_free(void *p) {
    for (size_t i = g_blocks.size(); i-- > 0;)  // (the latest life of an address malloc may have handed out twice)
        if (g_blocks[i].first == p) { g_blocks[i].second++; break; }
    g_live--;
    free(p);  // a second free of the same block is an ASan report
}
#define NND_DEVMEM_ALLOC(pp, bytes) fake_alloc((pp), (bytes))
#define NND_DEVMEM_FREE(p) fake_free(p)
#include "devmem.h"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static bool each_freed_once() {
    for (const auto &b : g_blocks)
        if (b.second != 1) return false;
    return true;
}
static int times_freed(const void *p) {  // of the first block at that address
    for (const auto &b : g_blocks)
        if (b.first == p) return b.second;
    return -1;
}

struct err_sink {
    std::string msg;
    void set_error(const char *fmt, ...) { msg = fmt; }
};

static void alloc_release() {
    nnd_devmem m;
    int32_t *a = nullptr;
    float *b = nullptr;
    uint8_t *c = nullptr;
    CHECK(m.alloc(&a, 10) && m.alloc(&b, 0) && m.alloc(&c, 3));  // (a count of 0 allocates one element)
    CHECK(a && b && c && g_live == 3);
    b[0] = 1.0f;  // ASan: the one element is there
    m.release_all();
    CHECK(g_live == 0 && g_blocks.size() == 3 && each_freed_once());
    m.release_all();  // no-op
    CHECK(g_live == 0 && each_freed_once());
}

static void grow_noop() {
    nnd_devmem m;
    int32_t *p = nullptr;
    int64_t cap = 0;
    CHECK(m.grow(&p, &cap, (int64_t)8, (int64_t)10) && cap == 10);
    int32_t *before = p;
    const int calls = g_calls;
    CHECK(m.grow(&p, &cap, (int64_t)10, (int64_t)99) && m.grow(&p, &cap, (int64_t)1, (int64_t)99));
    CHECK(g_calls == calls && p == before && cap == 10);
    float *q = nullptr;
    CHECK(m.grow2(&p, &q, &cap, (int64_t)10, (int64_t)99) && g_calls == calls && !q);
}

static void grow_success() {
    nnd_devmem m;
    int32_t *p = nullptr;
    size_t cap = 0;
    CHECK(m.grow(&p, &cap, (size_t)4, (size_t)5) && cap == 5);
    void *old = p;
    CHECK(m.grow(&p, &cap, (size_t)6, (size_t)7) && cap == 7 && p);
    p[6] = 1;  // ASan: new_cap elements are there
    CHECK(times_freed(old) == 1 && g_live == 1 && m.bases.size() == 1);
    m.release_all();
    CHECK(g_live == 0 && each_freed_once());
}

static void grow_fail_single() {
    nnd_devmem m;
    int32_t *p = nullptr;
    int64_t cap = 0;
    CHECK(m.grow(&p, &cap, (int64_t)4, (int64_t)4));
    g_fail_at = 1;
    CHECK(!m.grow(&p, &cap, (int64_t)8, (int64_t)10));
    CHECK(p == nullptr && cap == 0 && m.bases.empty() && g_live == 0);
    CHECK(m.grow(&p, &cap, (int64_t)8, (int64_t)10));  // the next call tries again
    CHECK(p && cap == 10 && g_live == 1 && m.bases.size() == 1);
}

static void grow2_fail(int which) {
    nnd_devmem m;
    int32_t *p = nullptr;
    uint64_t *q = nullptr;
    int64_t cap = 0;
    CHECK(m.grow2(&p, &q, &cap, (int64_t)4, (int64_t)4) && p && q && cap == 4 && g_live == 2);
    g_fail_at = which;
    CHECK(!m.grow2(&p, &q, &cap, (int64_t)8, (int64_t)10));
    CHECK(p == nullptr && q == nullptr && cap == 0 && g_live == 0 && m.bases.empty());
    CHECK(m.grow2(&p, (size_t)3, &q, (size_t)20, &cap, (int64_t)8, (int64_t)10) && p && q && cap == 10 && g_live == 2);
    q[19] = 1;  // ASan: the explicit counts are honoured
}

static void free_then_release() {
    nnd_devmem m;
    int32_t *a = nullptr, *b = nullptr;
    const float *c = nullptr;
    CHECK(m.alloc(&a, 4) && m.alloc(&b, 4) && m.alloc(&c, 4));
    m.free(&b);
    CHECK(b == nullptr && g_live == 2 && m.bases.size() == 2);
    m.free(&b);  // a null pointer: nothing to do
    m.free(&c);  // (a pointer to const: the handle's copy of the rows)
    CHECK(c == nullptr && g_live == 1);
    m.release_all();
    CHECK(g_live == 0 && each_freed_once());
}

static void biased() {
    nnd_devmem m;
    uint64_t *base = nullptr;
    CHECK(m.alloc(&base, 64));
    void *const allocated = base;
    uint64_t *work = base - 1000;  // what a shard's kernels index by global vertex id
    base = nullptr;
    (void)work;
    m.release_all();
    CHECK(g_live == 0 && times_freed(allocated) == 1);
}

static int scratch_scope(err_sink *e) {
    nnd_scratch tmp;
    int32_t *a = tmp.get<int32_t>(e, 4), *b = tmp.get<int32_t>(e, 0);
    float *c = tmp.get<float>(e, 16);
    CHECK(a && b && c && g_live == 3 && e->msg.empty());
    if (c) return 1;  // an early return out of the scope
    return 0;
}
static void scratch() {
    err_sink e;
    CHECK(scratch_scope(&e) == 1);
    CHECK(g_live == 0 && g_blocks.size() == 3 && each_freed_once());
    {
        nnd_scratch tmp;
        int32_t *a = tmp.get<int32_t>(&e, 4), *b = tmp.get<int32_t>(&e, 4);
        g_fail_at = 1;
        float *c = tmp.get<float>(&e, 4);
        CHECK(a && b && !c && !e.msg.empty());
        CHECK(g_live == 2 && tmp.bases.size() == 2);  // the earlier ones stay owned
    }
    CHECK(g_live == 0 && each_freed_once());
}

int main(int argc, char **argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "alloc_release") alloc_release();
    else if (c == "grow_noop") grow_noop();
    else if (c == "grow_success") grow_success();
    else if (c == "grow_fail_single") grow_fail_single();
    else if (c == "grow2_fail_first") grow2_fail(1);
    else if (c == "grow2_fail_second") grow2_fail(2);
    else if (c == "free_then_release") free_then_release();
    else if (c == "biased") biased();
    else if (c == "scratch") scratch();
    else {
        fprintf(stderr, "unknown case '%s'\n", c.c_str());
        return 2;
    }
    CHECK(g_live == 0);  // every owner of the case has gone out of scope
    printf("ok %s\n", c.c_str());
    return 0;
}
