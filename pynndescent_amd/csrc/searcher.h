// searcher.h -- the searcher's state (nnd_searcher_t of include/pynnd_amd.h) and the error macros of the files that work on it:
// searcher.hip (lifetime, fill, quantization), searcher_filter.hip (allow set, tag words) and query.hip (the walk and its entries).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "metric.h"
#include "devmem.h"
#include "../../include/pynnd_amd.h"

struct nnd_searcher_s {
    int device = 0;
    int64_t n = 0, nnz = 0, n_nodes = 0;
    int d = 0, dp = 0, metric = 0, n_neighbors = 0;
    float min_distance = 0.0f;
    uint32_t seed = 0;
    float *x = nullptr;        // (n, dp) rows padded to a multiple of 4 floats
    float *xn2 = nullptr;      // (n) squared norms (cosine; the prepared rows' for the codes 2..5)
    uint8_t *codes = nullptr;  // quantization="uint8": (n, dcs) codes, rows padded to 16 bytes with code 0
    float *cn2 = nullptr;      // (n) sum of LUT[c]^2 over a code row (cosine / dot)
    float *lut = nullptr;      // 512: the walk's codebook (256, padded with the last value), then the search table (+inf padded)
    int dcs = 0;               // code row stride: d rounded up to 16
    float tab_host[512];       // the host side of `lut` (the source of its stream-ordered upload)
    int32_t *indptr = nullptr, *indices = nullptr;
    float *hyper = nullptr, *offsets = nullptr;  // (n_nodes, dp), (n_nodes)
    int32_t *children = nullptr, *tree_idx = nullptr;
    hipStream_t stream = nullptr;
    int64_t last_spilled = 0;  // queries of the last call that ran on the global-memory tier
    bool force_big = false;    // nnd_searcher_set_tier(1): every query on the global-memory tier (tests)
    uint32_t *allow = nullptr;            // the filter's bitset over the searcher's numbering, (n + 31) / 32 words (allocated on first use)
    unsigned long long *fstat = nullptr;  // 2: allowed rows of the last filter, its out-of-range flag
    bool filter_on = false;               // nnd_searcher_set_filter*: the query entries run the filtered instances
    uint64_t *tags = nullptr;             // nnd_searcher_set_tags*: (n) tag words in the searcher's numbering (the tagged query entries)
    nnd_devmem mem;            // owner of the device buffers above (devmem.h)
    char err[512] = {0};
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
    }
};

// what a call without a searcher leaves for nnd_searcher_last_error(nullptr) (searcher.hip); shared by the three files, not exported
extern thread_local char g_serr[512] __attribute__((visibility("hidden")));

#define S_HIP(expr)                                                                                 \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            s->set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)
#define S_ALLOC(p, count)                                                                      \
    do {                                                                                       \
        if (!s->mem.alloc(p, count)) {                                                         \
            s->set_error("out of device memory: %s, %zu elements (%s:%d)", #p, (size_t)(count), __FILE__, __LINE__); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
