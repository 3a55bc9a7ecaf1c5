// csr_graph.h -- what csr_graph.hip shares with the other producers of an nnd_csr_t (fuzzy.hip, affinity.hip): the result's struct, the
// error sink of an entry without a handle, and the build of a CSR matrix from int32 k-lists that already lie on the device.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "devmem.h"
#include "state.h"

#define CSR_REG_CAP 256  // the widest k-list

struct nnd_csr_s {
    nnd_devmem mem;  // one block: the three arrays below are pieces of it
    int device = 0;
    int64_t m = 0, nnz = 0, long_rows = 0;
    int64_t *indptr = nullptr;
    int32_t *indices = nullptr;
    float *data = nullptr;
};

struct csr_err {  // the error sink of an entry without a handle: what nnd_last_global_error returns
    char msg[256];
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        nnd_set_global_error(msg);
    }
};
#define CSR_HIP(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            (void)hipGetLastError();                                                                        \
            err.set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);       \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

// How the symmetric form joins an entry and its twin: the smaller float (the graph export), or UMAP's fuzzy union of two
// membership strengths, mix * (a + b - a * b) + (1 - mix) * (a * b), a lone entry mix * a, and no entry where that is 0; or
// (sum, affinity.hip) the sum of the two times a scale, (a + b) * scale, a lone entry a * scale, and no entry where that is 0.
struct csr_combine {
    int fuzzy = 0;
    float mix = 1.0f;
    int sum = 0;
    float scale = 1.0f;
};
enum { CSR_RULE_MIN = 0, CSR_RULE_FUZZY = 1, CSR_RULE_SUM = 2 };  // the merge kernels' template argument

// The kernels of one export of the int32 k-lists ids / vals (device, row stride ld) on `st`; the result's arrays are allocated
// in g->mem, the scratch in tmp.  The stream is drained where a total has to reach the host; the caller drains it once more
// before the scratch goes.
int csr_build_i32(csr_err &err, nnd_scratch &tmp, hipStream_t st, nnd_csr_s *g, const int32_t *ids, const float *vals, int64_t m, int32_t k,
                  int64_t ld, int64_t n, int symmetric, csr_combine combine);
