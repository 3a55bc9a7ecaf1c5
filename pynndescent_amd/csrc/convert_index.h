// convert_index.h -- how the typed-rows conversion (devarray.hip k_rows_to_f32) splits a flat run of `count` elements into work
// items: a scalar head up to the first element whose address is a multiple of the vector size, a body of whole vectors of `vec`
// elements (one aligned vector load each), a scalar tail.  A (rows, d) C-contiguous point set is one such run of rows * d
// elements: d need not be a multiple of anything, and a view that starts in the middle of an allocation only has a longer head.
//
// Host and device C++ with no dependency on HIP, so that the arithmetic is tested on a CPU under a sanitizer
// (tests/convert_index_cpu.cpp): every element belongs to exactly one item, no item leaves [0, count), every vector is aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NND_CONV_HD __host__ __device__
#else
#define NND_CONV_HD
#endif

struct nnd_conv_plan {
    int64_t head;  // scalar items [0, head): element i
    int64_t body;  // vector items: element head + v * vec .. + vec
    int64_t tail;  // scalar items: element head + body * vec + t
    int vec;       // elements per vector item
};

// src_addr: address of element 0; elem_size: bytes per element; vec: elements per vector load (a power of two)
NND_CONV_HD static inline nnd_conv_plan nnd_conv_make_plan(uint64_t src_addr, int elem_size, int vec, int64_t count) {
    nnd_conv_plan p;
    p.vec = vec;
    if (count < 0) count = 0;
    const uint64_t align = (uint64_t)elem_size * (uint64_t)vec;
    const uint64_t mis = src_addr % align;
    if (mis % (uint64_t)elem_size != 0) {  // elements that straddle every vector boundary: no vector item at all
        p.head = count;
        p.body = p.tail = 0;
        return p;
    }
    int64_t head = mis ? (int64_t)((align - mis) / (uint64_t)elem_size) : 0;
    if (head > count) head = count;
    p.head = head;
    p.body = (count - head) / vec;
    p.tail = count - head - p.body * vec;
    return p;
}

NND_CONV_HD static inline int64_t nnd_conv_items(const nnd_conv_plan &p) { return p.body + p.head + p.tail; }

// Item `i` of nnd_conv_items(p): vector items come first (the bulk of the grid is uniform), then the head's and the tail's
// scalars.  *first: its first element; returns how many elements it holds (vec or 1).
NND_CONV_HD static inline int nnd_conv_item(const nnd_conv_plan &p, int64_t i, int64_t *first) {
    if (i < p.body) {
        *first = p.head + i * p.vec;
        return p.vec;
    }
    const int64_t j = i - p.body;
    *first = j < p.head ? j : p.head + p.body * p.vec + (j - p.head);
    return 1;
}
