// devmem.h -- who owns device memory.  Every device allocation of the library belongs to exactly one nnd_devmem: the handle's
// (state.h), a shard's, a searcher's, a communicator's, or the nnd_scratch of one call.  The owner keeps the BASE pointers it
// allocated; the structs keep their plain working pointers (which may be biased), and releasing the owner frees every base
// exactly once -- no list of fields to keep in step.  The one rule of the grow-only buffers lives here too: a capacity is
// published after the allocation it describes has succeeded, so a failed growth leaves (nullptr, 0) and the next call tries again.
//
// Host-only C++: the two primitives come in as macros, so the policy is tested on a CPU with a counting allocator
// (tests/test_devmem_cpu.py).  The library binds them here, and nowhere else, to hipMalloc / hipFree.
#pragma once
#include <assert.h>
#include <stddef.h>

#include <vector>

#ifndef NND_DEVMEM_ALLOC
#include <hip/hip_runtime.h>
static inline bool nnd_devmem_hip_alloc(void **p, size_t bytes) {
    if (hipMalloc(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();  // an out-of-memory is reported by the caller, not left behind as the thread's last error
    *p = nullptr;
    return false;
}
#define NND_DEVMEM_ALLOC(pp, bytes) nnd_devmem_hip_alloc((pp), (bytes))  // bool: *pp holds `bytes` bytes
#define NND_DEVMEM_FREE(p) ((void)hipFree(p))
#endif

struct nnd_devmem {
    std::vector<void *> bases;  // searched linearly: about a hundred entries, nothing here is on a timed path
    nnd_devmem() = default;
    nnd_devmem(const nnd_devmem &) = delete;
    nnd_devmem &operator=(const nnd_devmem &) = delete;
    ~nnd_devmem() { release_all(); }

    // a new buffer of `count` elements (0: one element); false, and *p == nullptr, when there is no memory
    template <typename T>
    bool alloc(T **p, size_t count) {
        void *q = nullptr;
        *p = nullptr;
        if (!NND_DEVMEM_ALLOC(&q, sizeof(T) * (count ? count : 1))) return false;
        bases.push_back(q);
        *p = (T *)q;
        return true;
    }
    // give one buffer back; *p must be null or a base this owner allocated (never a biased pointer)
    template <typename T>
    void free(T **p) {
        if (*p) {
            size_t i = 0;
            while (i < bases.size() && bases[i] != (const void *)*p) i++;
            assert(i < bases.size() && "nnd_devmem::free: not a base of this owner");
            if (i < bases.size()) {
                NND_DEVMEM_FREE(bases[i]);
                bases[i] = bases.back();
                bases.pop_back();
            }
        }
        *p = nullptr;
    }
    void release_all() {
        for (void *q : bases) NND_DEVMEM_FREE(q);
        bases.clear();
    }

    // Grow-only buffer: nothing happens while need <= *cap; otherwise the old buffer goes, (*p, *cap) = (nullptr, 0), and
    // new_cap elements (the call site's own headroom) are allocated.  The caller waits for the buffer's last reader first.
    template <typename T, typename C>
    bool grow(T **p, C *cap, C need, C new_cap) {
        if (need <= *cap) return true;
        free(p);
        *cap = 0;
        if (!alloc(p, (size_t)new_cap)) return false;
        *cap = new_cap;
        return true;
    }
    // two buffers under one capacity: both allocations succeed, or neither buffer is kept
    template <typename T, typename U, typename C>
    bool grow2(T **p, U **q, C *cap, C need, C new_cap) {
        return grow2(p, (size_t)new_cap, q, (size_t)new_cap, cap, need, new_cap);
    }
    // ... of count_p / count_q elements where the two are not new_cap elements each
    template <typename T, typename U, typename C>
    bool grow2(T **p, size_t count_p, U **q, size_t count_q, C *cap, C need, C new_cap) {
        if (need <= *cap) return true;
        free(p);
        free(q);
        *cap = 0;
        if (!alloc(p, count_p)) return false;
        if (!alloc(q, count_q)) {
            free(p);
            return false;
        }
        *cap = new_cap;
        return true;
    }
};

// Temporary device buffers of one call: released on every return path (the caller drains its stream before it returns).
struct nnd_scratch : nnd_devmem {
    template <typename T, typename E>
    T *get(E *err, size_t count) {  // nullptr (and err->set_error) when there is no memory; what was handed out before stays owned
        T *p = nullptr;
        if (!alloc(&p, count)) err->set_error("allocation of %zu scratch bytes on the device failed", sizeof(T) * count);
        return p;
    }
};
