// mst.h -- what mst.hip shares with cross.hip (the spanning tree: the forest's components joined by cross-component searches):
// the state of the Boruvka rounds, the forest's rounds as one call that leaves that state on the device, and the launch of the
// round kernels that do not care where a row's record came from (k_mst_pick, k_mst_hook, k_mst_jump, k_mst_flatten).  The
// kernels themselves stay in mst.hip: one translation unit compiles them, so both users run the same code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "csr_graph.h"

#define MST_EMPTY 0xFFFFFFFFFFFFFFFFull  // no key: above every (w, lo)
#define MST_NO_KEY 0xFFFFFFFFu           // the distance bits of a place that does not count; no hi
#define MST_FAULT 0x80000000u            // in a round's hook counter: a device loop met its bound, or a key was not whole

struct mst_state {
    int64_t m;
    int32_t cols;                // the columns of edge_ids / edge_w: one per round
    int32_t *comp, *comp_next;   // the component (a root's id) of every point
    int32_t *parent;             // of a root: itself, or the root it hooked to
    unsigned long long *best1;   // per root: the smallest (w bits << 32 | lo) of its rows
    uint32_t *best2;             // ... and the smallest hi among the rows that hold it
    unsigned long long *rec1;    // per row: its own smallest key
    uint32_t *rec2;
    unsigned char *dead;         // the row has no edge that leaves its component
    int32_t *edge_ids;           // (m, cols): the forest edge row i won in a round, -1
    float *edge_w;
    unsigned int *hooks;         // [cols + 1]: the hooks of a round, MST_FAULT
    int32_t *smallest;           // per root: its smallest member
    int32_t *flag, *pos;         // 1 at a smallest member; the exclusive sums
};

static inline size_t mst_room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct mst_carve {
    unsigned char *base = nullptr;
    size_t at = 0;
    template <typename T>
    T *take(size_t count) {
        T *p = (T *)(base + at);
        at += mst_room(sizeof(T) * (count ? count : 1));
        return p;
    }
};
static inline unsigned mst_grid(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}
static inline int mst_ceil_log2(int64_t m) {
    int r = 0;
    while (((int64_t)1 << r) < m) r++;
    return r;
}

// the forest's working memory: the state, and the room of the prefix sum over s.flag (both users number rows with it)
struct mst_work {
    mst_state s;
    unsigned char *scan_tmp = nullptr;
    size_t scan_bytes = 0;
};

int mst_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld_ids,
              int64_t ld_dists, int32_t min_samples, const int32_t *labels, const float *core);
// core distances, weights, the min-union `sym` and the forest's rounds (m > 0); afterwards w.s.comp holds every point's root,
// columns [0, *rounds) of w.s.edge_ids / edge_w the forest, every row is dead and every best1 / best2 is empty
int mst_forest_rounds(csr_err &err, nnd_scratch &tmp, nnd_csr_s &sym, hipStream_t st, const void *ids, int32_t id_bytes, const float *dists, int64_t m,
                      int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples, float *core, mst_work &w, int *rounds);
// a round's second half for rows whose records (rec1, rec2, dead) and components' best1 are written: the pick of hi, the hooks
// into column `round` and the counter s.hooks[round], the pointer jumping, the new components (s.comp and s.comp_next swapped)
void mst_launch_join(hipStream_t st, mst_state &s, int32_t round);
