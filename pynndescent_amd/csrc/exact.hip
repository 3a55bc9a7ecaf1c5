// exact.hip -- exact k nearest neighbours by brute force: the companion of the approximate index (ground truth, recall).
//
// Two tiers, and a certificate that decides per row which one answers (DESIGN.md "Exact search"):
//   k_exact_scan    streams the whole prepared point set past blocks of 64 query rows: f32 MFMA Gram tiles (gram.h), the
//                   alt-space distance of every pair (metric.h nnd_gram_to_dist), the W >= k smallest kept per row by the leaf kernel's
//                   pattern (screen against the row's W-th distance, ballot + compact into an LDS queue, rank merge of a full
//                   queue, merge.h).  It also keeps T, the smallest distance it did NOT keep.
//   k_exact_merge   folds the partial lists when the point set was split over gridDim.y slices.
//   k_exact_refine  recomputes the W candidates' distances from the ORIGINAL rows with float64 accumulation (metric.h
//                   nnd_ref_acc / nnd_ref_dist, every term in float64), sorts by (float64 distance, id), keeps k -- and certifies the row iff the k-th exact distance
//                   lies below T by more than the rounding-error band of the scan (exact_band.h): then nothing that was left
//                   out can belong to the top k.
//   k_exact_f64     the definition: all n original rows in float64, for exactly the rows that were not certified.
// An f32 Gram ranking alone is NOT exact: on two far modes of tight points (|x| ~ 1e3, spread 1e-2) it misses a true neighbour
// in every row however many candidates are refined; there the band exceeds every gap and the float64 tier answers.
#include "common.h"
#include "metric.h"
#include "state.h"
#include "gram.h"
#include "merge.h"
#include "exact_band.h"

#define EX_QB 64   // query rows per workgroup: 16 per wave
#define EX_TB 64   // data rows per tile: four 16x16 accumulator tiles per wave (the B operands of a wave are reused by its 16 rows)
#define EX_PC 24   // queue entries per query row; a queue is merged before a tile of 16 columns could overflow it (24: two workgroups per CU at DC = 128)
#define EX_BATCH 131072  // query rows per pass of the host driver (bounds the workspace)

// Make this wave's global writes (the rows of the partial lists) visible to its own later reads, lane to lane.  Workgroup scope:
// the wave's loads and stores go through the same L1, so this is a wait, not a cache operation (an agent-scope fence here
// writes back and invalidates L2 lines per merge: measured 4x slower on small sets).  Other workgroups read the lists in a
// later kernel only.
__device__ __forceinline__ void ex_global_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Merge ncand candidates into the sorted row (row_e, row_d) of W keys with the rank merges of merge.h.  newth: the row's W-th
// distance afterwards (+inf while the row is not full); dropped: the smallest distance that did NOT stay in the row (an entry
// pushed out, a candidate that did not get in), +inf if none -- the scan's T is the minimum over all of these.
template <bool WIDE, int NCH, typename CandFn>
__device__ __forceinline__ void ex_merge_into(uint64_t *scr, uint32_t *__restrict__ row_e, float *__restrict__ row_d, float *__restrict__ th_slot,
                                              int W, int ncand, CandFn cand, float &newth, float &dropped) {
    constexpr int U = WIDE ? NND_WIDE_U : 1;
    const int lane = nnd_lane();
    uint32_t oe[U];
    float od[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int j = lane + 64 * u;
        oe[u] = j < W ? row_e[j] : NND_EMPTY_E;
        od[u] = j < W ? row_d[j] : INFINITY;
    }
    const float th_old = row_d[W - 1];  // the merges take a candidate only if it is strictly below this
    if constexpr (WIDE) nnd_merge_row_lds<NCH>(scr, row_e, row_d, th_slot, W, ncand, cand);
    else nnd_merge_row_regs<NCH>(row_e, row_d, th_slot, oe[0], od[0], W, ncand, cand);
    ex_global_sync();
    const uint32_t we = row_e[W - 1];
    newth = row_d[W - 1];
    dropped = INFINITY;
    if (we != NND_EMPTY_E) {  // a full row: whatever sorts behind its last key, or was refused, is out
        const uint64_t wk = nnd_make_key(newth, we);
#pragma unroll
        for (int u = 0; u < U; u++)
            if (oe[u] != NND_EMPTY_E && nnd_make_key(od[u], oe[u]) > wk) dropped = fminf(dropped, od[u]);
        for (int c = lane; c < ncand; c += 64) {
            uint32_t id = 0;
            float dc = 0.0f;
            if (!cand(c, id, dc)) continue;
            if (!(dc < th_old) || nnd_make_key(dc, id) > wk) dropped = fminf(dropped, dc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dropped = fminf(dropped, __shfl_xor(dropped, o, 64));
    }
}

// ---- tier 1: the scan ----
// Workgroup (bx, by): query rows [64 bx, 64 bx + 64) against data rows [c_lo, c_hi) of slice by.  Wave w owns query rows
// 16 w .. 16 w + 15: lane l holds, per accumulator tile J, the Gram values of rows 4 (l >> 4) + r, r = 0..3, and column
// 16 J + (l & 15) -- so the threshold th[r], the reject minimum rej[r] and the queue fill fill[r] of those four rows live in
// registers, the same in all 16 lanes of a group.  DC: floats of a row staged per K chunk (dp <= DC: the query rows are staged
// once); WIDE: W > 64 (rows merged through LDS).
// FAM: the metric family (metric.h) -- NND_CODES_01, NND_CODES_0_5 (the codes 2..5; code 6 is refused by the host) or
// NND_CODES_BOOL (the boolean family: `metric` carries the column count, metric.h nnd_kernel_metric).
// MK: the masked scan: data row c is part of query row i's point set only if tags[c] & qmasks[i] != 0 -- `tags` one word per
// data row, `qmasks` one per query row of the batch; the other instances never read either.  The masks of a lane group's four
// rows live in registers beside th and rej, the tags of a data tile are staged beside snrm.  A pair that does not meet is neither
// admitted nor counted into rej: it is no rejected candidate, and the certificate's T must not see it.
// The three kernels of this file (k_exact_scan, k_exact_refine, k_exact_f64) are each one template around an inlined body: with
// the body in the __global__ function itself the compiler emits other code (DESIGN.md "The search kernels").
template <int DC, int FAM, bool WIDE, bool MK>
__device__ __forceinline__ void ex_scan_body(const float *__restrict__ xp, const float *__restrict__ nrm, int64_t n, int dp, int metric,
                                                    const float *__restrict__ qx, const float *__restrict__ qnrm, const int32_t *__restrict__ qids,
                                                    int self, int nq, int nq_pad, int W, int64_t rows_per_slice, uint32_t *__restrict__ list_e,
                                                    float *__restrict__ list_d, float *__restrict__ list_th, float *__restrict__ list_rej,
                                                    const uint64_t *__restrict__ tags /* MK: (n) */, const uint64_t *__restrict__ qmasks /* MK: (nq) */) {
    extern __shared__ __align__(16) unsigned char ex_smem[];
    float *Xs = (float *)ex_smem;                              // (EX_QB + EX_TB) rows of DC floats, swizzled: queries, then the data tile
    float *snrm = Xs + (EX_QB + EX_TB) * DC;                   // (EX_TB) nrm of the data tile
    uint64_t *stag = (uint64_t *)(snrm + EX_TB);               // MK: (EX_TB) tag words of the data tile (the other instances have no such array)
    int32_t *sq = (int32_t *)(snrm + EX_TB + (MK ? 2 * EX_TB : 0));  // (EX_QB) ids of the query rows, -1 = none
    uint2 *pend = (uint2 *)(sq + EX_QB);                       // (EX_QB, EX_PC) queues: (id, distance bits)
    uint64_t *wscr = (uint64_t *)(pend + EX_QB * EX_PC);       // WIDE: NND_WIDE_SCRATCH_WORDS per wave
    const int tid = threadIdx.x, lane = nnd_lane(), w = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int q0 = blockIdx.x * EX_QB;
    const int64_t c_lo = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t c_hi = c_lo + rows_per_slice < n ? c_lo + rows_per_slice : n;
    const size_t lbase = (size_t)blockIdx.y * nq_pad + q0 + 16 * w;  // first of this wave's 16 list rows
    if (tid < EX_QB) sq[tid] = q0 + tid < nq ? qids[q0 + tid] : -1;
    for (int idx = lane; idx < 16 * W; idx += 64) {
        list_e[lbase * W + idx] = NND_EMPTY_E;
        list_d[lbase * W + idx] = INFINITY;
    }
    if (lane < 16) list_th[lbase + lane] = INFINITY;
    ex_global_sync();
    __syncthreads();
    const bool multi = dp > DC;
    if (!multi) nnd_stage_rows<DC>(qx, dp, sq, EX_QB, 0, dp, Xs, tid, 256);
    float na[4], th[4], rej[4];
    int sid[4], fill[4];
    bool qok[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int id = sq[16 * w + 4 * g + r];
        qok[r] = id >= 0;
        na[r] = qok[r] ? qnrm[id] : 0.0f;
        sid[r] = (self && qok[r]) ? id : -2;
        th[r] = rej[r] = INFINITY;
        fill[r] = 0;
    }
    uint64_t qm[4] = {0ull, 0ull, 0ull, 0ull};
    if constexpr (MK) {
#pragma unroll
        for (int r = 0; r < 4; r++) qm[r] = qok[r] ? qmasks[q0 + 16 * w + 4 * g + r] : 0ull;
    }
    // merge the queues of this wave's rows into their lists
    auto flush = [&]() {
        nnd_wave_lds_sync();
#pragma unroll 1
        for (int rr = 0; rr < 16; rr++) {
            const int gq = rr >> 2, rq = rr & 3;
            const int f = rq == 0 ? fill[0] : rq == 1 ? fill[1] : rq == 2 ? fill[2] : fill[3];
            const int cnt = __builtin_amdgcn_readlane(f, 16 * gq);
            if (cnt == 0) continue;  // wave-uniform
            const size_t row = lbase + rr;
            const uint2 *pq = pend + (16 * w + rr) * EX_PC;
            float newth, dropped;
            ex_merge_into<WIDE, 1>(wscr + w * NND_WIDE_SCRATCH_WORDS, list_e + row * W, list_d + row * W, list_th + row, W, cnt,
                                   [&](int c, uint32_t &id, float &dc) {
                                       const uint2 s = pq[c];
                                       id = s.x;
                                       dc = __uint_as_float(s.y);
                                       return true;
                                   },
                                   newth, dropped);
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (g == gq && r == rq) {
                    th[r] = newth;
                    rej[r] = fminf(rej[r], dropped);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) fill[r] = 0;
        nnd_wave_lds_sync();  // the queues are read: the next tile may overwrite them
    };
    for (int64_t t0 = c_lo; t0 < c_hi; t0 += EX_TB) {
        f32x4 acc[4];
#pragma unroll
        for (int J = 0; J < 4; J++) acc[J] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < dp; c0 += DC) {
            const int cw = dp - c0 < DC ? dp - c0 : DC;
            __syncthreads();  // the operand reads of the previous chunk / tile are done
            if (multi) nnd_stage_rows<DC>(qx, dp, sq, EX_QB, c0, cw, Xs, tid, 256);
            const int nch = cw >> 2, total = EX_TB * nch;
#pragma unroll 4
            for (int idx = tid; idx < total; idx += 256) {
                const int r = idx / nch, ch = idx - r * nch;
                const int64_t row = t0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < c_hi) v = *(const float4 *)(xp + row * dp + c0 + 4 * ch);
                *(float4 *)&Xs[nnd_swz<DC>(EX_QB + r, ch)] = v;
            }
            if (c0 == 0 && tid < EX_TB) snrm[tid] = t0 + tid < c_hi ? nrm[t0 + tid] : 0.0f;
            if constexpr (MK) {
                if (c0 == 0 && tid < EX_TB) stag[tid] = t0 + tid < c_hi ? tags[t0 + tid] : 0ull;
            }
            __syncthreads();
            nnd_gram_chunk<DC, 4>(Xs, 16 * w, EX_QB, cw, acc, [](int) { return true; });
        }
#pragma unroll 1
        for (int J = 0; J < 4; J++) {
            const f32x4 a = J == 0 ? acc[0] : J == 1 ? acc[1] : J == 2 ? acc[2] : acc[3];
            const int col = 16 * J + c16;
            const int64_t cid = t0 + col;
            const bool cv = cid < c_hi;
            const float nb = snrm[col];
            uint64_t tg = 0ull;
            if constexpr (MK) tg = stag[col];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float val = nnd_gram_to_dist<FAM>(metric, a[r], na[r], nb);
                if ((int64_t)sid[r] == cid) val = nnd_self_dist<FAM>(metric, na[r]);
                bool in_set = cv;  // MK: and the pair's words meet
                if constexpr (MK) in_set = cv && (tg & qm[r]) != 0ull;
                const bool ok = in_set && qok[r] && val < th[r];
                if (in_set && !ok) rej[r] = fminf(rej[r], val);
                const uint32_t m16 = (uint32_t)(__ballot(ok) >> (16 * g)) & 0xFFFFu;
                if (ok) pend[(16 * w + 4 * g + r) * EX_PC + fill[r] + __popc(m16 & ((1u << c16) - 1u))] = make_uint2((uint32_t)cid, __float_as_uint(val));
                fill[r] += __popc(m16);
            }
            if (__ballot(fill[0] > EX_PC - 16 || fill[1] > EX_PC - 16 || fill[2] > EX_PC - 16 || fill[3] > EX_PC - 16)) flush();
        }
    }
    if (__ballot((fill[0] | fill[1] | fill[2] | fill[3]) != 0)) flush();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float v = rej[r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
        if (c16 == 0) list_rej[lbase + 4 * g + r] = v;
    }
}
template <int DC, int FAM, bool WIDE, bool MK>
__global__ __launch_bounds__(256) void k_exact_scan(const float *__restrict__ xp, const float *__restrict__ nrm, int64_t n, int dp, int metric,
                                                    const float *__restrict__ qx, const float *__restrict__ qnrm, const int32_t *__restrict__ qids,
                                                    int self, int nq, int nq_pad, int W, int64_t rows_per_slice, uint32_t *__restrict__ list_e,
                                                    float *__restrict__ list_d, float *__restrict__ list_th, float *__restrict__ list_rej,
                                                    const uint64_t *__restrict__ tags /* MK: (n) */, const uint64_t *__restrict__ qmasks /* MK: (nq) */) {
    ex_scan_body<DC, FAM, WIDE, MK>(xp, nrm, n, dp, metric, qx, qnrm, qids, self, nq, nq_pad, W, rows_per_slice, list_e, list_d, list_th, list_rej, tags, qmasks);
}

// ---- the slices' lists folded into slice 0's, one wave per query row ----
template <bool WIDE>
__global__ __launch_bounds__(256) void k_exact_merge(int nq, int nq_pad, int W, int n_slices, uint32_t *__restrict__ list_e, float *__restrict__ list_d,
                                                     float *__restrict__ list_th, float *__restrict__ list_rej) {
    __shared__ uint64_t scr[WIDE ? 4 * NND_WIDE_SCRATCH_WORDS : 1];
    const int lane = nnd_lane(), w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= nq) return;
    float t = list_rej[q];
    for (int s = 1; s < n_slices; s++) {
        const size_t src = (size_t)s * nq_pad + q;
        const uint32_t *se = list_e + src * W;
        const float *sd = list_d + src * W;
        float newth, dropped;
        ex_merge_into<WIDE, WIDE ? 4 : 1>(scr + (WIDE ? w * NND_WIDE_SCRATCH_WORDS : 0), list_e + (size_t)q * W, list_d + (size_t)q * W, list_th + q, W, W,
                                          [&](int c, uint32_t &id, float &dc) {
                                              const uint32_t e = se[c];
                                              id = e & NND_IDX_MASK;
                                              dc = sd[c];
                                              return e != NND_EMPTY_E;
                                          },
                                          newth, dropped);
        t = fminf(t, fminf(dropped, list_rej[src]));
    }
    if (lane == 0) list_rej[q] = t;
}

// ---- float64 distances of the original rows: the reference's formulas of metric.h, hellinger's terms in float64 too ----
struct ex_val {
    double r;   // alt-space distance, not yet rounded to float32 (FLT_MAX for the reference's "no similarity" cases)
    double g;   // the value the scan's Gram value approximates (codes 1, 5: cosine / coefficient; 2, 3: <a, b>), -inf if none
    double ax;  // codes 1..5: the query row's squared norm term
};
// the 16 lanes of a group on one pair; mua: the query row's mean (correlation)
// FAM: NND_CODES_01, NND_CODES_0_5 (the codes 2..5) or NND_CODES_BOOL (the counts, then the float64 twin on them and d)
template <int FAM>
__device__ __forceinline__ ex_val ex_pair_f64(int metric, const float *__restrict__ xa, const float *__restrict__ xb, int d, int l16, double mua) {
    constexpr bool XM = FAM != NND_CODES_01;
    double dot = 0.0, nx = 0.0, ny = 0.0;
    const double ma = XM ? mua : 0.0, mb = XM && metric == 4 ? nnd_row_mean_f64<16>(xb, d, l16) : 0.0;
    for (int t = l16; t < d; t += 16) nnd_ref_acc<FAM, NND_HELLINGER_F64>(metric, (double)xa[t] - ma, (double)xb[t] - mb, dot, nx, ny);
    const double dt = nnd_group_sum_f64<16>(dot);
    const double ax = metric == 0 ? 0.0 : nnd_group_sum_f64<16>(nx), ay = metric == 0 ? 0.0 : nnd_group_sum_f64<16>(ny);  // (code 0: dt is all)
    ex_val v;
    if constexpr (FAM == NND_CODES_BOOL) {  // certified in distance space (ex_certified): no Gram value
        v.r = nnd_ref_dist<NND_CODES_BOOL>(metric, dt, ax, ay, (double)d);
        v.g = -INFINITY;
        v.ax = ax;
        return v;
    }
    v.r = nnd_ref_dist<NND_CODES_0_5>(metric, dt, ax, ay);  // (both instances carry the whole conversion: XM splits the loop above only)
    v.g = -INFINITY;
    v.ax = ax;
    if (metric == 2 || metric == 3) {
        if (dt > 0.0) v.g = dt;
    } else if (metric != 4 && ax != 0.0 && ay != 0.0 && !(dt <= 0.0)) {  // cosine / hellinger: nnd_ref_dist's finite case
        v.g = dt / sqrt(ax * ay);
    }
    return v;
}

// Is the row's top k final?  rk / gk / ax: the k-th candidate's exact values; t: the smallest kernel distance the scan left
// out; na: the query's nrm word; nmax: the largest nrm of the point set (code 2: the largest |x|^2 of the raw rows).
template <int FAM>
__device__ __forceinline__ bool ex_certified(int metric, int d, int dp, double rk, double gk, double ax, float t, float na, double nmax) {
    if (t == INFINITY) return true;  // nothing was left out
    if constexpr (FAM == NND_CODES_BOOL) {  // the scan's values are exact functions of exact counts: the conversion's band alone
        if (metric == NND_BOOL_FIRST) return rk < (double)t - nnd_exact_band_jaccard((double)t);
        return rk < (double)t - nnd_exact_band_bool_rational((double)t);
    }
    if (metric == 0) return rk < (double)t - nnd_exact_band_sqeuclid(dp, (double)na, nmax);
    if (metric == 4) return rk < (double)t - nnd_exact_band_correlation(d, dp);
    if (!(gk > -INFINITY)) return false;
    if (metric == 3) return gk - nnd_exact_band_inner(dp, (double)na, nmax) > nnd_exact_gram_of_inverse_dist((double)t);
    // what was left out has a Gram value of at most gt (none above 0 if its kernel distance is FLT_MAX)
    const double gt = t >= NND_FLT_MAX ? 0.0 : nnd_exact_gram_of_log_dist((double)t);
    const double lim = gt + nnd_exact_band_unit(d, dp);
    if (metric == 2) return gk > lim * sqrt(ax * nmax) * (1.0 + 1e-12);  // <a, b> of the rows as given <= cosine |a| max |b|
    return gk > lim;
}

// ---- refinement and certificate: one wave per query row ----
template <int FAM>
__device__ __forceinline__ void ex_refine_body(const float *__restrict__ x, int d, int dp, int metric, const float *__restrict__ qraw,
                                                      const int32_t *__restrict__ qids, const float *__restrict__ qnrm, int nq, int k, int W,
                                                      const uint32_t *__restrict__ list_e, const float *__restrict__ list_rej,
                                                      const double *__restrict__ nmax, int32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                      int32_t *__restrict__ uncert, int32_t *__restrict__ n_uncert) {
    __shared__ uint32_t sid[4][NND_WIDE_K];
    __shared__ double sr[4][NND_WIDE_K], sg[4][NND_WIDE_K];
    __shared__ double kth[4][2];
    const int lane = nnd_lane(), w = threadIdx.x >> 6, grp = lane >> 4, l16 = lane & 15;
    const int q = blockIdx.x * 4 + w;
    if (q >= nq) return;
    for (int j = lane; j < W; j += 64) sid[w][j] = list_e[(size_t)q * W + j];
    nnd_wave_lds_sync();
    const int qid = qids[q];
    const float *xa = qraw + (int64_t)qid * d;  // (external queries: qid = q)
    const double mua = metric == 4 ? nnd_row_mean_f64<16>(xa, d, l16) : 0.0;
    double axq = 0.0;
    for (int j0 = 0; j0 < W; j0 += 4) {
        const int j = j0 + grp;
        const uint32_t e = j < W ? sid[w][j] : NND_EMPTY_E;
        const bool on = e != NND_EMPTY_E;
        const ex_val v = ex_pair_f64<FAM>(metric, xa, x + (int64_t)(on ? (e & NND_IDX_MASK) : 0) * d, d, l16, mua);
        axq = v.ax;
        if (l16 == 0 && j < W) {
            sr[w][j] = on ? v.r : INFINITY;
            sg[w][j] = on ? v.g : -INFINITY;
        }
    }
    nnd_wave_lds_sync();
    for (int j = lane; j < W; j += 64) {
        const uint32_t e = sid[w][j], myid = e == NND_EMPTY_E ? NND_IDX_MASK : (e & NND_IDX_MASK);
        const double myr = sr[w][j];
        int rank = 0;
        for (int c = 0; c < W; c++) {
            const uint32_t ec = sid[w][c], idc = ec == NND_EMPTY_E ? NND_IDX_MASK : (ec & NND_IDX_MASK);
            const double rc = sr[w][c];
            rank += (rc < myr || (rc == myr && (idc < myid || (idc == myid && c < j)))) ? 1 : 0;
        }
        if (rank < k) {
            out_idx[(size_t)q * k + rank] = e == NND_EMPTY_E ? -1 : (int32_t)myid;
            out_dist[(size_t)q * k + rank] = (float)myr;
            if (rank == k - 1) {
                kth[w][0] = myr;
                kth[w][1] = sg[w][j];
            }
        }
    }
    nnd_wave_lds_sync();
    if (lane == 0 && !ex_certified<FAM>(metric, d, dp, kth[w][0], kth[w][1], axq, list_rej[q], qnrm[qid], *nmax)) uncert[atomicAdd(n_uncert, 1)] = q;
}
template <int FAM>
__global__ __launch_bounds__(256) void k_exact_refine(const float *__restrict__ x, int d, int dp, int metric, const float *__restrict__ qraw,
                                                      const int32_t *__restrict__ qids, const float *__restrict__ qnrm, int nq, int k, int W,
                                                      const uint32_t *__restrict__ list_e, const float *__restrict__ list_rej,
                                                      const double *__restrict__ nmax, int32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                      int32_t *__restrict__ uncert, int32_t *__restrict__ n_uncert) {
    ex_refine_body<FAM>(x, d, dp, metric, qraw, qids, qnrm, nq, k, W, list_e, list_rej, nmax, out_idx, out_dist, uncert, n_uncert);
}

// ---- tier 2: all n original rows in float64, one workgroup per listed query row ----
// Wave w takes data rows 16 i + 4 w + (0..3), four at a time (16 lanes each), in ascending order, and keeps its k best in an LDS
// list sorted by (distance, id): a row enters only if it is strictly closer than the list's last (its id is larger than every
// id the wave has seen).  The four lists are then ranked against each other.  MK: rows whose tag word does not
// meet the query row's mask are passed over, and the places that fewer than k allowed rows leave open get (-1, inf).
template <int FAM, bool MK>
__device__ __forceinline__ void ex_f64_body(const float *__restrict__ x, int64_t n, int d, int metric, const float *__restrict__ qraw,
                                                   const int32_t *__restrict__ qids, int k, const int32_t *__restrict__ list,
                                                   int32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                   const uint64_t *__restrict__ tags /* MK: (n) */, const uint64_t *__restrict__ qmasks /* MK: (nq) */) {
    __shared__ double ld[4][NND_WIDE_K];
    __shared__ int32_t li[4][NND_WIDE_K];
    __shared__ int scnt[4];
    const int lane = nnd_lane(), w = threadIdx.x >> 6, grp = lane >> 4, l16 = lane & 15;
    const int q = list[blockIdx.x];
    const float *xa = qraw + (int64_t)qids[q] * d;
    const double mua = metric == 4 ? nnd_row_mean_f64<16>(xa, d, l16) : 0.0;
    uint64_t qm = 0ull;
    if constexpr (MK) qm = qmasks[q];
    int cnt = 0;
    double worst = INFINITY;
    for (int64_t b0 = 4 * w; b0 < n; b0 += 16) {
        const int64_t jb = b0 + grp;
        const ex_val v = ex_pair_f64<FAM>(metric, xa, x + (jb < n ? jb : 0) * d, d, l16, mua);
#pragma unroll 1
        for (int u = 0; u < 4; u++) {
            const double ru = __longlong_as_double((long long)nnd_readlane_u64((uint64_t)__double_as_longlong(v.r), 16 * u));
            const int64_t ju = b0 + u;
            if (ju >= n || !(cnt < k || ru < worst)) continue;  // wave-uniform
            if constexpr (MK) {
                if ((tags[ju] & qm) == 0ull) continue;  // wave-uniform
            }
            double old_d[NND_WIDE_U];
            int32_t old_i[NND_WIDE_U];
            int below = 0;
#pragma unroll
            for (int t = 0; t < NND_WIDE_U; t++) {
                const int j = lane + 64 * t;
                old_d[t] = j < cnt ? ld[w][j] : INFINITY;
                old_i[t] = j < cnt ? li[w][j] : 0;
                below += (j < cnt && old_d[t] <= ru) ? 1 : 0;
            }
            const int pos = nnd_wave_sum_i32(below);
            const int nc = cnt < k ? cnt + 1 : k;
            nnd_wave_lds_sync();
#pragma unroll
            for (int t = 0; t < NND_WIDE_U; t++) {
                const int j = lane + 64 * t;
                if (j < cnt && j >= pos && j + 1 < nc) {
                    ld[w][j + 1] = old_d[t];
                    li[w][j + 1] = old_i[t];
                }
            }
            if (lane == 0) {
                ld[w][pos] = ru;
                li[w][pos] = (int32_t)ju;
            }
            nnd_wave_lds_sync();
            cnt = nc;
            worst = cnt == k ? ld[w][k - 1] : INFINITY;
        }
    }
    if (lane == 0) scnt[w] = cnt;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 4 * k; idx += 256) {
        const int lw = idx / k, j = idx - lw * k;
        if (j >= scnt[lw]) continue;
        const double myr = ld[lw][j];
        const int32_t myid = li[lw][j];
        int rank = 0;
        for (int ow = 0; ow < 4; ow++) {
            const int oc = scnt[ow];
            for (int c = 0; c < oc; c++) {
                const double rc = ld[ow][c];
                rank += (rc < myr || (rc == myr && li[ow][c] < myid)) ? 1 : 0;
            }
        }
        if (rank < k) {
            out_idx[(size_t)q * k + rank] = myid;
            out_dist[(size_t)q * k + rank] = (float)myr;
        }
    }
    if constexpr (MK) {  // every allowed row is in one of the four lists while they hold fewer than k together
        const int total = scnt[0] + scnt[1] + scnt[2] + scnt[3];
        for (int j = total + (int)threadIdx.x; j < k; j += 256) {
            out_idx[(size_t)q * k + j] = -1;
            out_dist[(size_t)q * k + j] = INFINITY;
        }
    }
}
template <int FAM, bool MK>
__global__ __launch_bounds__(256) void k_exact_f64(const float *__restrict__ x, int64_t n, int d, int metric, const float *__restrict__ qraw,
                                                   const int32_t *__restrict__ qids, int k, const int32_t *__restrict__ list,
                                                   int32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                   const uint64_t *__restrict__ tags /* MK: (n) */, const uint64_t *__restrict__ qmasks /* MK: (nq) */) {
    ex_f64_body<FAM, MK>(x, n, d, metric, qraw, qids, k, list, out_idx, out_dist, tags, qmasks);
}

// the largest nrm of the point set (codes 0, 3), or the largest |x|^2 of the rows as given (code 2), as a double; 16 lanes per row
__global__ __launch_bounds__(256) void k_exact_nmax(const float *__restrict__ x, const float *__restrict__ nrm, int64_t n, int d, int metric,
                                                    double *__restrict__ out) {
    const int l16 = threadIdx.x & 15;
    double best = 0.0;
    for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; row < n; row += ((int64_t)gridDim.x * 256) >> 4) {
        double v = 0.0;
        if (metric == 2) {
            for (int t = l16; t < d; t += 16) v += (double)x[row * d + t] * (double)x[row * d + t];
            v = nnd_group_sum_f64<16>(v);
        } else {
            v = (double)nrm[row];
        }
        best = fmax(best, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, 64));
    // non-negative doubles order like their bit patterns
    if (nnd_lane() == 0) atomicMax((unsigned long long *)out, (unsigned long long)__double_as_longlong(best));
}
__global__ void k_exact_iota(int32_t *__restrict__ p, int n, int base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = base + i;
}
// row ids that arrive on the device are checked there, on their way into the batch: an id outside [0, n) is counted and replaced
// by 0 (the scan would read that row), and the count comes back with the batch's answers
__global__ __launch_bounds__(256) void k_exact_take_ids(const int32_t *__restrict__ ids, int count, int64_t n, int32_t *__restrict__ out, int32_t *__restrict__ n_bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t id = ids[i];
    const bool bad = id < 0 || (int64_t)id >= n;
    out[i] = bad ? 0 : id;
    if (bad) atomicAdd(n_bad, 1);
}

// ---- host side ----
int nnd_exact_slices_for(int64_t n, int64_t nq) {
    if (nq > EX_BATCH) nq = EX_BATCH;
    // ~1024 workgroups (four per CU) when the query blocks alone do not fill the chip; a slice is a whole number of tiles
    const int64_t nqb = (nq + EX_QB - 1) / EX_QB, ntiles = (n + EX_TB - 1) / EX_TB;
    int64_t s = nqb > 0 ? (1024 + nqb - 1) / nqb : 1;
    if (s > 64) s = 64;
    if (s > ntiles) s = ntiles;
    if (s < 1) s = 1;
    const int64_t tps = (ntiles + s - 1) / s;
    return (int)((ntiles + tps - 1) / tps);
}
// list width: k plus slack, a width the merges take (one entry per lane up to 64, whole 64s above), at most NND_WIDE_K.  The slack
// only moves the share of rows that need the float64 tier.
static int ex_list_width(int k) {
    if (k <= 20) return 32;
    if (k <= 48) return 64;
    const int w = ((k + 32 + 63) / 64) * 64;
    return w > NND_WIDE_K ? NND_WIDE_K : w;
}
static size_t ex_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the metric's family as a table index: NND_CODES_01, NND_CODES_0_5, NND_CODES_BOOL
static int ex_family(int metric) { return nnd_metric_bool(metric) ? 2 : metric >= 2 ? 1 : 0; }
// every instance of the scan for one DC, by [family][wide][masked]
template <int DC>
static auto ex_scan_kernel(int fam, bool wide, bool masked) -> decltype(&k_exact_scan<DC, NND_CODES_01, false, false>) {
#define EX_SCAN(FAM) {{k_exact_scan<DC, FAM, false, false>, k_exact_scan<DC, FAM, false, true>}, {k_exact_scan<DC, FAM, true, false>, k_exact_scan<DC, FAM, true, true>}}
    static const decltype(&k_exact_scan<DC, NND_CODES_01, false, false>) table[3][2][2] = {EX_SCAN(NND_CODES_01), EX_SCAN(NND_CODES_0_5), EX_SCAN(NND_CODES_BOOL)};
#undef EX_SCAN
    return table[fam][wide][masked];
}
static auto ex_refine_kernel(int fam) -> decltype(&k_exact_refine<NND_CODES_01>) {
    static const decltype(&k_exact_refine<NND_CODES_01>) table[3] = {k_exact_refine<NND_CODES_01>, k_exact_refine<NND_CODES_0_5>, k_exact_refine<NND_CODES_BOOL>};
    return table[fam];
}
static auto ex_f64_kernel(int fam, bool masked) -> decltype(&k_exact_f64<NND_CODES_01, false>) {
    static const decltype(&k_exact_f64<NND_CODES_01, false>) table[3][2] = {{k_exact_f64<NND_CODES_01, false>, k_exact_f64<NND_CODES_01, true>},
                                                                            {k_exact_f64<NND_CODES_0_5, false>, k_exact_f64<NND_CODES_0_5, true>},
                                                                            {k_exact_f64<NND_CODES_BOOL, false>, k_exact_f64<NND_CODES_BOOL, true>}};
    return table[fam][masked];
}

// `tags` (with `qmasks`): the masked scan; nullptr: the plain one
template <int DC>
static int ex_launch_scan(nnd_ctx *ctx, bool wide, dim3 grid, const float *qx, const float *qnrm, const int32_t *qids, int self, int nq, int nq_pad,
                          int W, int64_t rows_per_slice, uint32_t *le, float *ld, float *lth, float *lrej, const uint64_t *tags, const uint64_t *qmasks) {
    const size_t lds = sizeof(float) * ((EX_QB + EX_TB) * DC + EX_TB) + sizeof(int32_t) * EX_QB + sizeof(uint2) * EX_QB * EX_PC +
                       (wide ? sizeof(uint64_t) * 4 * NND_WIDE_SCRATCH_WORDS : 0) + (tags ? sizeof(uint64_t) * EX_TB : 0);
    auto kern = ex_scan_kernel<DC>(ex_family(ctx->p.metric), wide, tags != nullptr);
    if (lds > 48 * 1024) NND_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, ctx->stream, ctx->xp, ctx->nrm, ctx->n, ctx->dp, nnd_kmetric(ctx), qx, qnrm, qids, self, nq, nq_pad, W, rows_per_slice,
                       le, ld, lth, lrej, tags, qmasks);
    NND_HIP_CHECK(hipGetLastError());
    return 0;
}

static size_t ex_dtype_size(int dtype) { return dtype == NND_DTYPE_FLOAT64 ? 8 : dtype == NND_DTYPE_FLOAT32 ? 4 : 2; }

// `dev` (the device entries): row ids / queries are read from, and the answers written to, memory of the handle's device -- every
// copy below becomes device to device on the handle's stream; only the per-batch scalars cross the bus
// `tg` (the masked entries): device pointers to the n tag words of the point set and the nq_all mask words of the query rows
int nnd_exact_knn_impl(nnd_ctx *ctx, const int64_t *rows, const float *q, int64_t nq_all, int k, int32_t *out_idx, float *out_dist, nnd_exact_stats *st,
                       const nnd_exact_dev *dev, const nnd_exact_tags *tg) {
    const uint64_t *tags = tg ? tg->tags_dev : nullptr;
    const int64_t n = ctx->n;
    const int d = ctx->d, dp = ctx->dp, metric = ctx->p.metric;
    const bool self = dev ? dev->q_dev == nullptr : q == nullptr, force_f64 = (ctx->p.flags & NND_FLAG_TEST_EXACT_F64) != 0;
    const bool some_rows = dev ? dev->rows_dev != nullptr : rows != nullptr;
    const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n > (int64_t)NND_IDX_MASK) { ctx->set_error("exact search: more than 2^31 - 1 points"); return 1; }
    const int W = ex_list_width(k);
    const bool wide = W > 64;
    nnd_exact_stats s{};
    std::vector<int32_t> ids;
    if (self && rows && !dev) {
        ids.resize((size_t)nq_all);
        for (int64_t i = 0; i < nq_all; i++) {
            if (rows[i] < 0 || rows[i] >= n) { ctx->set_error("exact search: row id %lld is outside [0, %lld)", (long long)rows[i], (long long)n); return 1; }
            ids[(size_t)i] = (int32_t)rows[i];
        }
    }
    // the workspace of one batch of query rows, carved out of one grow-only buffer of the handle
    const int64_t bmax = nq_all < EX_BATCH ? nq_all : EX_BATCH;
    const int64_t bpad = (bmax + EX_QB - 1) / EX_QB * EX_QB;
    int s_cap = 1;  // (a short last batch is split into more slices than a full one)
    for (int64_t b0 = 0; b0 < nq_all; b0 += EX_BATCH) {
        const int sb = nnd_exact_slices_for(n, nq_all - b0 < EX_BATCH ? nq_all - b0 : EX_BATCH);
        if (sb > s_cap) s_cap = sb;
    }
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += ex_align(bytes); return o; };
    const size_t o_qids = carve(sizeof(int32_t) * bpad), o_qraw = carve(self ? 0 : sizeof(float) * bmax * d), o_qp = carve(self ? 0 : sizeof(float) * bpad * dp),
                 o_qnrm = carve(self ? 0 : sizeof(float) * bpad), o_le = carve(sizeof(uint32_t) * (size_t)s_cap * bpad * W),
                 o_ld = carve(sizeof(float) * (size_t)s_cap * bpad * W), o_th = carve(sizeof(float) * (size_t)s_cap * bpad),
                 o_rej = carve(sizeof(float) * (size_t)s_cap * bpad), o_oi = carve(sizeof(int32_t) * bmax * k), o_od = carve(sizeof(float) * bmax * k),
                 o_unc = carve(sizeof(int32_t) * bpad), o_misc = carve(64);
    if (!ctx->mem.grow(&ctx->exact_ws, &ctx->exact_ws_cap, off, off)) { ctx->set_error("exact search: allocation of %zu workspace bytes on the device failed", off); return 1; }
    unsigned char *ws = ctx->exact_ws;
    int32_t *qids = (int32_t *)(ws + o_qids), *oi = (int32_t *)(ws + o_oi), *unc = (int32_t *)(ws + o_unc);
    float *qraw_own = (float *)(ws + o_qraw), *qp = (float *)(ws + o_qp), *qn = (float *)(ws + o_qnrm), *ld = (float *)(ws + o_ld), *lth = (float *)(ws + o_th),
          *lrej = (float *)(ws + o_rej), *od = (float *)(ws + o_od);
    uint32_t *le = (uint32_t *)(ws + o_le);
    double *nmax = (double *)(ws + o_misc);
    int32_t *n_unc = (int32_t *)(ws + o_misc + 8), *n_bad = (int32_t *)(ws + o_misc + 12);

    NND_HIP_CHECK(hipMemsetAsync(nmax, 0, 16, ctx->stream));
    if (!force_f64 && (metric == 0 || metric == 2 || metric == 3)) {
        int64_t blocks = (n * 16 + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_exact_nmax, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->x_orig, ctx->nrm, n, d, metric, nmax);
        NND_HIP_CHECK(hipGetLastError());
    }
    for (int64_t b0 = 0; b0 < nq_all; b0 += EX_BATCH) {
        const int nq = (int)(nq_all - b0 < EX_BATCH ? nq_all - b0 : EX_BATCH);
        const int nq_pad = (nq + EX_QB - 1) / EX_QB * EX_QB;
        if (self && some_rows) {
            if (dev) {
                hipLaunchKernelGGL(k_exact_take_ids, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, dev->rows_dev + b0, nq, n, qids, n_bad);
                NND_HIP_CHECK(hipGetLastError());
            } else NND_HIP_CHECK(hipMemcpyAsync(qids, ids.data() + b0, sizeof(int32_t) * nq, hipMemcpyHostToDevice, ctx->stream));
        } else {  // all rows: ids b0 ..; external queries: their index in the batch's own prepared copy
            hipLaunchKernelGGL(k_exact_iota, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, qids, nq, self ? (int)b0 : 0);
            NND_HIP_CHECK(hipGetLastError());
        }
        const float *qraw = ctx->x_orig, *qx = ctx->xp, *qnrm = ctx->nrm;
        if (!self) {
            // the queries through the point set's own preparation (code 0: the SET's column means): the prep kernels write where
            // the handle's prepared-row pointers point
            if (dev) {  // typed device queries: converted (dot: and L2-normalised, as the typed data entry does) into the same copy
                const char *src = (const char *)dev->q_dev + (size_t)b0 * d * ex_dtype_size(dev->q_dtype);
                if (nnd_launch_rows_f32(ctx->stream, src, dev->q_dtype, nq, d, metric == NND_METRIC_ALT_DOT, qraw_own)) {
                    (void)hipGetLastError();
                    ctx->set_error("exact search: conversion kernel launch failed");
                    return 1;
                }
            } else {
                NND_HIP_CHECK(hipMemcpyAsync(qraw_own, q + b0 * d, sizeof(float) * (size_t)nq * d, hipMemcpyHostToDevice, ctx->stream));
            }
            float *xp0 = ctx->xp, *nrm0 = ctx->nrm;
            uint16_t *xh0 = ctx->xh;
            float2 *nr20 = ctx->nr2;
            ctx->xp = qp; ctx->nrm = qn; ctx->xh = nullptr; ctx->nr2 = nullptr;
            const int rc = nnd_prep_rows(ctx, qraw_own, 0, nq, false);
            ctx->xp = xp0; ctx->nrm = nrm0; ctx->xh = xh0; ctx->nr2 = nr20;
            if (rc) return 1;
            qraw = qraw_own; qx = qp; qnrm = qn;
        }
        NND_HIP_CHECK(hipMemsetAsync(n_unc, 0, sizeof(int32_t), ctx->stream));
        const uint64_t *qmasks = tg ? tg->masks_dev + b0 : nullptr;
        int n_fallback = nq;
        if (!force_f64) {
            const int S = nnd_exact_slices_for(n, nq);
            const int64_t ntiles = (n + EX_TB - 1) / EX_TB, rows_per_slice = (ntiles + S - 1) / S * EX_TB;
            const dim3 grid((unsigned)(nq_pad / EX_QB), (unsigned)S);
            const int t_scan = t_begin(ctx);
            int rc;
            if (dp <= 32) rc = ex_launch_scan<32>(ctx, wide, grid, qx, qnrm, qids, self, nq, nq_pad, W, rows_per_slice, le, ld, lth, lrej, tags, qmasks);
            else if (dp <= 64) rc = ex_launch_scan<64>(ctx, wide, grid, qx, qnrm, qids, self, nq, nq_pad, W, rows_per_slice, le, ld, lth, lrej, tags, qmasks);
            else rc = ex_launch_scan<128>(ctx, wide, grid, qx, qnrm, qids, self, nq, nq_pad, W, rows_per_slice, le, ld, lth, lrej, tags, qmasks);
            if (rc) return 1;
            if (S > 1) {
                hipLaunchKernelGGL(wide ? k_exact_merge<true> : k_exact_merge<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, nq, nq_pad, W, S, le, ld, lth, lrej);
                NND_HIP_CHECK(hipGetLastError());
            }
            t_end(ctx, t_scan, &s.ms_scan, true);
            const int t_ref = t_begin(ctx);
            hipLaunchKernelGGL(ex_refine_kernel(ex_family(metric)), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, ctx->x_orig, d, dp, metric, qraw,
                               qids, qnrm, nq, k, W, le, lrej, nmax, oi, od, unc, n_unc);
            NND_HIP_CHECK(hipGetLastError());
            t_end(ctx, t_ref, &s.ms_refine, true);
            NND_HIP_CHECK(hipMemcpyAsync(&ctx->h_pin->spare[0], n_unc, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            t_flush(ctx);
            NND_HIP_CHECK(nnd_sync_spin(ctx));
            n_fallback = *(const int32_t *)&ctx->h_pin->spare[0];
            s.pairs += (int64_t)nq * n;
            s.mfma += (int64_t)grid.x * ntiles * 4 /* waves */ * 4 /* accumulator tiles */ * (dp / 4);
        } else {
            hipLaunchKernelGGL(k_exact_iota, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, unc, nq, 0);
            NND_HIP_CHECK(hipGetLastError());
        }
        if (n_fallback > 0) {
            const int t_fb = t_begin(ctx);
            hipLaunchKernelGGL(ex_f64_kernel(ex_family(metric), tags != nullptr), dim3((unsigned)n_fallback), dim3(256), 0, ctx->stream, ctx->x_orig, n, d, metric, qraw, qids,
                               k, unc, oi, od, tags, qmasks);
            NND_HIP_CHECK(hipGetLastError());
            t_end(ctx, t_fb, &s.ms_fallback, true);
        }
        NND_HIP_CHECK(hipMemcpyAsync(out_idx + b0 * k, oi, sizeof(int32_t) * (size_t)nq * k, out_kind, ctx->stream));
        NND_HIP_CHECK(hipMemcpyAsync(out_dist + b0 * k, od, sizeof(float) * (size_t)nq * k, out_kind, ctx->stream));
        const bool ids_checked = dev && self && some_rows;
        if (ids_checked) NND_HIP_CHECK(hipMemcpyAsync(&ctx->h_pin->spare[1], n_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        t_flush(ctx);
        NND_HIP_CHECK(nnd_sync_spin(ctx));
        if (ids_checked && *(const int32_t *)&ctx->h_pin->spare[1]) {
            ctx->set_error("exact search: %d row ids are outside [0, %lld)", (int)*(const int32_t *)&ctx->h_pin->spare[1], (long long)n);
            return 1;
        }
        s.n_rows += nq;
        s.n_fallback += n_fallback;
    }
    if (st) *st = s;
    return 0;
}
