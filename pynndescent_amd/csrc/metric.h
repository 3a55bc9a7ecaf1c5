// metric.h -- what a metric code means on the device: the one home of every distance formula on prepared rows and of the
// float64 reference formula on the rows as given.  (query.hip keeps the float32 formulas of its own that work on RAW rows:
// the cosine of q_quad_dist, the uint8 proxies of q_quad_proxy and the rerank's un-clamped dot.)
//
// Metric codes (include/pynnd_amd.h NND_METRIC_*): 0 sqeuclidean, 1 alt cosine, 2 alt dot, 3 alt inner product,
// 4 correlation, 5 alt hellinger, 6 proxy inner product, 8..16 the boolean family (below).  The prep kernel turns every row into a "prepared" row whose inner
// products give the distance (DESIGN.md "Metrics"):
//   unit metrics (1, 2, 4, 5): rows L2-normalised after a per-metric transform (none / none / minus the row mean / sqrt);
//     nrm = 1 (non-zero row) or 0 (zero row); the trees split angularly;
//   norm metrics (0, 3, 6): rows centred on the column mean (0) or as given (3, 6); nrm = |x|^2; euclidean trees;
//   boolean metrics (8..16): indicator rows (x != 0 -> 1.0f, else 0.0f), norm metrics too: nrm = nnz(x); euclidean trees.
// The metrics with a fixed linear map (seuclidean, wminkowski with p = 2, mahalanobis) have no code and no formula here: they
// are code 0 on rows that k_linear_rows (linear.hip) transformed once, y = A (x - c), before any kernel of this header sees them.
// Four pieces, and which kernel takes which (DESIGN.md "Metrics" has the table):
//   1. nnd_gram_to_dist / nnd_self_dist   float32 Gram value of two prepared rows -> distance (every kernel that ranks)
//   2. nnd_ref_acc / nnd_ref_dist         float64 reference formula on the rows AS GIVEN (the distances handed back)
//   3. nnd_row_pair_dist                  float32 distance of two prepared rows, one wave per pair
//   4. nnd_row_mean_f64 / nnd_unit_transform   the unit-row transform of prep and query
// The part above `#ifdef __HIPCC__` is plain C++ (tests/metric_cpu.cpp compiles it with the host compiler, no HIP headers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define NND_HD __host__ __device__
#else
#define NND_HD
#endif
#define NND_HD_INLINE NND_HD inline __attribute__((always_inline))

#define NND_FLT_MAX 3.402823466e+38f

NND_HD_INLINE bool nnd_metric_unit(int metric) { return metric == 1 || metric == 2 || metric == 4 || metric == 5; }

// The boolean family (include/pynnd_amd.h NND_METRIC_JACCARD .. NND_METRIC_YULE): 8 jaccard (alternative_jaccard), 9 dice,
// 10 sokalsneath, 11 matching, 12 rogerstanimoto, 13 sokalmichener, 14 kulsinski, 15 russellrao, 16 yule (7 is no code:
// tests/test_plan_cpu.py pins its refusal).  Six of the formulas
// need the true column count d, and the ranking kernels receive only dp.  d travels INSIDE the kernels' `metric` argument:
// for these codes a launcher hands over nnd_kernel_metric(code, d) = code | d << 8, so no kernel's argument block grows and
// the instances of the other codes see the value they always saw (DESIGN.md "Boolean metrics").  nnd_create refuses
// d >= 2^23 for the family: the counts stay exact float32 integers and the packed value an int.
#define NND_BOOL_FIRST 8
#define NND_BOOL_LAST 16
NND_HD_INLINE bool nnd_metric_bool(int code) { return code >= NND_BOOL_FIRST && code <= NND_BOOL_LAST; }
NND_HD_INLINE int nnd_kernel_metric(int code, int d) { return nnd_metric_bool(code) ? code | (d << 8) : code; }

// The codes a kernel instance can meet, fixed at compile time: a conversion carries the branches of its family's codes and no
// others (in the unrolled epilogues of the Gram kernels every branch is paid per accumulator register: the six-way branch cost
// k_local_join16<32, 1|2, false> four VGPRs, DESIGN.md "Metrics").  A new kernel takes the narrowest family its launcher
// guarantees, NND_CODES_ANY if the code is only known at run time.  The values are the XM template arguments of the join
// kernels (join.hip), so they are part of those kernels' names.
enum nnd_metric_family {
    NND_CODES_01 = 0,   // sqeuclidean / cosine
    NND_CODES_0_5 = 1,  // every code but 6 (kernels where code 6 has an instance of its own, or is refused by the host)
    NND_CODE_6 = 2,     // proxy inner product alone: no branch on the code
    NND_CODES_BOOL = 3, // the boolean family alone (8..16, `metric` packed by nnd_kernel_metric): the branch among its nine formulas
    NND_CODES_ANY = 4,  // 0..6, by a branch on the code (the first template argument of the build kernels' instances for these codes:
                        // k_leaf_join<4, ...>, k_diversify_rows<4, ...>; no join kernel has it); the boolean family is never part of
                        // a branch: every kernel that ranks has instances of its own for it (NND_CODES_BOOL)
};

// ---------------------------------------------------------------------------------------------------------------------
// 2. The reference's formula in float64 on a pair of rows as given: what finalize hands back and exact search ranks by.
//      sqeuclidean  sum (x_i - y_i)^2                                                     (distances.py:63-91)
//      cosine       log2(sqrt(|x|^2 |y|^2) / <x,y>)                                       (distances.py:583-630)
//      dot          -log2 <x,y> on the rows as given (NNDescent normalises them on the host)   (distances.py:680-702)
//      inner product 1 / <x,y>                                                            (distances.py:759-790)
//      correlation  1 - <x-mx, y-my> / sqrt(|x-mx|^2 |y-my|^2), the row means first       (distances.py:1284-1313)
//      hellinger    log2(sqrt(|x|_1 |y|_1) / sum sqrt(x_i y_i))                           (distances.py:1387-1417)
//      proxy inner product  max(-log2(<x,y> / sqrt(|x|^2 |y|^2)), 0) + 1 / sqrt<x,y>      (distances.py:810-838)
//    nnd_ref_acc adds one coordinate pair to the three sums (code 0: the squared difference into `dot`; code 4: a and b
//    already minus their row means); nnd_ref_dist turns the sums into the distance.
// The float64 kernels have always kept an instance of their own for the codes 0 / 1 (it does not carry the other codes'
// registers), so nnd_ref_acc<NND_CODES_01> serves the codes 0 and 1 and every other family the codes above 1: a kernel picks
// the family by the same test that picks its instance (finalize.hip, exact.hip).  The build is bit-reproducible, and the last
// bit of a sum depends on whether a product is fused into its addition, so the two halves are written as they have always been
// compiled: fused multiply-adds for the codes 0 / 1 (written out, or the compiler merges the two branches' updates of `dot`
// into one unfused addition); plain statements, `dot` first, for the others (where the code is a compile-time constant they
// are fused, where it is a run-time value the branches' updates are merged and are not: profiles/metric_header_isa.txt).
// Each branch must end on the same sum as its siblings, or the merged update goes through a pointer and the sums to scratch.
// The hellinger term sqrt(x_i y_i) is the one place where the two users differ, on purpose: finalize takes it as the reference
// does, sqrtf of the float32 product, so that the distances handed back are the reference's; exact search takes it in float64
// (the float32 terms move a distance by 1e-7, enough to swap two near neighbours of a ranking that claims to be exact).
//    The boolean family (8..16) counts: dot += (a != 0 && b != 0), nx += (a != 0), ny += (b != 0) on the rows as given, then
//    nnd_bool_dist_f64 on the three counts and the column count d, which nnd_ref_dist takes as a fourth value.
enum nnd_hellinger_terms { NND_HELLINGER_F32, NND_HELLINGER_F64 };

// The boolean family's conversion in float64, the twin of the device's nnd_bool_dist below: (code, c, na, nb, d) -> distance
// for c = n_TT, na = nnz(x), nb = nnz(y) (reference distances.py:259-552; ne = n_TF + n_FT = na + nb - 2c).
//   jaccard        0 if the union is empty, FLT_MAX if c = 0 (+inf in the reference), else -log2(c / (c + ne))
//   dice           0 if ne = 0, else ne / (2c + ne)              sokalsneath  the same with 0.5c
//   matching       ne / d                                        rogerstanimoto, sokalmichener  2ne / (d + ne)
//   kulsinski      0 if ne = 0, else (ne - c + d) / (ne + d)     russellrao   0 if c = na = nb, else (d - c) / d
//   yule           0 if n_TF = 0 or n_FT = 0, else 2 n_TF n_FT / (c n_FF + n_TF n_FT)
NND_HD_INLINE double nnd_bool_dist_f64(int code, double c, double na, double nb, double d) {
    const double ne = na + nb - 2.0 * c;
    switch (code) {
        case 8: {
            if (c + ne == 0.0) return 0.0;
            if (c == 0.0) return (double)NND_FLT_MAX;
            const double r = -log2(c / (c + ne));
            return r > 0.0 ? r : 0.0;
        }
        case 9: return ne == 0.0 ? 0.0 : ne / (2.0 * c + ne);
        case 10: return ne == 0.0 ? 0.0 : ne / (0.5 * c + ne);
        case 11: return ne / d;
        case 12:
        case 13: return (2.0 * ne) / (d + ne);
        case 14: return ne == 0.0 ? 0.0 : (ne - c + d) / (ne + d);
        case 15: return (c == na && c == nb) ? 0.0 : (d - c) / d;
        default: {
            const double tf = na - c, ft = nb - c, ff = d - na - nb + c;
            if (tf == 0.0 || ft == 0.0) return 0.0;
            return (2.0 * tf * ft) / (c * ff + tf * ft);
        }
    }
}

template <int FAM, int HELL>
NND_HD_INLINE void nnd_ref_acc(int metric, double a, double b, double &dot, double &nx, double &ny) {
    if constexpr (FAM == NND_CODES_01) {
        if (metric == 0) {
            dot = fma(a - b, a - b, dot);
        } else {
            nx = fma(a, a, nx);
            ny = fma(b, b, ny);
            dot = fma(a, b, dot);
        }
    } else if constexpr (FAM == NND_CODES_BOOL) {  // the counts n_TT, nnz(x), nnz(y)
        dot += (a != 0.0 && b != 0.0) ? 1.0 : 0.0;
        nx += a != 0.0 ? 1.0 : 0.0;
        ny += b != 0.0 ? 1.0 : 0.0;
    } else if (metric == 5) {  // sum sqrt(x_i y_i), |x|_1, |y|_1
        if constexpr (HELL == NND_HELLINGER_F32) dot += (double)sqrtf((float)a * (float)b);
        else dot += sqrt(a * b);
        nx += a;
        ny += b;
    } else {
        dot += a * b;
        nx += a * a;
        ny += b * b;
    }
}
// The distance as a double: 0, 1 and FLT_MAX come out exactly, so a cast to float32 keeps them; every value is >= 0.
// No intrinsics: the same text runs on the host.
template <int FAM>
NND_HD_INLINE double nnd_ref_dist(int metric, double dt, double ax, double ay, double d = 0.0) {
    if constexpr (FAM == NND_CODES_BOOL) return nnd_bool_dist_f64(metric & 0xff, dt, ax, ay, d);
    constexpr bool m01 = FAM == NND_CODES_01, m6 = FAM == NND_CODE_6 || FAM == NND_CODES_ANY;
    if (metric == 0) return dt;
    if (!m01 && (metric == 2 || metric == 3)) {  // alternative_dot / alternative_inner_product: FLT_MAX for <x,y> <= 0
        if (!(dt > 0.0)) return (double)NND_FLT_MAX;
        const double r = metric == 2 ? -log2(dt) : 1.0 / dt;
        return r > 0.0 ? fmin(r, (double)NND_FLT_MAX) : 0.0;
    }
    if (m6 && metric == 6) {  // proxy_inner_product: FLT_MAX for a zero row or <x,y> <= 0 (nnd_proxy_ip_dist)
        if (ax == 0.0 || ay == 0.0 || !(dt > 0.0)) return (double)NND_FLT_MAX;
        const double c = -log2(dt / sqrt(ax * ay));
        return fmin((c > 0.0 ? c : 0.0) + 1.0 / sqrt(dt), (double)NND_FLT_MAX);
    }
    if (!m01 && metric == 4) {  // correlation: 0 if both rows have zero variance, 1 if <x,y> = 0
        if (ax == 0.0 && ay == 0.0) return 0.0;
        if (dt == 0.0) return 1.0;
        const double r = 1.0 - dt / sqrt(ax * ay);
        return r > 0.0 ? r : 0.0;
    }
    if (ax == 0.0 && ay == 0.0) return 0.0;  // alternative_cosine / alternative_hellinger
    if (ax == 0.0 || ay == 0.0 || dt <= 0.0) return (double)NND_FLT_MAX;
    const double r = log2(sqrt(ax * ay) / dt);
    return r > 0.0 ? r : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. (first half) The per-element transform of the unit-row metrics before the normalisation: correlation subtracts the row
// mean mu, hellinger takes the square root (a negative entry raises the negative-input flag; its NaN never reaches a distance
// the host hands out).  The mean stays in float64 up to the subtraction: rounded to float32 first, a row on a large common
// offset (1e3 + N(0, 1e-2)) would lose half an ulp of the offset, a relative error of 3e-3 in its centred entries (2e-4 in a
// distance, DESIGN.md "Metrics").  Every user takes mu from nnd_row_mean_f64 and hands it over as a double.
NND_HD_INLINE float nnd_unit_transform(int metric, float v, double mu) {
    if (metric == 4) return (float)((double)v - mu);
    if (metric == 5) return sqrtf(v);
    return v;
}

#ifdef __HIPCC__
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// 1. Gram value -> alt-space distance.  Every value is >= 0: the k-lists order distances by their float bits.
//   euclid:  |a|^2 + |b|^2 - 2<a,b>          (reference distances.py:63-91 in Gram form)
//   cosine / hellinger: rows are pre-normalised, na/nb are 1 (non-zero row) or 0 (zero row):
//            0 if both zero, FLT_MAX if one zero or <a,b> <= 0, else -log2(<a,b>) (distances.py:583-630, 1387-1417)
//   dot:     FLT_MAX if either row is zero (both zero too) or <a,b> <= 0, else -log2(<a,b>) (distances.py:680-702)
//   inner product: FLT_MAX if <a,b> <= 0, else 1 / <a,b> (distances.py:759-790)
//   correlation: rows centred and normalised: 0 if both zero, else 1 - <a,b> clamped >= 0 (distances.py:1284-1313)
//   proxy inner product: rows as given, na/nb = |a|^2, |b|^2: FLT_MAX if either row is zero or <a,b> <= 0, else
//            max(-log2(<a,b> / sqrt(|a|^2 |b|^2)), 0) + 1 / sqrt(<a,b>) (distances.py:810-838; <a,b> = 0 is +inf there:
//            DESIGN.md "Proxy distances")
// Three transcendental instructions (two v_rsq_f32, one v_log_f32, 1 ulp each) instead of IEEE sqrt / divide sequences: the
// conversion sits in the unrolled epilogues of the Gram kernels, where every instruction is paid per accumulator register.
// The cosine is g * rsq(na) * rsq(nb) (no product of the norms: it cannot overflow where the cosine is finite).
__device__ __forceinline__ float nnd_proxy_ip_dist(float g, float na, float nb) {
    if (na == 0.0f || nb == 0.0f || !(g > 0.0f)) return NND_FLT_MAX;
    const float cosv = g * __frsqrt_rn(na) * __frsqrt_rn(nb);
    return fminf(nnd_clamp_dist(-__log2f(cosv)) + __frsqrt_rn(g), NND_FLT_MAX);
}
// The boolean family: the ONE conversion of every ranking site (the joins' XM = 3 instances, the leaf kernels, k_pairwise,
// nnd_row_pair_dist, k_query, the exact scan), so that two kernels cannot disagree on a pair.  c, na, nb are Gram values of
// indicator rows: integers below 2^24, exact in float32 whatever the summation order, so the result is a function of four
// integers.  Every operation is one IEEE float32 operation, never fused (contraction is off in the body: yule's c n_FF +
// n_TF n_FT is the one place where a fused multiply-add would round differently) and the division is the correctly rounded one,
// not v_rcp_f32: tests/boolean_util.py restates the expressions in float32 numpy and the GPU tests hold the eight rational
// formulas to them bit for bit.  jaccard's -log2 is the hardware's (v_log_f32, 1 ulp), as cosine's.
__device__ __forceinline__ float nnd_bool_dist(int code, float c, float na, float nb, float d) {
#pragma clang fp contract(off)
    const float ne = na + nb - (c + c);
    switch (code) {
        case 8: {
            const float u = c + ne;
            if (u == 0.0f) return 0.0f;
            if (c == 0.0f) return NND_FLT_MAX;
            return nnd_clamp_dist(-__log2f(__fdiv_rn(c, u)));
        }
        case 9: return ne == 0.0f ? 0.0f : __fdiv_rn(ne, 2.0f * c + ne);
        case 10: return ne == 0.0f ? 0.0f : __fdiv_rn(ne, 0.5f * c + ne);
        case 11: return __fdiv_rn(ne, d);
        case 12:
        case 13: return __fdiv_rn(ne + ne, d + ne);
        case 14: return ne == 0.0f ? 0.0f : __fdiv_rn(ne - c + d, ne + d);
        case 15: return (c == na && c == nb) ? 0.0f : __fdiv_rn(d - c, d);
        default: {
            const float tf = na - c, ft = nb - c, ff = d - na - nb + c;
            if (tf == 0.0f || ft == 0.0f) return 0.0f;
            const float p = tf * ft;
            return __fdiv_rn(p + p, c * ff + p);
        }
    }
}
template <int FAM>
__device__ __forceinline__ float nnd_gram_to_dist(int metric, float g, float na, float nb) {
    constexpr bool m01 = FAM == NND_CODES_01;
    if constexpr (FAM == NND_CODE_6) return nnd_proxy_ip_dist(g, na, nb);
    if constexpr (FAM == NND_CODES_BOOL) return nnd_bool_dist(metric & 0xff, g, na, nb, (float)(metric >> 8));
    if (metric == 0) return nnd_clamp_dist(na + nb - 2.0f * g);
    if (!m01 && metric == 3) return g > 0.0f ? fminf(1.0f / g, NND_FLT_MAX) : NND_FLT_MAX;
    if constexpr (FAM == NND_CODES_ANY)
        if (metric == 6) return nnd_proxy_ip_dist(g, na, nb);
    if (na == 0.0f && nb == 0.0f && (m01 || metric != 2)) return 0.0f;
    if (!m01 && metric == 4) return nnd_clamp_dist(1.0f - g);
    if (na == 0.0f || nb == 0.0f || g <= 0.0f) return NND_FLT_MAX;
    return nnd_clamp_dist(-__log2f(g));
}
// d(x, x) of a row with prepared norm value n (nrm): the join kernels set the self pair by this rule instead of the Gram
// value.  The reference does evaluate the pair (utils.py:619 starts the inner loop at j): 0 for every metric whose
// distance to itself is 0, FLT_MAX for a zero row under dot, 1 / |x|^2 under inner product, 1 / |x| under its proxy.
template <int FAM>
__device__ __forceinline__ float nnd_self_dist(int metric, float n) {
    constexpr bool only6 = FAM == NND_CODE_6;
    if constexpr (FAM == NND_CODES_01 || FAM == NND_CODES_BOOL) return 0.0f;  // (the boolean family: 0 for all nine)
    if (!only6 && metric == 3) return n > 0.0f ? fminf(1.0f / n, NND_FLT_MAX) : NND_FLT_MAX;
    if (only6 || (FAM == NND_CODES_ANY && metric == 6)) return n > 0.0f ? fminf(__frsqrt_rn(n), NND_FLT_MAX) : NND_FLT_MAX;
    if (metric == 2 && n == 0.0f) return NND_FLT_MAX;
    return 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. Alt-space distance of the prepared rows a and b, one wave per pair (all 64 lanes take part): lane-strided partial sums,
// then nnd_wave_sum_f32; the difference form for sqeuclidean.  merge.hip (random init, proposals without a stored distance)
// and prune.hip (the pruning passes).
template <int FAM = NND_CODES_ANY>
__device__ __forceinline__ float nnd_row_pair_dist(const float *__restrict__ xp, int dp, const float *__restrict__ nrm, int metric,
                                                   int64_t a, int64_t b) {
    const float *xa = xp + a * dp, *xb = xp + b * dp;
    float s = 0.0f;
    for (int j = nnd_lane(); j < dp; j += 64) {
        const float p = xa[j], q = xb[j];
        s += metric == 0 ? (p - q) * (p - q) : p * q;
    }
    s = nnd_wave_sum_f32(s);
    if constexpr (FAM == NND_CODES_BOOL) return nnd_gram_to_dist<FAM>(metric, s, nrm[a], nrm[b]);  // (0 / 1 products: s is a count)
    if (metric == 0) return nnd_clamp_dist(s);
    return nnd_gram_to_dist<NND_CODES_ANY>(metric, s, nrm[a], nrm[b]);
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. / 4. (device half) float64 sum over an aligned group of LANES lanes (16: four pairs per wave in finalize and exact
// search; 64: the wave), and the mean of the d floats at xr over such a group, lane l of it taking l, l + LANES, ...: in
// float64, as the reference's correlation does (a constant row centres to exact zeros).
template <int LANES>
__device__ __forceinline__ double nnd_group_sum_f64(double v) {
#pragma unroll
    for (int o = LANES >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int LANES>
__device__ __forceinline__ double nnd_row_mean_f64(const float *xr, int d, int l) {
    double m = 0.0;
    for (int t = l; t < d; t += LANES) m += (double)xr[t];
    return nnd_group_sum_f64<LANES>(m) / (double)d;
}
#endif  // __HIPCC__
