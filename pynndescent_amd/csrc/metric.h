// metric.h -- what a metric code means on the device: the one home of every distance formula on prepared rows and of the
// float64 reference formula on the rows as given.  (query.hip keeps the float32 formulas of its own that work on RAW rows:
// the cosine of q_quad_dist, the uint8 proxies of q_quad_proxy and the rerank's un-clamped dot.)
//
// Metric codes (include/pynnd_amd.h NND_METRIC_*): 0 sqeuclidean, 1 alt cosine, 2 alt dot, 3 alt inner product,
// 4 correlation, 5 alt hellinger, 6 proxy inner product.  The prep kernel turns every row into a "prepared" row whose inner
// products give the distance (DESIGN.md "Metrics"):
//   unit metrics (1, 2, 4, 5): rows L2-normalised after a per-metric transform (none / none / minus the row mean / sqrt);
//     nrm = 1 (non-zero row) or 0 (zero row); the trees split angularly;
//   norm metrics (0, 3, 6): rows centred on the column mean (0) or as given (3, 6); nrm = |x|^2; euclidean trees.
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

// The codes a kernel instance can meet, fixed at compile time: a conversion carries the branches of its family's codes and no
// others (in the unrolled epilogues of the Gram kernels every branch is paid per accumulator register: the six-way branch cost
// k_local_join16<32, 1|2, false> four VGPRs, DESIGN.md "Metrics").  A new kernel takes the narrowest family its launcher
// guarantees, NND_CODES_ANY if the code is only known at run time.  The values are the XM template arguments of the join
// kernels (join.hip), so they are part of those kernels' names.
enum nnd_metric_family {
    NND_CODES_01 = 0,   // sqeuclidean / cosine
    NND_CODES_0_5 = 1,  // every code but 6 (kernels where code 6 has an instance of its own, or is refused by the host)
    NND_CODE_6 = 2,     // proxy inner product alone: no branch on the code
    NND_CODES_ANY = 3,  // 0..6, by a branch on the code
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
enum nnd_hellinger_terms { NND_HELLINGER_F32, NND_HELLINGER_F64 };

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
NND_HD_INLINE double nnd_ref_dist(int metric, double dt, double ax, double ay) {
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
template <int FAM>
__device__ __forceinline__ float nnd_gram_to_dist(int metric, float g, float na, float nb) {
    constexpr bool m01 = FAM == NND_CODES_01;
    if constexpr (FAM == NND_CODE_6) return nnd_proxy_ip_dist(g, na, nb);
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
    if constexpr (FAM == NND_CODES_01) return 0.0f;
    if (!only6 && metric == 3) return n > 0.0f ? fminf(1.0f / n, NND_FLT_MAX) : NND_FLT_MAX;
    if (only6 || (FAM == NND_CODES_ANY && metric == 6)) return n > 0.0f ? fminf(__frsqrt_rn(n), NND_FLT_MAX) : NND_FLT_MAX;
    if (metric == 2 && n == 0.0f) return NND_FLT_MAX;
    return 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. Alt-space distance of the prepared rows a and b, one wave per pair (all 64 lanes take part): lane-strided partial sums,
// then nnd_wave_sum_f32; the difference form for sqeuclidean.  merge.hip (random init, proposals without a stored distance)
// and prune.hip (the pruning passes).
__device__ __forceinline__ float nnd_row_pair_dist(const float *__restrict__ xp, int dp, const float *__restrict__ nrm, int metric,
                                                   int64_t a, int64_t b) {
    const float *xa = xp + a * dp, *xb = xp + b * dp;
    float s = 0.0f;
    for (int j = nnd_lane(); j < dp; j += 64) {
        const float p = xa[j], q = xb[j];
        s += metric == 0 ? (p - q) * (p - q) : p * q;
    }
    s = nnd_wave_sum_f32(s);
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
