// exact_band.h -- how far the f32 kernel distance of the exact search's scan (exact.hip k_exact_scan) can be from the
// exact distance of the ORIGINAL rows.  The certificate of k_exact_refine rests on these bounds (DESIGN.md "Exact search"
// derives them); they are rigorous and deliberately crude: a wider band only sends more rows to the float64 tier.
//
// No HIP includes: the host compiler builds this header too (tests/test_exact_band_cpu.py emulates the scan's arithmetic on
// the CPU and checks every bound against float64).
//
// What the scan computes for a query row a and a data row b of the prepared (n, dp) matrix:
//   g   = the Gram value <a, b>: one f32 fmaf chain over the dp coordinates, g = fmaf(a[i], b[i], g) starting from 0, in the
//         order i = 16 t + 4 c + e with t (16-float group) outermost, then e = 0..3 (the component of a 16-byte chunk), then
//         c = 0..3 (the lane group of the MFMA, its k index) innermost: v_mfma_f32_16x16x4_f32 is bitwise such a chain.
//         Rows wider than the LDS tile are contracted chunk after chunk into the same accumulators: t simply runs on.
//         (The bounds below hold for ANY order of the chain; the order is stated so that the emulation matches bit for bit.)
//   nrm = prep.hip's norm word: sum of squares of the prepared coordinates in f32 (codes 0, 3), 1 / 0 for the unit rows
//   the distance by nnd_gram_to_dist (metric.h)
// and what stands between a prepared coordinate and the original one: ONE f32 rounding for code 0 (raw - mean[j]), none for
// code 3, and for the unit rows (codes 1, 2, 4, 5) the transform (none / none / minus the float64 row mean / sqrtf), the f32
// sum of squares, 1 / sqrtf and one multiplication.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NND_BAND_FN __host__ __device__ static inline
#else
#define NND_BAND_FN static inline
#endif

#define NND_EXACT_U 5.9604644775390625e-08 /* 2^-24: unit roundoff of float32 */
#define NND_EXACT_DP_MAX 8192              /* above it dp * u is no longer small against 1: every row takes the float64 tier */

// code 0, DISTANCE space: |kernel value - sum (a_j - b_j)^2 of the raw rows| <= band.  na, nb: the two nrm words (f32 values
// of |a - mean|^2, |b - mean|^2).  Terms, in units of u (|A|^2 + |B|^2): dp + 1 for the two norms, dp for twice the Gram
// chain (2 |<A,B>| <= |A|^2 + |B|^2), 4 for the two roundings of na + nb - 2 g, 4 for the rounding of the centred
// coordinates -- 2 dp + 9, taken as 2 dp + 16; the factor 1.01 pays for the second-order terms and for reading the norms off
// their rounded f32 values (dp u <= 2^-11).
NND_BAND_FN double nnd_exact_band_sqeuclid(int dp, double na, double nb) {
    if (dp > NND_EXACT_DP_MAX) return INFINITY;
    return (2.0 * dp + 16.0) * NND_EXACT_U * 1.01 * (na + nb);
}
// code 3, GRAM space: |g - <a, b>| <= band (rows as given: no rounding before the chain).  na, nb: the nrm words.
NND_BAND_FN double nnd_exact_band_inner(int dp, double na, double nb) {
    if (dp > NND_EXACT_DP_MAX) return INFINITY;
    return (dp + 2.0) * NND_EXACT_U * 1.01 * sqrt(na * nb);
}
// codes 1, 2, 4, 5, GRAM space: |g - <a, b> / (|a| |b|)| <= band for the transformed rows a, b in exact arithmetic (cosine of
// the raw rows / of the row-centred rows / Bhattacharyya coefficient).  In units of u: dp for the chain over unit rows, d + 7
// for the two normalisations ((d + 1) / 2 for each sum of squares under the square root, 3 for 1 / sqrtf and the product),
// 8 for the transforms (one rounding per coordinate, and the float32 sqrtf(x y) terms of the reference's hellinger) --
// dp + d + 15, doubled and rounded up.
NND_BAND_FN double nnd_exact_band_unit(int d, int dp) {
    if (dp > NND_EXACT_DP_MAX) return INFINITY;
    return (2.0 * dp + 2.0 * d + 64.0) * NND_EXACT_U;
}
// correlation is ranked by 1 - g: the subtraction rounds once more (and is clamped at 0, towards the exact value)
NND_BAND_FN double nnd_exact_band_correlation(int d, int dp) { return nnd_exact_band_unit(d, dp) + 2.0 * NND_EXACT_U; }
// the -log2 metrics are certified in Gram space.  What the scan left out has a kernel distance -log2f(g) >= T; with the
// hardware logarithm trusted to |log2f(x) - log2(x)| <= 2^-20 max(1, |log2 x|) (the ISA gives 1 ulp) its Gram value is at most
// this:
NND_BAND_FN double nnd_exact_gram_of_log_dist(double t) {
    const double slack = 9.5367431640625e-07 * (t > 1.0 ? t : 1.0);
    return exp2(-(t - slack));
}
// ... and under 1 / g >= T (one division, rounded once) at most this:
NND_BAND_FN double nnd_exact_gram_of_inverse_dist(double t) { return (1.0 + 4.0 * NND_EXACT_U) / t; }
// The boolean family (codes 8..16), DISTANCE space.  The scan's Gram value and both norm words are counts of indicator rows:
// integers below 2^24, exact in float32 in any summation order.  So the band is that of the conversion alone (metric.h
// nnd_bool_dist).  The eight rational formulas are quotients of two sums of non-negative terms, every difference in them one of
// integers that float32 holds exactly: at most three roundings in the denominator (yule: two products and a sum; below 2^24,
// as at every d below 2^12, none at all) and one in the numerator, then ONE correctly rounded division -- (1 + u)^5 relative,
// taken as 8 u of the value.  (With exact operands the correctly rounded quotient is monotone in the exact one, and the band
// is needed only to decide ties strictly; a row whose k-th exact distance EQUALS what the scan left out goes to the float64 tier.)
NND_BAND_FN double nnd_exact_band_bool_rational(double t) { return 8.0 * NND_EXACT_U * t; }
// jaccard is -log2f of one correctly rounded quotient in (0, 1]: the quotient's rounding moves the logarithm by at most
// u / ln 2 < 2 u, and the hardware logarithm is trusted as above, 2^-20 max(1, |log2 x|).  FLT_MAX (no common column) is exact.
NND_BAND_FN double nnd_exact_band_jaccard(double t) {
    if (t >= 3.0e38) return 0.0;
    return 9.5367431640625e-07 * (t > 1.0 ? t : 1.0) + 2.0 * NND_EXACT_U;
}
