// exact_band_cpu.cpp -- the rounding-error bands of the exact search (pynndescent_amd/csrc/exact_band.h) against an emulation
// of the scan's float32 arithmetic on the CPU (tests/test_exact_band_cpu.py).
//
//   exact_band_cpu <metric code> <n> <d> <n_query_rows> <file of n * d float32>
//
// Emulated, as prep.hip / gram.h / metric.h compute it: the float32 preparation of the rows (code 0: minus the column mean;
// codes 1, 2, 4, 5: transform, f32 sum of squares, 1 / sqrtf, product; code 3: as given), the nrm word, the Gram value as ONE
// fmaf chain in the kernel's K order (exact_band.h), nnd_gram_to_dist's combination.  Compared with the float64 value of the
// ORIGINAL rows.  Prints the largest error / band ratio; exit status 1 if any pair exceeds its band.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "exact_band.h"

static bool unit_metric(int m) { return m == 1 || m == 2 || m == 4 || m == 5; }

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int metric = atoi(argv[1]), n = atoi(argv[2]), d = atoi(argv[3]), nq = atoi(argv[4]);
    const int dp = (d + 31) / 32 * 32;
    std::vector<float> x((size_t)n * d);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    fclose(f);

    // ---- preparation (prep.hip) ----
    std::vector<float> mean(dp, 0.0f), xp((size_t)n * dp, 0.0f), nrm(n, 0.0f);
    if (metric == 0)
        for (int j = 0; j < d; j++) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s += (double)x[(size_t)i * d + j];
            mean[j] = (float)(s / (double)n);
        }
    for (int i = 0; i < n; i++) {
        const float *src = &x[(size_t)i * d];
        float *dst = &xp[(size_t)i * dp];
        if (!unit_metric(metric)) {
            float s = 0.0f;
            for (int j = 0; j < d; j++) {
                const float v = metric == 0 ? src[j] - mean[j] : src[j];
                dst[j] = v;
                s += v * v;
            }
            nrm[i] = s;
        } else {
            double mu = 0.0;
            if (metric == 4) {
                for (int j = 0; j < d; j++) mu += (double)src[j];
                mu /= (double)d;
            }
            float s = 0.0f;
            for (int j = 0; j < d; j++) {
                const float v = metric == 4 ? (float)((double)src[j] - mu) : metric == 5 ? sqrtf(src[j]) : src[j];
                dst[j] = v;
                s += v * v;
            }
            const float inv = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
            for (int j = 0; j < d; j++) dst[j] *= inv;
            nrm[i] = s > 0.0f ? 1.0f : 0.0f;
        }
    }

    // ---- every pair (query row a < nq, data row b) ----
    double worst = 0.0;
    long long bad = 0, pairs = 0;
    for (int a = 0; a < nq; a++) {
        const float *pa = &xp[(size_t)a * dp], *ra = &x[(size_t)a * d];
        double mua = 0.0;
        if (metric == 4) {
            for (int j = 0; j < d; j++) mua += (double)ra[j];
            mua /= (double)d;
        }
        for (int b = 0; b < n; b++) {
            const float *pb = &xp[(size_t)b * dp], *rb = &x[(size_t)b * d];
            // the Gram value: one fmaf chain, 16-float group t outermost, then the component e of a 16-byte chunk, then the
            // MFMA's k index c (the lane group) innermost
            float g = 0.0f;
            for (int t = 0; t < dp / 16; t++)
                for (int e = 0; e < 4; e++)
                    for (int c = 0; c < 4; c++) {
                        const int i = 16 * t + 4 * c + e;
                        g = fmaf(pa[i], pb[i], g);
                    }
            // the float64 value of the original rows
            double mub = 0.0;
            if (metric == 4) {
                for (int j = 0; j < d; j++) mub += (double)rb[j];
                mub /= (double)d;
            }
            double s = 0.0, dot = 0.0, dot32 = 0.0, ax = 0.0, ay = 0.0;
            for (int j = 0; j < d; j++) {
                const double u = (double)ra[j] - mua, v = (double)rb[j] - mub;
                s += (u - v) * (u - v);
                if (metric == 5) {
                    dot += sqrt(u * v);
                    dot32 += (double)sqrtf((float)u * (float)v);  // the reference's float32 terms (finalize.hip, exact.hip)
                    ax += u;
                    ay += v;
                } else {
                    dot += u * v;
                    ax += u * u;
                    ay += v * v;
                }
            }
            double err, band;
            if (metric == 0) {
                float kv = nrm[a] + nrm[b] - 2.0f * g;  // nnd_gram_to_dist, clamped at 0
                kv = kv > 0.0f ? kv : 0.0f;
                err = fabs((double)kv - s);
                band = nnd_exact_band_sqeuclid(dp, (double)nrm[a], (double)nrm[b]);
            } else if (metric == 3) {
                err = fabs((double)g - dot);
                band = nnd_exact_band_inner(dp, (double)nrm[a], (double)nrm[b]);
            } else {
                if (!(ax > 0.0) || !(ay > 0.0)) continue;  // zero rows: flagged in nrm, no Gram value is read
                const double den = sqrt(ax * ay);
                err = fabs((double)g - dot / den);
                if (metric == 5) err = fmax(err, fabs((double)g - dot32 / den));
                band = nnd_exact_band_unit(d, dp);
                if (metric == 4) {  // ranked by 1 - g, clamped at 0
                    float kv = 1.0f - g;
                    kv = kv > 0.0f ? kv : 0.0f;
                    const double r = 1.0 - dot / den;
                    const double e2 = fabs((double)kv - (r > 0.0 ? r : 0.0)) / nnd_exact_band_correlation(d, dp) * band;
                    err = fmax(err, e2);
                }
            }
            pairs++;
            const double ratio = err / band;
            if (!(ratio <= 1.0)) bad++;
            if (ratio > worst) worst = ratio;
        }
    }
    printf("pairs %lld worst %.6g bad %lld\n", pairs, worst, bad);
    return bad ? 1 : 0;
}
