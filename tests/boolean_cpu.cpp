// boolean_cpu.cpp -- the float64 conversion of the boolean family (pynndescent_amd/csrc/metric.h nnd_bool_dist_f64, through
// nnd_ref_dist<NND_CODES_BOOL>) on a CPU, driven by test_boolean_metrics_cpu.py: the header is compiled by the host compiler,
// without HIP headers.  argv[1] = the largest column count D.  For every code 8..16 and every consistent count tuple with
// d <= D -- 0 <= a, b <= d and max(0, a + b - d) <= c <= min(a, b) -- one line "<code> <c> <a> <b> <d> <distance>", the
// distance as a C99 hex double.  nnd_ref_acc<NND_CODES_BOOL> is exercised too: the counts are accumulated from indicator
// pairs laid out as c x (1,1), (a - c) x (1,0), (b - c) x (0,1) and the rest (0,0), with non-unit non-zero values.
#include <stdio.h>
#include <stdlib.h>

#include "metric.h"

int main(int argc, char **argv) {
    const int D = argc > 1 ? atoi(argv[1]) : 12;
    for (int code = NND_BOOL_FIRST; code <= NND_BOOL_LAST; code++)
        for (int d = 1; d <= D; d++)
            for (int a = 0; a <= d; a++)
                for (int b = 0; b <= d; b++)
                    for (int c = (a + b > d ? a + b - d : 0); c <= (a < b ? a : b); c++) {
                        double dot = 0.0, nx = 0.0, ny = 0.0;
                        for (int t = 0; t < d; t++) {
                            const double xv = t < a ? 0.25 * (t + 1) : 0.0;                          // the first a columns of x
                            const double yv = (t < c || (t >= a && t < a + b - c)) ? -3.0 : 0.0;     // c shared, b - c of its own
                            nnd_ref_acc<NND_CODES_BOOL, NND_HELLINGER_F64>(code, xv, yv, dot, nx, ny);
                        }
                        if (dot != c || nx != a || ny != b) {
                            fprintf(stderr, "counts differ: code %d c %d a %d b %d d %d -> %g %g %g\n", code, c, a, b, d, dot, nx, ny);
                            return 1;
                        }
                        printf("%d %d %d %d %d %a\n", code, c, a, b, d, nnd_ref_dist<NND_CODES_BOOL>(code, dot, nx, ny, (double)d));
                    }
    return 0;
}
