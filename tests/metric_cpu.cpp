// metric_cpu.cpp -- the float64 "sums to distance" function of pynndescent_amd/csrc/metric.h on a CPU (driven by
// test_metric_cpu.py): the header is compiled by the host compiler, without HIP headers, under AddressSanitizer and UBSan.
// stdin: one pair per line, "<metric code> <dot> <ax> <ay>" (C99 hex doubles; code 0: the squared-difference sum as <dot>).
// stdout: per line the float32 bit pattern of nnd_ref_dist<NND_CODES_ANY>.  Every narrower family that holds the code must
// give the same double: a disagreement prints the line to stderr and the exit status is 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "metric.h"

static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    char line[256];
    int bad = 0;
    while (fgets(line, sizeof line, stdin)) {
        char *p = line;
        const int metric = (int)strtol(p, &p, 10);
        const double dt = strtod(p, &p), ax = strtod(p, &p), ay = strtod(p, &p);
        const double r = nnd_ref_dist<NND_CODES_ANY>(metric, dt, ax, ay);
        bool ok = true;
        if (metric <= 1) ok = ok && same(r, nnd_ref_dist<NND_CODES_01>(metric, dt, ax, ay));
        if (metric <= 5) ok = ok && same(r, nnd_ref_dist<NND_CODES_0_5>(metric, dt, ax, ay));
        if (metric == 6) ok = ok && same(r, nnd_ref_dist<NND_CODE_6>(metric, dt, ax, ay));
        if (!ok) {
            fprintf(stderr, "families disagree: %s", line);
            bad = 1;
        }
        const float f = (float)r;
        uint32_t bits;
        memcpy(&bits, &f, sizeof bits);
        printf("%08x\n", bits);
    }
    return bad;
}
