// leaf_plan_cpu.cpp -- the leaf-seeding table (pynndescent_amd/csrc/leaf_plan.h) on a CPU, driven by test_leaf_plan_cpu.py: for every
// k in 1..256 and every longest run in 2..256 one line "k longest" followed by, per launch, " name m_lo grid_y threads", the name
// spelled as tests/leaf_reference.py (forms) spells it: without the family argument.  Host compiler only: the header needs no HIP.
#include <stdio.h>

#include "leaf_plan.h"

static void print_name(const nnd_leaf_form &f) {
    if (f.kind == NND_LEAF_PLAIN) printf("k_leaf_join<%d,%d,64%s>", f.nt, f.nw, f.flag ? ",true" : "");
    else printf("%s<%d,%d%s>", f.kind == NND_LEAF_RB ? "k_leaf_join_rb" : "k_leaf_join_sym", f.nt, f.nw, f.flag ? ",true" : "");
}

int main() {
    for (int k = 1; k <= 256; k++)
        for (int longest = 2; longest <= 256; longest++) {
            const nnd_leaf_cell &plan = nnd_leaf_plan(k, longest);
            printf("%d %d", k, longest);
            for (int i = 0; i < plan.n; i++) {
                const nnd_leaf_form &f = nnd_leaf_forms[plan.launch[i].form];
                printf(" ");
                print_name(f);
                printf(" %d %d %d", plan.launch[i].m_lo, f.grid_y(), f.threads());
            }
            printf("\n");
        }
    return 0;
}
