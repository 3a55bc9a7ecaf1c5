// leaf_plan.h -- which leaf-seeding kernels a round launches: the single statement of the table that leaf_join.hip
// (run_leaf_rounds) launches by and that tests/leaf_reference.py (forms) models.  Host code without HIP headers, like plan.h:
// tests/leaf_plan_cpu.cpp prints the whole table without a device.
#pragma once

enum nnd_leaf_kind { NND_LEAF_PLAIN, NND_LEAF_RB, NND_LEAF_SYM };  // k_leaf_join / k_leaf_join_rb / k_leaf_join_sym

// One kernel form.  flag: QW of k_leaf_join (quarter-wave merges, k <= 16), WIDE of k_leaf_join_rb (rows merged through LDS, k > 64).
struct nnd_leaf_form {
    nnd_leaf_kind kind;
    int nt, nw;  // the leaf's tile rows (at most nt * 16 points) and the waves of a workgroup
    bool flag;
    constexpr int threads() const { return nw * 64; }
    // a row-block workgroup takes 8 * nw rows of its leaf (k_leaf_join_rb: blockIdx.y); the other kinds the whole leaf
    constexpr int grid_y() const { return kind == NND_LEAF_RB ? (nt * 16 + nw * 8 - 1) / (nw * 8) : 1; }
};
enum nnd_leaf_form_id { NND_LF_QW4, NND_LF_QW44, NND_LF_QW5, NND_LF_QW6, NND_LF_P4, NND_LF_P5, NND_LF_P6, NND_LF_SYM6, NND_LF_SYM10,
                        NND_LF_RB8, NND_LF_RB10, NND_LF_RB16, NND_LF_W8, NND_LF_W10, NND_LF_W16, NND_LEAF_FORMS };
constexpr nnd_leaf_form nnd_leaf_forms[NND_LEAF_FORMS] = {
    {NND_LEAF_PLAIN, 4, 8, true}, {NND_LEAF_PLAIN, 4, 4, true}, {NND_LEAF_PLAIN, 5, 8, true}, {NND_LEAF_PLAIN, 6, 8, true},
    {NND_LEAF_PLAIN, 4, 8, false}, {NND_LEAF_PLAIN, 5, 8, false}, {NND_LEAF_PLAIN, 6, 8, false},
    {NND_LEAF_SYM, 6, 8, false}, {NND_LEAF_SYM, 10, 8, false},
    {NND_LEAF_RB, 8, 8, false}, {NND_LEAF_RB, 10, 8, false}, {NND_LEAF_RB, 16, 8, false},
    {NND_LEAF_RB, 8, 8, true}, {NND_LEAF_RB, 10, 8, true}, {NND_LEAF_RB, 16, 8, true},
};

// One launch over the round's leaf table: the PLAIN and SYM kernels take the leaves of m_lo < points <= nt * 16 (a workgroup whose
// leaf belongs to the other launch leaves at once); the row-block kernels take every leaf.
struct nnd_leaf_launch {
    nnd_leaf_form_id form;
    int m_lo;
};

// The launches of one cell of the table: n of them (1 or 2), in launch order.
struct nnd_leaf_cell {
    int n;
    nnd_leaf_launch launch[2];
};

// Rows: the longest run of the round, first row that holds it (the last one takes whatever is longer: runs are cut at 256).
// Columns: k <= 16 (quarter-wave merges) | 17..32 (two rows per wave) | 33..64 (a row per wave) | > 64 (rows merged through LDS).
//   65..80 points at k <= 16, the default leaf_size: leaves of <= 64 points -- 85 % of the leaves, 3/4 of the points -- get FOUR
//   waves and 21 KB of LDS, so that 6 of them are in flight per CU instead of 4.  The kernel is bound by exposed latency, not by a
//   pipe (profiles/r06_leaf_occupancy.log: 375 / 425 / 535 us per tree with 4 / 3 / 2 workgroups per CU).
//   97..160 points at k 17..32 (k = 30, the reference's default, gives leaf_size 150): the same split at 96 points.
constexpr struct {
    int longest;
    nnd_leaf_cell cell[4];
} nnd_leaf_table[] = {
    {64,  {{1, {{NND_LF_QW4, 0}}},                    {1, {{NND_LF_SYM6, 0}}},                     {1, {{NND_LF_P4, 0}}},   {1, {{NND_LF_W8, 0}}}}},
    {80,  {{2, {{NND_LF_QW44, 0}, {NND_LF_QW5, 64}}}, {1, {{NND_LF_SYM6, 0}}},                     {1, {{NND_LF_P5, 0}}},   {1, {{NND_LF_W8, 0}}}}},
    {96,  {{1, {{NND_LF_QW6, 0}}},                    {1, {{NND_LF_SYM6, 0}}},                     {1, {{NND_LF_P6, 0}}},   {1, {{NND_LF_W8, 0}}}}},
    {128, {{1, {{NND_LF_RB8, 0}}},                    {2, {{NND_LF_SYM6, 0}, {NND_LF_SYM10, 96}}}, {1, {{NND_LF_RB8, 0}}},  {1, {{NND_LF_W8, 0}}}}},
    {160, {{1, {{NND_LF_RB10, 0}}},                   {2, {{NND_LF_SYM6, 0}, {NND_LF_SYM10, 96}}}, {1, {{NND_LF_RB10, 0}}}, {1, {{NND_LF_W10, 0}}}}},
    {256, {{1, {{NND_LF_RB16, 0}}},                   {1, {{NND_LF_RB16, 0}}},                     {1, {{NND_LF_RB16, 0}}}, {1, {{NND_LF_W16, 0}}}}},
};
constexpr int NND_LEAF_ROWS = (int)(sizeof(nnd_leaf_table) / sizeof(nnd_leaf_table[0]));

// the launches of a round for rows of k neighbours when the longest run has `longest` points
static inline const nnd_leaf_cell &nnd_leaf_plan(int k, int longest) {
    int r = 0;
    while (r < NND_LEAF_ROWS - 1 && longest > nnd_leaf_table[r].longest) r++;
    return nnd_leaf_table[r].cell[k <= 16 ? 0 : k <= 32 ? 1 : k <= 64 ? 2 : 3];
}
