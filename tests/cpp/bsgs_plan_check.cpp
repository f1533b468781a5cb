// bsgs_plan_check -- crc_bsgs_plan / crc_bsgs_elements / crc_diag_plan (crcnn_amd/host/diag_plan.h) on matrices read from a text file, printed for
// tests/test_bsgs_cpu.py to compare with the Python planner.
//   bsgs_plan_check <file>        file: any number of cases "M n B out in" followed by out * in integers
// Per case: "bad <number of elements>" where the planner refuses, else four lines: "baby ..", "giant ..", "rows .." (all [giant][baby][n] words), "elts ..".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "diag_plan.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: bsgs_plan_check <file>\n"); return 1; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "bsgs_plan_check: cannot open %s\n", argv[1]); return 1; }
    int M, n, B, out, in;
    while (fscanf(f, "%d %d %d %d %d", &M, &n, &B, &out, &in) == 5) {
        if (out < 0 || in < 0 || out > 4096 || in > 4096) { fclose(f); return 2; }
        std::vector<std::vector<int64_t>> W((size_t)out, std::vector<int64_t>((size_t)in));
        for (auto &r : W) for (auto &v : r) if (fscanf(f, "%" SCNd64, &v) != 1) { fclose(f); return 2; }
        std::vector<int> baby{-7}, giant{-7};                        // (a refusal must leave them alone)
        std::vector<int64_t> rows{-7};
        if (!crc_bsgs_plan(W, M, n, B, baby, giant, rows)) {
            if (baby != std::vector<int>{-7} || giant != std::vector<int>{-7} || rows != std::vector<int64_t>{-7}) return 3;
            printf("bad %zu\n", crc_bsgs_elements(M, B, n).size());     // (no elements either, unless only the matrix is at fault)
            continue;
        }
        if (rows.size() != baby.size() * giant.size() * (size_t)n) return 4;
        printf("baby"); for (int b : baby) printf(" %d", b);
        printf("\ngiant"); for (int g : giant) printf(" %d", g);
        printf("\nrows"); for (int64_t v : rows) printf(" %" PRId64, v);
        printf("\nelts"); for (uint64_t e : crc_bsgs_elements(M, B, n)) printf(" %" PRIu64, e);
        printf("\n");
        if (B == M) {                                                // the flat plan is the split at B = M
            std::vector<int> steps; std::vector<int64_t> flat;
            if (!crc_diag_plan(W, M, n, steps, flat) || steps != baby || flat != rows) return 5;
        }
    }
    fclose(f);
    return 0;
}
