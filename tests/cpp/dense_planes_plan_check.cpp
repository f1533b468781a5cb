// dense_planes_plan_check -- crc_dense_planes_plan / crc_dense_planes_fold (crcnn_amd/host/diag_plan.h) on cases read from a text file, printed for
// tests/test_dense_planes_cpu.py to compare with the Python planner.
//   dense_planes_plan_check <file>        file: any number of cases "n M P O Cin t", then P input slots, O output slots and O * Cin * P integers
// Per case: "bad" where the planner refuses, else three lines: "steps ..", "elts ..", "fold .." ([R][Cin][n]).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "diag_plan.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: dense_planes_plan_check <file>\n"); return 1; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "dense_planes_plan_check: cannot open %s\n", argv[1]); return 1; }
    int n, M, NP, O, Cin;
    int64_t t;
    while (fscanf(f, "%d %d %d %d %d %" SCNd64, &n, &M, &NP, &O, &Cin, &t) == 6) {
        if (NP < 0 || O < 0 || Cin < 0 || NP > 4096 || O > 4096 || Cin > 64) { fclose(f); return 2; }
        std::vector<int> in((size_t)NP), out((size_t)O);
        for (auto &v : in) if (fscanf(f, "%d", &v) != 1) { fclose(f); return 2; }
        for (auto &v : out) if (fscanf(f, "%d", &v) != 1) { fclose(f); return 2; }
        std::vector<int64_t> w((size_t)O * Cin * NP);
        for (auto &v : w) if (fscanf(f, "%" SCNd64, &v) != 1) { fclose(f); return 2; }
        DensePlanesPlan P;
        P.steps = {-7};                                                 // (a refusal must leave the plan alone)
        if (!crc_dense_planes_plan(n, M, in, out, P)) {
            if (P.steps != std::vector<int>{-7} || !P.elements.empty() || !P.out_at.empty() || P.n) return 3;
            printf("bad\n");
            continue;
        }
        std::vector<int64_t> rows{-7};
        if (crc_dense_planes_fold(P, std::vector<int64_t>(w.size() + 1), Cin, t, rows) || rows != std::vector<int64_t>{-7}) return 4;   // a wrong size
        if (crc_dense_planes_fold(P, w, Cin, 1, rows) || crc_dense_planes_fold_step(P, w, Cin, t, (int)P.steps.size(), rows) || rows != std::vector<int64_t>{-7}) return 4;
        if (!crc_dense_planes_fold(P, w, Cin, t, rows) || rows.size() != P.steps.size() * (size_t)Cin * n) return 5;
        if (P.elements.size() != P.steps.size() || P.steps.empty()) return 6;
        printf("steps"); for (int s : P.steps) printf(" %d", s);
        printf("\nelts"); for (uint64_t e : P.elements) printf(" %" PRIu64, e);
        printf("\nfold"); for (int64_t v : rows) printf(" %" PRId64, v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
