// conv_slots_geom_plan_check -- crc_conv_slots_plan_geom / crc_conv_slots_fold_geom / crc_conv_slots_mask_slots (crcnn_amd/host/diag_plan.h) on cases read from a
// text file, printed for tests/test_conv_slots_pad_cpu.py to compare with the Python planner.
//   conv_slots_geom_plan_check <file>   file: any number of cases "n M pitch origin H W fh fw dil pad stride pool pool_stride Cout Cin t" followed by
//                                       Cout * Cin * fh * fw integers
// Per case: "bad" where the planner refuses, else six lines: "steps ..", "elts ..", "geom out_h out_w out_dil clean", "valid ..", "fold .." ([Cout][Cin][T]),
// "mask .." (the slots of the first period that are 1; the program checks that every period repeats them).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "diag_plan.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: conv_slots_geom_plan_check <file>\n"); return 1; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "conv_slots_geom_plan_check: cannot open %s\n", argv[1]); return 1; }
    int n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps, Cout, Cin;
    int64_t t;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %" SCNd64, &n, &M, &pitch, &origin, &H, &W, &fh, &fw, &dil, &pad, &stride, &pool, &ps, &Cout, &Cin,
                  &t) == 16) {
        if (Cout < 0 || Cin < 0 || fh < 0 || fw < 0 || Cout > 64 || Cin > 64 || fh > 64 || fw > 64) { fclose(f); return 2; }
        std::vector<int64_t> w((size_t)Cout * Cin * fh * fw);
        for (auto &v : w) if (fscanf(f, "%" SCNd64, &v) != 1) { fclose(f); return 2; }
        ConvSlotsGeomPlan P;
        P.steps = {-7};                                                 // (a refusal must leave the plan alone)
        if (!crc_conv_slots_plan_geom(n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps, P)) {
            if (P.steps != std::vector<int>{-7} || !P.elements.empty() || !P.valid.empty() || P.n) return 3;
            printf("bad\n");
            continue;
        }
        std::vector<int64_t> fold{-7};
        if (crc_conv_slots_fold_geom(P, std::vector<int64_t>(w.size() + 1), Cout, Cin, t, fold) || fold != std::vector<int64_t>{-7}) return 4;   // a wrong size
        if (!crc_conv_slots_fold_geom(P, w, Cout, Cin, t, fold) || fold.size() != (size_t)Cout * Cin * P.steps.size()) return 5;
        if (P.elements.size() != P.steps.size() || P.valid.size() != (size_t)P.out_h * P.out_w) return 6;
        const std::vector<int64_t> mask = crc_conv_slots_mask_slots(P);
        if (mask.size() != (size_t)n) return 7;
        for (int i = 0; i < n; i++) if ((mask[i] != 0 && mask[i] != 1) || mask[i] != mask[i % M]) return 8;
        printf("steps"); for (int s : P.steps) printf(" %d", s);
        printf("\nelts"); for (uint64_t e : P.elements) printf(" %" PRIu64, e);
        printf("\ngeom %d %d %d %d", P.out_h, P.out_w, P.out_dil, P.needs_clean_input ? 1 : 0);
        printf("\nvalid"); for (int v : P.valid) printf(" %d", v);
        printf("\nfold"); for (int64_t v : fold) printf(" %" PRId64, v);
        printf("\nmask"); for (int i = 0; i < M; i++) if (mask[i]) printf(" %d", i);
        printf("\n");
    }
    fclose(f);
    return 0;
}
