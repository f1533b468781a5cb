// dense_planes_plan_sanitize_main -- crc_dense_planes_plan and crc_dense_planes_fold (crcnn_amd/host/diag_plan.h) under the host address and undefined-behaviour
// sanitizers: a stand-alone program, no engine and no device.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I crcnn_amd/host tools/dense_planes_plan_sanitize_main.cpp -o dense_planes_plan_sanitize
// Walks rings n <= 512, every power-of-two and some other M, random input and output slot lists (valid, empty, duplicated, out of range), 1 to 3 channels,
// weights up to the int64 limits, and checks the plan on integer slots: with the inputs at their slots of every period and random junk elsewhere,
// Sum_j Sum_c rows[j][c][(i + steps[j]) mod n/2] x_c[(i + steps[j]) mod n/2] at EVERY slot i of both rows equals the layer's output where i mod M is an output
// slot and 0 elsewhere, mod t, in 128-bit integers.
// Prints "ok <plans> <refusals>"; any other exit is a failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "diag_plan.h"

typedef __int128 i128;
static uint64_t state = 88172645463325252ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

int main()
{
    long plans = 0, refusals = 0;
    const int64_t ts[3] = {65537, 2, ((int64_t)1 << 61) - 1};
    for (int n : {0, 2, 6, 16, 64, 512})
        for (int M : {0, 1, 2, 3, 8, 32, 48, 256, 512})
            for (int trial = 0; trial < 12; trial++) {
                const int span = M > 0 ? M : 4;
                const int NP = trial == 0 ? 0 : 1 + (int)(rnd() % (uint64_t)(span < 9 ? span : 9)), O = trial == 1 ? 0 : 1 + (int)(rnd() % (uint64_t)(span < 7 ? span : 7));
                std::vector<int> in, out;
                auto draw = [&](std::vector<int> &v, int cnt) {             // distinct slots of [0, span), in random order
                    while ((int)v.size() < cnt) {
                        const int s = (int)(rnd() % (uint64_t)span);
                        bool seen = false;
                        for (int w : v) seen = seen || w == s;
                        if (!seen) v.push_back(s);
                    }
                };
                draw(in, NP); draw(out, O);
                if (trial == 2 && !in.empty()) in.push_back(in[0]);        // a duplicate
                if (trial == 3 && !out.empty()) out.push_back(out[0]);
                if (trial == 4) in.push_back(span);                         // outside [0, M)
                if (trial == 5) out.push_back(-1);
                const bool pow2 = M >= 1 && !(M & (M - 1)) && n >= 2 && !(n & (n - 1)) && M <= n / 2;
                const bool valid = pow2 && !in.empty() && !out.empty() && trial > 5;
                DensePlanesPlan P;
                if (crc_dense_planes_plan(n, M, in, out, P) != valid) { fprintf(stderr, "admission n %d M %d trial %d\n", n, M, trial); return 1; }
                if (!valid) { refusals++; if (P.n || !P.steps.empty() || !P.out_at.empty()) return 2; continue; }
                plans++;
                const int R = (int)P.steps.size(), Cin = 1 + (int)(plans % 3), h = n / 2;
                if (R < 1 || R > (int)(in.size() * out.size()) || (int)P.elements.size() != R) return 3;
                for (int j = 0; j < R; j++) {
                    if (P.steps[j] < 0 || P.steps[j] >= M || (j && P.steps[j] <= P.steps[j - 1])) return 4;
                    if (!(P.elements[j] & 1) || P.elements[j] >= 2 * (uint64_t)n || (P.steps[j] == 0) != (P.elements[j] == 1)) return 4;
                }
                const int64_t t = ts[plans % 3];
                std::vector<int64_t> w(out.size() * (size_t)Cin * in.size()), rows;
                for (auto &v : w) v = (int64_t)rnd();                       // any int64
                w[0] = INT64_MIN; w[w.size() - 1] = INT64_MAX;
                if (crc_dense_planes_fold(P, w, Cin + 1, t, rows) || crc_dense_planes_fold(P, w, Cin, 1, rows) || crc_dense_planes_fold_step(P, w, Cin, t, R, rows)
                    || crc_dense_planes_fold_step(P, w, Cin, t, -1, rows) || !rows.empty()) return 5;
                if (!crc_dense_planes_fold(P, w, Cin, t, rows) || rows.size() != (size_t)R * Cin * n) return 6;
                for (int64_t v : rows) if (v < 0 || v >= t) return 7;
                // planes [Cin][n]: junk below t everywhere, the inputs at their slots of every period
                std::vector<int64_t> xs((size_t)Cin * in.size()), x((size_t)Cin * n);
                for (auto &v : xs) v = (int64_t)(rnd() % (uint64_t)t);
                for (int c = 0; c < Cin; c++) {
                    std::vector<int64_t> per((size_t)M);
                    for (auto &v : per) v = (int64_t)(rnd() % (uint64_t)t);
                    for (size_t p = 0; p < in.size(); p++) per[(size_t)in[p]] = xs[(size_t)c * in.size() + p];
                    for (int i = 0; i < n; i++) x[(size_t)c * n + i] = per[(size_t)(i % M)];
                }
                for (int half = 0; half < 2; half++)
                    for (int i = 0; i < h; i++) {
                        i128 got = 0, want = 0;
                        for (int j = 0; j < R; j++)
                            for (int c = 0; c < Cin; c++) {
                                const size_t at = (size_t)c * n + half * h + (i + P.steps[j]) % h;
                                got = (got + (i128)rows[(size_t)j * Cin * n + at] * x[at]) % t;
                            }
                        const int o = P.out_at[(size_t)(i % M)];
                        if (o >= 0)
                            for (int c = 0; c < Cin; c++)
                                for (size_t p = 0; p < in.size(); p++) {
                                    int64_t wv = w[((size_t)o * Cin + c) * in.size() + p] % t;
                                    if (wv < 0) wv += t;
                                    want = (want + (i128)wv * xs[(size_t)c * in.size() + p]) % t;
                                }
                        if (got != want) { fprintf(stderr, "slots n %d M %d trial %d slot %d\n", n, M, trial, half * h + i); return 8; }
                    }
            }
    printf("ok %ld %ld\n", plans, refusals);
    return 0;
}
