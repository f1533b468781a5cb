// bsgs_plan_sanitize_main -- crc_bsgs_plan and crc_bsgs_elements (crcnn_amd/host/diag_plan.h) under the host address and undefined-behaviour sanitizers: a
// stand-alone program, no engine and no device.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I crcnn_amd/host tools/bsgs_plan_sanitize_main.cpp -o bsgs_plan_sanitize
// Walks every M <= 64, every n from 2 M to 8 M, every B from 0 to 2 M (valid and not), dense, ragged, sparse, empty and oversized matrices with entries up to the
// int64 limits, and checks the plan against the product in 128-bit integers: y[i] = Sum_{j, b} rows[j][b][i + giant_j] x[i + giant_j + baby_b] = (W x)[i mod M].
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
    for (int M = 0; M <= 64; M++)
        for (int n : {2 * M, 4 * M, 8 * M, M, 1})
            for (int B = 0; B <= 2 * M + 1; B++)
                for (int kind = 0; kind < 5; kind++) {
                    const int out = kind == 4 ? M + 1 : kind == 1 ? (M + 1) / 2 : M;
                    std::vector<std::vector<int64_t>> W((size_t)(out > 0 ? out : 0));
                    for (size_t i = 0; i < W.size(); i++) {
                        W[i].resize(kind == 1 ? (i * 7) % (size_t)(M + 1) : (size_t)M);                  // ragged rows
                        for (auto &v : W[i]) v = kind == 3 ? 0 : kind == 2 && rnd() % 4 ? 0 : (int64_t)rnd();   // sparse, zero, or any int64
                    }
                    std::vector<int> baby, giant; std::vector<int64_t> rows;
                    const bool pow2M = M >= 1 && !(M & (M - 1)), pow2B = B >= 1 && !(B & (B - 1));
                    const bool valid = pow2M && pow2B && B <= M && n >= 2 && M <= n / 2 && kind != 4;
                    if (crc_bsgs_plan(W, M, n, B, baby, giant, rows) != valid) { fprintf(stderr, "admission M %d n %d B %d kind %d\n", M, n, B, kind); return 1; }
                    const std::vector<uint64_t> elts = crc_bsgs_elements(M, B, n);
                    if (!valid) {
                        refusals++;
                        if (kind != 4 && !elts.empty()) return 2;
                        continue;
                    }
                    plans++;
                    if (elts.size() != (size_t)(B + M / B - 2) || rows.size() != baby.size() * giant.size() * (size_t)n) return 3;
                    for (uint64_t e : elts) if (!(e & 1) || e >= 2 * (uint64_t)n || e == 1) return 4;
                    std::vector<int64_t> x((size_t)M);
                    for (auto &v : x) v = (int64_t)(rnd() >> 34);
                    const int h = n / 2;
                    for (int i = 0; i < n; i++) {                                       // slot i: row i / h of n/2 slots, a rotation stays inside its row
                        i128 got = 0, want = 0;
                        for (size_t j = 0; j < giant.size(); j++)
                            for (size_t b = 0; b < baby.size(); b++) {
                                const int at = i / h * h + (i % h + giant[j]) % h;
                                got += (i128)rows[(j * baby.size() + b) * (size_t)n + at] * x[(size_t)((at % h + baby[b]) % h % M)];
                            }
                        const size_t r = (size_t)(i % M);
                        if (r < W.size()) for (size_t c = 0; c < W[r].size(); c++) want += (i128)W[r][c] * x[c];
                        if (got != want) { fprintf(stderr, "product M %d n %d B %d kind %d slot %d\n", M, n, B, kind, i); return 5; }
                    }
                }
    printf("ok %ld %ld\n", plans, refusals);
    return 0;
}
