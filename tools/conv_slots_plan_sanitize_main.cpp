// conv_slots_plan_sanitize_main -- crc_conv_slots_plan and crc_conv_slots_fold (crcnn_amd/host/diag_plan.h) under the host address and undefined-behaviour
// sanitizers: a stand-alone program, no engine and no device.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I crcnn_amd/host tools/conv_slots_plan_sanitize_main.cpp -o conv_slots_plan_sanitize
// Walks rings n <= 512, every power-of-two and some other M, plane shapes, pitches, windows, dilations and pools (valid and not), weights up to the int64 limits,
// and checks the plan on integer slots: with the plane tiled with period M and random junk elsewhere, Sum_tau fold[tau] x[(slot + steps[tau]) mod n/2] at every
// valid slot of every period equals the convolution followed by the sum pool, mod t, in 128-bit integers.
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
            for (int H = 0; H <= 6; H++)
                for (int W = 0; W <= 6; W += 1 + (H & 1))
                    for (int pitch : {W - 1, W, W + 3})
                        for (int fh = 0; fh <= 3; fh++)
                            for (int fw = 1; fw <= 3; fw += 2)
                                for (int dil = 0; dil <= 3; dil++)
                                    for (int pool = 0; pool <= 3; pool++) {
                                        ConvSlotsPlan P;
                                        const bool pow2 = M >= 1 && !(M & (M - 1)) && n >= 2 && !(n & (n - 1)) && M <= n / 2;
                                        const bool pos = pitch >= 1 && H >= 1 && W >= 1 && fh >= 1 && fw >= 1 && dil >= 1 && pool >= 1;
                                        bool valid = pow2 && pos && W <= pitch && fh <= H && fw <= W && dil * ((H - 1) * pitch + W - 1) < M;
                                        valid = valid && (H - fh + 1) / pool >= 1 && (W - fw + 1) / pool >= 1
                                                && dil * ((fh + pool - 2) * pitch + fw + pool - 2) < n / 2;
                                        if (crc_conv_slots_plan(n, M, pitch, H, W, fh, fw, dil, pool, P) != valid) {
                                            fprintf(stderr, "admission n %d M %d pitch %d H %d W %d f %d %d dil %d pool %d\n", n, M, pitch, H, W, fh, fw, dil, pool);
                                            return 1;
                                        }
                                        if (!valid) { refusals++; if (P.n || !P.steps.empty()) return 2; continue; }
                                        plans++;
                                        const int T = (fh + pool - 1) * (fw + pool - 1), Cout = 2, Cin = 2, h = n / 2;
                                        if ((int)P.steps.size() != T || (int)P.elements.size() != T || P.elements[0] != 1 || P.out_dil != dil * pool) return 3;
                                        for (uint64_t e : P.elements) if (!(e & 1) || e >= 2 * (uint64_t)n) return 4;
                                        const int64_t t = ts[plans % 3];
                                        std::vector<int64_t> w((size_t)Cout * Cin * fh * fw), fold;
                                        for (auto &v : w) v = (int64_t)rnd();                               // any int64
                                        w[0] = INT64_MIN; w[w.size() - 1] = INT64_MAX;
                                        if (crc_conv_slots_fold(P, w, Cout, Cin + 1, t, fold) || !fold.empty()) return 5;
                                        if (!crc_conv_slots_fold(P, w, Cout, Cin, t, fold) || fold.size() != (size_t)Cout * Cin * T) return 6;
                                        for (int64_t v : fold) if (v < 0 || v >= t) return 7;
                                        // planes [Cin][n]: junk below t everywhere, the image at its slots of every period
                                        std::vector<int64_t> img((size_t)Cin * H * W), x((size_t)Cin * n);
                                        for (auto &v : img) v = (int64_t)(rnd() % (uint64_t)t);
                                        for (int ci = 0; ci < Cin; ci++) {
                                            std::vector<int64_t> per((size_t)M);
                                            for (auto &v : per) v = (int64_t)(rnd() % (uint64_t)t);
                                            for (int y = 0; y < H; y++) for (int xx = 0; xx < W; xx++) per[(size_t)(dil * (y * pitch + xx))] = img[((size_t)ci * H + y) * W + xx];
                                            for (int i = 0; i < n; i++) x[(size_t)ci * n + i] = per[(size_t)(i % M)];
                                        }
                                        for (int co = 0; co < Cout; co++)
                                            for (int half = 0; half < 2; half++)
                                                for (int base = 0; base < h; base += M)
                                                    for (size_t vi = 0; vi < P.valid.size(); vi++) {
                                                        const int slot = base + P.valid[vi], oy = (int)vi / P.out_w, ox = (int)vi % P.out_w;
                                                        i128 got = 0, want = 0;
                                                        for (int ci = 0; ci < Cin; ci++) {
                                                            for (int tau = 0; tau < T; tau++)
                                                                got = (got + (i128)fold[((size_t)co * Cin + ci) * T + tau]
                                                                                 * x[(size_t)ci * n + half * h + (slot + P.steps[tau]) % h]) % t;
                                                            for (int u = 0; u < pool; u++) for (int v = 0; v < pool; v++)
                                                                for (int a = 0; a < fh; a++) for (int b = 0; b < fw; b++) {
                                                                    int64_t wv = w[(((size_t)co * Cin + ci) * fh + a) * fw + b] % t;
                                                                    if (wv < 0) wv += t;
                                                                    want = (want + (i128)wv * img[((size_t)ci * H + pool * oy + u + a) * W + pool * ox + v + b]) % t;
                                                                }
                                                        }
                                                        if (got != want) {
                                                            fprintf(stderr, "slots n %d M %d pitch %d H %d W %d f %d %d dil %d pool %d slot %d\n", n, M, pitch, H, W, fh, fw, dil, pool, slot);
                                                            return 8;
                                                        }
                                                    }
                                    }
    printf("ok %ld %ld\n", plans, refusals);
    return 0;
}
