// conv_slots_geom_plan_sanitize_main -- crc_conv_slots_plan_geom, crc_conv_slots_fold_geom and crc_conv_slots_mask_slots (crcnn_amd/host/diag_plan.h) under the
// host address and undefined-behaviour sanitizers: a stand-alone program, no engine and no device.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I crcnn_amd/host tools/conv_slots_geom_plan_sanitize_main.cpp -o conv_slots_geom_plan_sanitize
// Walks rings n <= 512, power-of-two and other M, plane shapes, pitches and origins with margins 0 .. 2, windows, pads 0 .. 2, strides, pools and pool strides,
// dilations (valid and not), weights up to the int64 limits, and some arguments at the int limits.  For every plan it checks, on integer slots -- the plane tiled
// with period M, random junk at every other slot where pad = 0 and zeros there where pad > 0 -- that Sum_tau fold[tau] x[(slot + steps[tau]) mod n/2] at every valid
// slot of every period equals the padded, strided, pooled convolution mod t in 128-bit integers, and that the mask is the tiled valid list.  At pad = 0,
// stride = 1, pool_stride = pool and origin = 0 the plan must be crc_conv_slots_plan's, admission included.
// Prints "ok <plans> <refusals>"; any other exit is a failure.
#include <climits>
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
    {                                                                   // arguments at the limits: refused without overflow
        ConvSlotsGeomPlan P;
        const int N = 1 << 30, M29 = 1 << 29;
        if (crc_conv_slots_plan_geom(INT_MIN, M29, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, P)) return 20;
        for (int which = 0; which < 11; which++)
            for (int other = 0; other < 11; other++) {
                int a[11] = {8, 0, 4, 4, 3, 3, 1, 1, 1, 1, 1};          // pitch origin H W fh fw dil pad stride pool pool_stride
                a[which] = INT_MAX;
                if (crc_conv_slots_plan_geom(N, M29, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], P)) return 21;
                a[which] = M29; a[other] = M29;                          // two factors at the period: every product on the way must hold
                if (which != other && crc_conv_slots_plan_geom(N, M29, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], P)) return 24;
            }
        if (crc_conv_slots_plan_geom(2048, 1024, 2, 0, 2, 2, 1, 1, 1024, 0, 1024, 1, 1024, P)) return 22;   // dil stride pool_stride = 2^30: beyond the period
        if (P.n || !P.steps.empty()) return 23;
    }
    for (int n : {0, 2, 6, 64, 512})
        for (int M : {0, 1, 3, 32, 48, 256, 512})
            for (int H = 0; H <= 5; H += 1 + (H > 2))
                for (int W = 1; W <= 5; W += 2)
                    for (int margin = 0; margin <= 2; margin++)
                        for (int fh = 0; fh <= 3; fh++)
                            for (int pad = -1; pad <= 2; pad++)
                                for (int dil = 0; dil <= 2; dil++)
                                    for (int stride = 0; stride <= 2; stride++)
                                        for (int pool = 0; pool <= 2; pool++)
                                            for (int ps = 0; ps <= 2; ps++) {
                                                const int fw = 1 + (fh + pad + 1) % 3, pitch = W + margin - (margin == 0 && (H & 1) && fh == 0 ? 1 : 0);
                                                const int origin = margin * (pitch + 1);
                                                ConvSlotsGeomPlan P;
                                                const bool ok = crc_conv_slots_plan_geom(n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps, P);
                                                if (pad == 0 && stride == 1 && origin == 0 && (ps == 0 || ps == pool)) {      // the old planner's own parameters
                                                    ConvSlotsPlan O;
                                                    if (crc_conv_slots_plan(n, M, pitch, H, W, fh, fw, dil, pool, O) != ok) return 30;
                                                    if (ok && (O.steps != P.steps || O.elements != P.elements || O.valid != P.valid || O.out_h != P.out_h || O.out_w != P.out_w ||
                                                               O.out_dil != P.out_dil)) return 31;
                                                }
                                                if (!ok) { refusals++; if (P.n || !P.steps.empty() || !P.valid.empty()) return 2; continue; }
                                                plans++;
                                                const int q = ps ? ps : pool, eh = fh + stride * (pool - 1), ew = fw + stride * (pool - 1), T = eh * ew, Cout = 2, Cin = 2, h = n / 2;
                                                if ((int)P.steps.size() != T || (int)P.elements.size() != T || P.out_dil != dil * stride * q || P.needs_clean_input != (pad > 0)) return 3;
                                                for (uint64_t e : P.elements) if (!(e & 1) || e >= 2 * (uint64_t)n) return 4;
                                                const int64_t t = ts[plans % 3];
                                                std::vector<int64_t> w((size_t)Cout * Cin * fh * fw), fold;
                                                for (auto &v : w) v = (int64_t)rnd();                       // any int64
                                                w[0] = INT64_MIN; w[w.size() - 1] = INT64_MAX;
                                                if (crc_conv_slots_fold_geom(P, w, Cout, Cin + 1, t, fold) || !fold.empty()) return 5;
                                                if (!crc_conv_slots_fold_geom(P, w, Cout, Cin, t, fold) || fold.size() != (size_t)Cout * Cin * T) return 6;
                                                for (int64_t v : fold) if (v < 0 || v >= t) return 7;
                                                const std::vector<int64_t> mask = crc_conv_slots_mask_slots(P);
                                                std::vector<char> isv((size_t)M, 0);
                                                for (int v : P.valid) { if (v < 0 || v >= M || isv[(size_t)v]) return 9; isv[(size_t)v] = 1; }
                                                if ((int)mask.size() != n) return 10;
                                                for (int i = 0; i < n; i++) if (mask[(size_t)i] != isv[(size_t)(i % M)]) return 11;
                                                // planes [Cin][n]: the image at its slots of every period; elsewhere junk below t (pad = 0) or zeros (the clean input pad > 0 needs)
                                                std::vector<int64_t> img((size_t)Cin * H * W), x((size_t)Cin * n);
                                                for (auto &v : img) v = (int64_t)(rnd() % (uint64_t)t);
                                                for (int ci = 0; ci < Cin; ci++) {
                                                    std::vector<int64_t> per((size_t)M, 0);
                                                    if (pad == 0) for (auto &v : per) v = (int64_t)(rnd() % (uint64_t)t);
                                                    for (int y = 0; y < H; y++)
                                                        for (int xx = 0; xx < W; xx++) per[(size_t)(origin + dil * (y * pitch + xx))] = img[((size_t)ci * H + y) * W + xx];
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
                                                                                         * x[(size_t)ci * n + half * h + ((slot + P.steps[tau]) % h + h) % h]) % t;
                                                                    for (int u = 0; u < pool; u++) for (int v = 0; v < pool; v++)
                                                                        for (int a = 0; a < fh; a++) for (int b = 0; b < fw; b++) {
                                                                            const int iy = stride * (q * oy + u) + a - pad, ix = stride * (q * ox + v) + b - pad;
                                                                            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;      // a zero of the padding
                                                                            int64_t wv = w[(((size_t)co * Cin + ci) * fh + a) * fw + b] % t;
                                                                            if (wv < 0) wv += t;
                                                                            want = (want + (i128)wv * img[((size_t)ci * H + iy) * W + ix]) % t;
                                                                        }
                                                                }
                                                                if (got != want) {
                                                                    fprintf(stderr, "slots n %d M %d pitch %d origin %d H %d W %d f %d %d dil %d pad %d stride %d pool %d %d slot %d\n", n, M,
                                                                            pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps, slot);
                                                                    return 8;
                                                                }
                                                            }
                                            }
    if (plans < 1000) return 12;
    printf("ok %ld %ld\n", plans, refusals);
    return 0;
}
