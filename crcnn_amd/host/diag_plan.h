// diag_plan.h -- the plan of the diagonal matrix-vector product over slots (matvecSlots, crcnn_host.h), header only: no engine, no device.
// W (out x in, out and in <= M) is taken as zero-padded to M x M, M a power of two <= n/2.  For every diagonal d with a non-zero entry: steps gets d and rows gets
// n more words, rows[r][i] = W[i mod M][(i mod M + d) mod M] -- period M over both rows of n/2 slots.  false (nothing written) for a bad M or shape.
#pragma once
#include <cstdint>
#include <vector>

inline bool crc_diag_plan(const std::vector<std::vector<int64_t>> &W, int M, int n, std::vector<int> &steps, std::vector<int64_t> &rows)
{
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || (int)W.size() > M) return false;
    for (auto &r : W) if ((int)r.size() > M) return false;
    steps.clear(); rows.clear();
    std::vector<int64_t> diag((size_t)M);
    for (int d = 0; d < M; d++) {
        bool any = false;
        for (int i = 0; i < M; i++) {
            const int j = (i + d) % M;
            diag[i] = i < (int)W.size() && j < (int)W[i].size() ? W[i][j] : 0;
            any = any || diag[i] != 0;
        }
        if (!any) continue;
        steps.push_back(d);
        for (int i = 0; i < n; i++) rows.push_back(diag[i % M]);
    }
    return true;
}

// ---- baby-step / giant-step (matvecSlotsBsgs; crc_diag_mac_bsgs_forms) ----
// A diagonal d = B j + b (0 <= b < B, B a power of two, 1 <= B <= M) is reached as rotate(., B j) of a product with rotate(x, b):
//     y = Sum_j rotate_rows( Sum_b rows[j][b] (.) rotate_rows(x, b), B j ),   rows[j][b][i] = W[(i - B j) mod M][(i + b) mod M]
// (the diagonal d, rotated back by the giant step that follows the product; period M over both rows of n/2 slots).  giant_steps gets B j for every group j
// with a non-zero entry, baby_steps every b with a non-zero entry in a kept group, rows [giant][baby][n] with zero rows where a pair (j, b) is empty.
// Preconditions as crc_diag_plan, plus those on B; false (nothing written) otherwise.
inline bool crc_bsgs_plan(const std::vector<std::vector<int64_t>> &W, int M, int n, int B, std::vector<int> &baby_steps, std::vector<int> &giant_steps,
                          std::vector<int64_t> &rows)
{
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || (int)W.size() > M || B < 1 || (B & (B - 1)) || B > M) return false;
    for (auto &r : W) if ((int)r.size() > M) return false;
    auto at = [&](int i, int j) -> int64_t { return i < (int)W.size() && j < (int)W[i].size() ? W[i][j] : 0; };
    std::vector<char> used((size_t)M, 0), baby((size_t)B, 0);           // diagonals with a non-zero entry; baby steps with one
    for (int d = 0; d < M; d++)
        for (int i = 0; i < M && !used[d]; i++) used[d] = at(i, (i + d) % M) != 0;
    baby_steps.clear(); giant_steps.clear(); rows.clear();
    for (int j = 0; j < M / B; j++) {
        bool any = false;
        for (int b = 0; b < B; b++) if (used[B * j + b]) { any = true; baby[b] = 1; }
        if (any) giant_steps.push_back(B * j);
    }
    for (int b = 0; b < B; b++) if (baby[b]) baby_steps.push_back(b);
    for (int gs : giant_steps)
        for (int b : baby_steps)
            for (int i = 0; i < n; i++) rows.push_back(at(((i - gs) % M + M) % M, (i + b) % M));
    return true;
}
// the Galois elements of a dense M x M product split at B: 3^s mod 2n (crc_galois_elt_rows) of every baby step 1 .. B - 1 and every giant step B, 2 B, .. M - B,
// each once, in that order -- the key set to generate.  Empty for bad arguments (those of crc_bsgs_plan) and for M = 1
inline std::vector<uint64_t> crc_bsgs_elements(int M, int B, int n)
{
    std::vector<uint64_t> out;
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || B < 1 || (B & (B - 1)) || B > M) return out;
    const uint64_t mask = 2 * (uint64_t)n - 1;
    uint64_t g = 1;
    for (int s = 1; s < M; s++) {
        g = g * 3 & mask;
        if (s < B || s % B == 0) out.push_back(g);
    }
    return out;
}

// ---- the packed convolution over slots (convSlots; crc_conv_slots_forms) ----
// ONE image, one channel plane per ciphertext: pixel (y, x) of an H x W plane at slot dil (y pitch + x), tiled with period M over both rows of n/2 slots (matvecSlots'
// input contract).  A 'valid' convolution with an fh x fw window, stride 1 on the dilated grid, then a pool x pool sum pool of stride pool folded in front of the
// rotations: the window becomes (fh + pool - 1) x (fw + pool - 1), tap (a, b) is the row rotation by dil (a pitch + b) with the weight
// w'[a][b] = Sum_{u, v < pool} w[a - u][b - v], and output (y, x) lands where input (pool y, pool x) was: at slot out_dil (y pitch + x), out_dil = dil pool.
// Slots outside `valid` hold junk that the next layer's weights never read: no masks, no zero padding.
struct ConvSlotsPlan {
    int n = 0, M = 0, pitch = 0, fh = 0, fw = 0, pool = 0;
    int out_h = 0, out_w = 0, out_dil = 0;
    std::vector<int> steps;                  // [T] row-major over the enlarged window
    std::vector<uint64_t> elements;          // [T] 3^step mod 2n (crc_galois_elt_rows); tap (0, 0): the element 1, which needs no key
    std::vector<int> valid;                  // [out_h out_w] row-major: the slots of the first period that hold an output
};
// false (P untouched) for M not a power of two <= n/2, a plane that does not fit (W <= pitch, dil ((H - 1) pitch + W - 1) < M), a window larger than the plane,
// a pool that leaves no output, a step >= n/2
inline bool crc_conv_slots_plan(int n, int M, int pitch, int H, int W, int fh, int fw, int dil, int pool, ConvSlotsPlan &P)
{
    if (n < 2 || (n & (n - 1)) || M < 1 || (M & (M - 1)) || M > n / 2) return false;
    if (pitch < 1 || H < 1 || W < 1 || fh < 1 || fw < 1 || dil < 1 || pool < 1 || W > pitch || fh > H || fw > W) return false;
    if ((int64_t)dil * ((int64_t)(H - 1) * pitch + W - 1) >= M) return false;      // (every factor is below M from here on: no overflow)
    const int oh = (H - fh + 1) / pool, ow = (W - fw + 1) / pool, eh = fh + pool - 1, ew = fw + pool - 1;
    if (oh < 1 || ow < 1 || (int64_t)dil * ((int64_t)(eh - 1) * pitch + ew - 1) >= n / 2) return false;
    ConvSlotsPlan Q;
    Q.n = n; Q.M = M; Q.pitch = pitch; Q.fh = fh; Q.fw = fw; Q.pool = pool; Q.out_h = oh; Q.out_w = ow; Q.out_dil = dil * pool;
    const uint64_t mask = 2 * (uint64_t)n - 1;
    for (int a = 0; a < eh; a++)
        for (int b = 0; b < ew; b++) {
            const int s = dil * (a * pitch + b);
            uint64_t g = 1;
            for (uint64_t e = (uint64_t)s, x = 3; e; e >>= 1, x = x * x & mask) if (e & 1) g = g * x & mask;
            Q.steps.push_back(s); Q.elements.push_back(g);
        }
    for (int y = 0; y < oh; y++) for (int x = 0; x < ow; x++) Q.valid.push_back(Q.out_dil * (y * pitch + x));
    P = Q;
    return true;
}
// w [Cout][Cin][fh][fw] (any int64) -> out [Cout][Cin][T] in [0, t): the pool's window sum folded into the taps, mod t.  false (out untouched) for a size that is
// not Cout Cin fh fw, or t < 2
inline bool crc_conv_slots_fold(const ConvSlotsPlan &P, const std::vector<int64_t> &w, int Cout, int Cin, int64_t t, std::vector<int64_t> &out)
{
    if (Cout < 1 || Cin < 1 || t < 2 || P.fh < 1 || P.fw < 1 || P.pool < 1 || w.size() != (size_t)Cout * Cin * P.fh * P.fw) return false;
    const int eh = P.fh + P.pool - 1, ew = P.fw + P.pool - 1;
    std::vector<int64_t> o((size_t)Cout * Cin * eh * ew, 0);
    for (size_t c = 0; c < (size_t)Cout * Cin; c++)
        for (int a = 0; a < P.fh; a++)
            for (int b = 0; b < P.fw; b++) {
                int64_t v = w[(c * P.fh + a) * P.fw + b] % t;
                if (v < 0) v += t;
                for (int u = 0; u < P.pool; u++)
                    for (int x = 0; x < P.pool; x++) {
                        int64_t &d = o[(c * eh + a + u) * ew + b + x];
                        d = d >= t - v ? d - (t - v) : d + v;               // (d + v mod t without leaving [0, t))
                    }
            }
    out = o;
    return true;
}
