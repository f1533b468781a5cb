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

// ---- the packed convolution with strides, zero padding and a general pool (convSlots with a bias and a mask; crc_conv_slots_bias_mask_forms) ----
// Pixel (y, x) of an H x W plane at slot origin + dil (y pitch + x), tiled with period M over both rows of n/2 slots.  `pad` zero pixels on every side, conv
// stride `stride`, then a pool x pool sum pool of stride pool_stride on the convolution's outputs (pool = 1: none; pool_stride = 0 means pool).  The window becomes
// eh x ew = (fh + stride (pool - 1)) x (fw + stride (pool - 1)); tap (a, b) is the row rotation by dil ((a - pad) pitch + (b - pad)) -- a negative step is a right
// rotation, crc_galois_elt_rows' rule: 3^(n/2 - |step|) -- with the weight w'[a][b] = Sum_{u, v < pool} w[a - stride u][b - stride v]; ch = (H + 2 pad - fh) / stride
// + 1 convolution rows, out_h = (ch - pool) / pool_stride + 1 pooled ones, and output (y, x) lands at origin + out_dil (y pitch + x), out_dil = dil stride
// pool_stride: the same origin and pitch.
// pad = 0: slots that hold no pixel may hold anything (every tap of a valid output reads a pixel).  pad > 0: needs_clean_input -- every slot of a period that is no
// pixel must hold exactly 0, because that is where the taps beyond the edge read.  A result multiplied by mask_slots is clean again, and so is what
// encryptImagePlanes with a margin or densePlanes writes.
struct ConvSlotsGeomPlan {
    int n = 0, M = 0, pitch = 0, origin = 0, fh = 0, fw = 0, pad = 0, stride = 0, pool = 0, pool_stride = 0;
    int out_h = 0, out_w = 0, out_dil = 0;
    bool needs_clean_input = false;
    std::vector<int> steps;                  // [T] row-major over the enlarged window; negative: a right rotation
    std::vector<uint64_t> elements;          // [T] crc_galois_elt_rows(step); step 0: the element 1, which needs no key
    std::vector<int> valid;                  // [out_h out_w] row-major: the slots of the first period that hold an output
};
// false (P untouched) for what crc_conv_slots_plan refuses (M not a power of two <= n/2, a plane that does not fit, a window larger than the padded plane, no
// output, |step| >= n/2), for outputs that leave the period or share a slot, and -- by enumeration over every tap of every valid output -- for a tap beyond the
// plane's edge that lands on another pixel's slot modulo M: too little margin (pitch < W + pad, or an origin too small).  With pad = 0, stride = 1,
// pool_stride = pool and origin = 0 the steps, elements, output geometry and valid list are crc_conv_slots_plan's
inline bool crc_conv_slots_plan_geom(int n, int M, int pitch, int origin, int H, int W, int fh, int fw, int dil, int pad, int stride, int pool, int pool_stride,
                                     ConvSlotsGeomPlan &P)
{
    if (n < 2 || (n & (n - 1)) || M < 1 || (M & (M - 1)) || M > n / 2) return false;
    if (pool_stride == 0) pool_stride = pool;
    if (pitch < 1 || H < 1 || W < 1 || fh < 1 || fw < 1 || dil < 1 || stride < 1 || pool < 1 || pool_stride < 1 || pad < 0 || origin < 0 || W > pitch) return false;
    for (int v : {pitch, origin, H, W, fh, fw, dil, pad, stride, pool, pool_stride}) if (v > M) return false;     // (every factor at most M <= 2^30 from here on)
    const int64_t span = (int64_t)(H - 1) * pitch + W - 1;
    if (origin >= M || (span > 0 && dil > ((int64_t)M - 1 - origin) / span)) return false;                      // origin + dil span >= M
    if (fh > H + 2 * (int64_t)pad || fw > W + 2 * (int64_t)pad) return false;
    const int64_t ch = (H + 2 * (int64_t)pad - fh) / stride + 1, cw = (W + 2 * (int64_t)pad - fw) / stride + 1;
    if (ch < pool || cw < pool) return false;
    const int64_t oh = (ch - pool) / pool_stride + 1, ow = (cw - pool) / pool_stride + 1;
    const int64_t eh = fh + (int64_t)stride * (pool - 1), ew = fw + (int64_t)stride * (pool - 1);               // (<= H + 2 pad, W + 2 pad: ch, cw >= pool)
    if ((int64_t)dil * stride > 0x7fffffff || (int64_t)dil * stride * pool_stride > 0x7fffffff) return false;  // (dil stride <= 2^60, then <= 2^31 times 2^30)
    const int64_t od = (int64_t)dil * stride * pool_stride;
    const int64_t last = (oh - 1) * pitch + ow - 1;
    if (last > 0 && od > ((int64_t)M - 1 - origin) / last) return false;                                         // an output beyond the period
    int64_t far = 0;                                                                                             // max |(a - pad) pitch + (b - pad)|: at a corner
    for (int64_t a : {(int64_t)0, eh - 1})
        for (int64_t b : {(int64_t)0, ew - 1}) {
            const int64_t v = (a - pad) * pitch + (b - pad);
            far = v < 0 ? (-v > far ? -v : far) : (v > far ? v : far);
        }
    if (far > 0 && dil > (n / 2 - 1) / far) return false;                                                        // |step| >= n/2
    ConvSlotsGeomPlan Q;
    Q.n = n; Q.M = M; Q.pitch = pitch; Q.origin = origin; Q.fh = fh; Q.fw = fw; Q.pad = pad; Q.stride = stride; Q.pool = pool; Q.pool_stride = pool_stride;
    Q.out_h = (int)oh; Q.out_w = (int)ow; Q.out_dil = (int)od; Q.needs_clean_input = pad > 0;
    const uint64_t mask = 2 * (uint64_t)n - 1;
    for (int64_t a = 0; a < eh; a++)
        for (int64_t b = 0; b < ew; b++) {
            const int s = (int)(dil * ((a - pad) * pitch + (b - pad)));
            uint64_t g = 1;
            for (uint64_t e = (uint64_t)(s < 0 ? n / 2 + s : s), x = 3; e; e >>= 1, x = x * x & mask) if (e & 1) g = g * x & mask;
            Q.steps.push_back(s); Q.elements.push_back(g);
        }
    std::vector<char> pixel((size_t)M, 0), out((size_t)M, 0);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) pixel[(size_t)(origin + (int64_t)dil * ((int64_t)y * pitch + x))] = 1;
    for (int64_t y = 0; y < oh; y++)
        for (int64_t x = 0; x < ow; x++) {
            const int64_t s = origin + od * (y * pitch + x);
            if (out[(size_t)s]) return false;                                                                    // two outputs in one slot
            out[(size_t)s] = 1; Q.valid.push_back((int)s);
            for (int64_t a = 0; a < eh && pad > 0; a++)
                for (int64_t b = 0; b < ew; b++) {
                    const int64_t iy = (int64_t)stride * pool_stride * y + a - pad, ix = (int64_t)stride * pool_stride * x + b - pad;
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) continue;
                    if (pixel[(size_t)(((s + Q.steps[(size_t)(a * ew + b)]) % M + M) % M)]) return false;        // a zero of the padding that is a pixel
                }
        }
    P = Q;
    return true;
}
// w [Cout][Cin][fh][fw] (any int64) -> out [Cout][Cin][T] in [0, t): w'[a][b] = Sum_{u, v < pool} w[a - stride u][b - stride v] mod t.  false (out untouched)
// for a size that is not Cout Cin fh fw, or t < 2
inline bool crc_conv_slots_fold_geom(const ConvSlotsGeomPlan &P, const std::vector<int64_t> &w, int Cout, int Cin, int64_t t, std::vector<int64_t> &out)
{
    if (Cout < 1 || Cin < 1 || t < 2 || P.fh < 1 || P.fw < 1 || P.pool < 1 || P.stride < 1 || w.size() != (size_t)Cout * Cin * P.fh * P.fw) return false;
    const size_t eh = (size_t)P.fh + (size_t)P.stride * (P.pool - 1), ew = (size_t)P.fw + (size_t)P.stride * (P.pool - 1);
    std::vector<int64_t> o((size_t)Cout * Cin * eh * ew, 0);
    for (size_t c = 0; c < (size_t)Cout * Cin; c++)
        for (int a = 0; a < P.fh; a++)
            for (int b = 0; b < P.fw; b++) {
                int64_t v = w[(c * P.fh + a) * P.fw + b] % t;
                if (v < 0) v += t;
                for (int u = 0; u < P.pool; u++)
                    for (int x = 0; x < P.pool; x++) {
                        int64_t &d = o[(c * eh + a + (size_t)P.stride * u) * ew + b + (size_t)P.stride * x];
                        d = d >= t - v ? d - (t - v) : d + v;               // (d + v mod t without leaving [0, t))
                    }
            }
    out = o;
    return true;
}
// the 0/1 slot vector [n] that is 1 exactly where (slot mod M) is a valid output: the plaintext whose NTT-form row is crc_conv_slots_bias_mask_forms' d_mask_ntt
inline std::vector<int64_t> crc_conv_slots_mask_slots(const ConvSlotsGeomPlan &P)
{
    std::vector<int64_t> m((size_t)(P.n > 0 ? P.n : 0), 0);
    for (int s : P.valid) for (int i = s; P.M > 0 && i < P.n; i += P.M) m[(size_t)i] = 1;
    return m;
}

// ---- the dense layer over channel planes (densePlanes; crc_dense_planes_forms) ----
// Cin ciphertexts x_c whose valid entries sit at the slots in_slots [P] of every period M (tiled over both rows of n/2 slots: matvecSlots' contract; every other
// slot may hold junk), O outputs that land at the slots out_slots [O].  The OUTPUTS are rotated (rotate_rows' convention: after a rotation by r, slot i holds
// old slot (i + r) mod n/2):
//     y = Sum_j rotate_rows( Sum_c rows[j][c] (.) x_c, steps[j] ),   steps: the distinct values (in_slots[p] - out_slots[o]) mod M, ascending,
//     rows[j][c][i] = W[o][c][p]  for i mod M = in_slots[p] where out_slots[o] = (in_slots[p] - steps[j]) mod M;  0 where no such o exists and at every other slot
// so that y holds Sum_c Sum_p W[o][c][p] x_c[in_slots[p]] at out_slots[o] and exactly 0 at every other slot of the period: one key switch per step whatever Cin
// is.  The caller chooses out_slots, and the choice decides the number of steps.
struct DensePlanesPlan {
    int n = 0, M = 0;
    std::vector<int> in_slots, out_slots;
    std::vector<int> steps;                  // [R] ascending; step 0 is the element 1, which needs no key
    std::vector<uint64_t> elements;          // [R] 3^step mod 2n (crc_galois_elt_rows)
    std::vector<int> out_at;                 // [M] the output whose slot this is, or -1
};
// false (P untouched) for M not a power of two <= n/2, an empty or duplicated slot list, a slot outside [0, M)
inline bool crc_dense_planes_plan(int n, int M, const std::vector<int> &in_slots, const std::vector<int> &out_slots, DensePlanesPlan &P)
{
    if (n < 2 || (n & (n - 1)) || M < 1 || (M & (M - 1)) || M > n / 2 || in_slots.empty() || out_slots.empty()) return false;
    DensePlanesPlan Q;
    Q.n = n; Q.M = M; Q.in_slots = in_slots; Q.out_slots = out_slots;
    Q.out_at.assign((size_t)M, -1);
    std::vector<char> in_seen((size_t)M, 0), used((size_t)M, 0);
    for (int s : in_slots) { if (s < 0 || s >= M || in_seen[s]) return false; in_seen[s] = 1; }
    for (size_t o = 0; o < out_slots.size(); o++) {
        const int s = out_slots[o];
        if (s < 0 || s >= M || Q.out_at[s] >= 0) return false;
        Q.out_at[s] = (int)o;
    }
    for (int p : in_slots) for (int o : out_slots) used[((p - o) % M + M) % M] = 1;
    const uint64_t mask = 2 * (uint64_t)n - 1;
    uint64_t g = 1;
    for (int s = 0; s < M; s++, g = g * 3 & mask)
        if (used[s]) { Q.steps.push_back(s); Q.elements.push_back(g); }
    P = Q;
    return true;
}
// the rows of ONE step: W [O][Cin][P] (any int64, taken mod t) -> rows [Cin][n] in [0, t).  false (rows untouched) for a weight count that is not O Cin P,
// Cin < 1, t < 2 or a step index outside the plan
inline bool crc_dense_planes_fold_step(const DensePlanesPlan &P, const std::vector<int64_t> &W, int Cin, int64_t t, int j, std::vector<int64_t> &rows)
{
    const size_t O = P.out_slots.size(), NP = P.in_slots.size();
    if (Cin < 1 || t < 2 || j < 0 || j >= (int)P.steps.size() || P.M < 1 || W.size() != O * (size_t)Cin * NP) return false;
    std::vector<int64_t> r((size_t)Cin * P.n, 0);
    for (size_t p = 0; p < NP; p++) {
        const int sp = P.in_slots[p], o = P.out_at[((sp - P.steps[j]) % P.M + P.M) % P.M];
        if (o < 0) continue;
        for (int c = 0; c < Cin; c++) {
            int64_t v = W[((size_t)o * Cin + c) * NP + p] % t;
            if (v < 0) v += t;
            for (int i = sp; i < P.n; i += P.M) r[(size_t)c * P.n + i] = v;
        }
    }
    rows = r;
    return true;
}
// every step: rows [R][Cin][n]
inline bool crc_dense_planes_fold(const DensePlanesPlan &P, const std::vector<int64_t> &W, int Cin, int64_t t, std::vector<int64_t> &rows)
{
    std::vector<int64_t> all, one;
    for (int j = 0; j < (int)P.steps.size(); j++) {
        if (!crc_dense_planes_fold_step(P, W, Cin, t, j, one)) return false;
        all.insert(all.end(), one.begin(), one.end());
    }
    if (P.steps.empty()) return false;
    rows = all;
    return true;
}
// where a packed convolution leaves its outputs: the in_slots of the dense layer behind it
inline std::vector<int> crc_dense_planes_in_slots(const ConvSlotsPlan &P) { return P.valid; }
inline std::vector<int> crc_dense_planes_in_slots(const ConvSlotsGeomPlan &P) { return P.valid; }
