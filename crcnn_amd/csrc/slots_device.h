// slots_device.h -- device side of slot batching (kernels_slots.hip): argument block, block -> item order, the bodies of slots_compose_kernel and
// slots_decompose_kernel, of slots_rescale_kernel, of slots_act_kernel and of the two kernels over several plain moduli (slots_crt_*).  A header so that
// tests/cpp/slots_kernel_check.cpp, slots_rescale_kernel_check.cpp, slots_act_kernel_check.cpp and slots_crt_kernel_check.cpp can run the same text on the CPU,
// one thread per workgroup, under sanitizers.
#pragma once
#include "ntt_device.h"

// Items per XCD group.  In the image-major layout (item_stride 1, slot_stride = pixels) the workgroups of items c .. c + 15 read the same 128-byte lines, 8 bytes
// each: they take consecutive slots of ONE XCD (xcd_group), so a line comes from memory once and from that XCD's L2 fifteen times.
#define CRC_SLOT_GROUP 16

struct SlotArgs {
    const long long *vals_in; long long *vals_out;          // compose reads vals_in, decompose writes vals_out
    const u64 *plain_in; u64 *plain_out;                    // [count][n]
    const ulonglong2 *W; const u32 *idx;
    size_t count, item_stride, slot_stride;
    int n, logn, slots;
    u64 t, one_s;
};

// the row of this workgroup, for all three kernels: false for the blocks that pad the grid
__device__ __forceinline__ bool slot_item(size_t count, size_t &item)
{
    size_t grp; unsigned member;
    if (!xcd_group(blockIdx.x, CRC_SLOT_GROUP, (count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP, grp, member)) return false;
    item = grp * CRC_SLOT_GROUP + member;
    return item < count;
}
// any int64 -> its residue mod t (the magnitude through the Shoup reduction, then the sign; -2^63 has the magnitude 2^63)
__device__ __forceinline__ u64 slot_residue(long long x, u64 t, u64 one_s)
{
    const u64 mag = x < 0 ? 0 - (u64)x : (u64)x;
    const u64 r = mulmod_shoup(mag, 1, one_s, t);
    return x < 0 && r ? t - r : r;
}

// The gap-1 stage stays a pass of its own at log2 n = 3 m + 1 (FUSE1 off): the image is filled (compose) / drained (decompose) in SLOT order, so that the
// strided or contiguous value accesses stay in the caller's order, and the pairs (s, s + 1) the fused stage works on never meet in one lane.
template <bool LAZY>
__device__ __forceinline__ void slots_compose_body(const SlotArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 t = a.t, one_s = a.one_s;
    const long long *v = a.vals_in + item * a.item_stride;
    for (int i = tid; i < n; i += nt) sm[lpad((int)a.idx[i])] = i < a.slots ? slot_residue(v[(size_t)i * a.slot_stride], t, one_s) : 0;
    __syncthreads();
    ntt_row_passes<true, LAZY, 3, false>(sm, a.W, n, a.logn, t, t + t);
    u64 *dst = a.plain_out + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // below 16 t (lazy) / 2 t (strict): one Shoup reduction makes it canonical
        st2(dst + s, mulmod_shoup(r.x, 1, one_s, t), mulmod_shoup(r.y, 1, one_s, t));
    }
}

template <bool LAZY>
__device__ __forceinline__ void slots_decompose_body(const SlotArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 t = a.t, one_s = a.one_s, half = (t - 1) >> 1;
    const u64 *src = a.plain_in + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 p = ld2(src + s);
        sm_store_pair64(sm, s, mulmod_shoup(p.x, 1, one_s, t), mulmod_shoup(p.y, 1, one_s, t));
    }
    __syncthreads();
    ntt_row_passes<false, LAZY, 3, false>(sm, a.W, n, a.logn, t, t + t);
    long long *out = a.vals_out + item * a.item_stride;
    for (int i = tid; i < a.slots; i += nt) {
        const u64 r = mulmod_shoup(sm[lpad((int)a.idx[i])], 1, one_s, t);      // below (1 + 4 log2 n) t (lazy) / 4 t (strict)
        out[(size_t)i * a.slot_stride] = r > half ? (long long)r - (long long)t : (long long)r;
    }
}

// ---- rescale: every slot of a plaintext divided by an integer D, rounded to nearest (ties towards +infinity) -------------------------------------------------
// The operation is the same in every slot, so the slot -> position map cancels: forward transform, the division in POSITION order, inverse transform; no idx
// loads and no slot count.  Position order also puts the pair (s, s + 1) into one lane, so at log2 n = 3 m + 1 the division sits between the two gap-1 stages
// (FUSE1 on in both directions: 4 + 4 LDS passes where decompose + compose run 5 + 5).
struct SlotRescaleArgs {
    const u64 *plain_in; u64 *plain_out;                    // [count][n]; the same pointer is allowed (a workgroup has read its row before it writes)
    const ulonglong2 *Wf, *Wi;                              // t's forward / inverse tables
    size_t count;
    int n, logn;
    u64 t, one_s;
    u64 D, recip;                                           // recip = floor(2^64 / D); 2^64 - 1 for D = 1 (the correction step makes up for it)
    u64 hpos, hneg;                                         // D >> 1 and (D - 1) >> 1: what rounding adds to the magnitude of a value >= 0 / < 0
};

// floor(x / D) for any 64-bit x, 1 <= D < 2^64: with recip = (2^64 - e) / D, 0 <= e < D, x recip / 2^64 = x / D - x e / (D 2^64) lies in (x / D - 1, x / D], so
// the estimate is the quotient or one short, as in mulmod_shoup.  D = 1 with recip = 2^64 - 1: the estimate is x - 1 (0 for x = 0), the remainder 1 (0), corrected.
__device__ __forceinline__ u64 slot_quotient(u64 x, u64 D, u64 recip)
{
    const u64 qe = mulhi64(x, recip);
    return x - qe * D >= D ? qe + 1 : qe;
}
// canonical r -> the residue of floor(v / D + 1/2), v the centred value of r.  v >= 0: floor((v + hpos) / D); v < 0: -ceil((|v| - hpos) / D) =
// -floor((|v| + hneg) / D) (hpos + hneg = D - 1).  |v| <= (t - 1) / 2 < 2^62 and D <= 2^62: the sum stays below 2^63; the quotient is at most |v|, below t.
__device__ __forceinline__ u64 slot_rescale_value(u64 r, const SlotRescaleArgs &a, u64 half)
{
    const bool neg = r > half;
    const u64 mag = neg ? a.t - r : r;
    const u64 qv = slot_quotient(mag + (neg ? a.hneg : a.hpos), a.D, a.recip);
    return neg && qv ? a.t - qv : qv;
}

template <bool LAZY>
__device__ __forceinline__ void slots_rescale_body(const SlotRescaleArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 t = a.t, t2 = t + t, one_s = a.one_s, half = (t - 1) >> 1;
    const bool fuse1 = ntt_fused_stage(a.logn);
    const ulonglong2 *F1 = a.Wf + (n >> 1), *I1 = a.Wi + (n >> 1);
    const u64 *src = a.plain_in + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 p = ld2(src + s);
        sm_store_pair64(sm, s, mulmod_shoup(p.x, 1, one_s, t), mulmod_shoup(p.y, 1, one_s, t));
    }
    __syncthreads();
    ntt_row_passes<false, LAZY, 3, true>(sm, a.Wf, n, a.logn, t, t2);
    for (int s = 2 * tid; s < n; s += 2 * nt) {              // a lane owns its 16-byte slot of the image: no barrier inside this loop
        ulonglong2 v = sm_load_pair64(sm, s);
        if (fuse1) fwd_pair_stage<LAZY>(v, F1[s >> 1], t, t2);
        v.x = slot_rescale_value(mulmod_shoup(v.x, 1, one_s, t), a, half);      // below (1 + 4 log2 n) t (lazy) / 4 t (strict) -> canonical -> rescaled
        v.y = slot_rescale_value(mulmod_shoup(v.y, 1, one_s, t), a, half);
        if (fuse1) inv_pair_stage<LAZY>(v, I1[s >> 1], t, t2);
        sm_store_pair64(sm, s, v.x, v.y);
    }
    __syncthreads();
    ntt_row_passes<true, LAZY, 3, true>(sm, a.Wi, n, a.logn, t, t2);
    u64 *dst = a.plain_out + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // below 16 t (lazy) / 2 t (strict)
        st2(dst + s, mulmod_shoup(r.x, 1, one_s, t), mulmod_shoup(r.y, 1, one_s, t));
    }
}

// ---- client-side activation: the maximum over a window of plaintext ROWS, slot by slot, then the rescale's division, ReLU and a cap ---------------------------
// out[pl][i][j] = compose(act(max over a < xf, b < yf of the centred slots of in[pl][i xs + a][j ys + b])), act(m) = min(max(floor(m / D + 1/2), 0 if relu), cap if
// cap).  Slot-wise and the same in every slot, so the slot -> position map cancels as it does for the rescale: everything happens in position order.  Rounding is
// non-decreasing, hence one division per output, behind the maximum.
struct SlotActArgs {
    const u64 *plain_in; u64 *plain_out;                    // [planes][xd][yd][n] -> [planes][xo][yo][n]; the same pointer only for a 1 x 1 window of stride 1
    const ulonglong2 *Wf, *Wi;
    size_t count;                                           // output rows: planes * xo * yo
    int n, logn;
    u64 t, one_s;
    u64 D, recip;                                           // as SlotRescaleArgs (what rounding adds, D >> 1 and (D - 1) >> 1, is formed where it is used)
    int xd, yd, xs, ys, xf, yf, xo, yo;
    int relu; u64 cap;                                      // cap = 0: none; otherwise 1 <= cap <= (t - 1) / 2
};

// centred maximum m -> the residue of act(m).  |m| <= (t - 1) / 2 and D <= 2^62: the sums stay below 2^63 as in slot_rescale_value.  A negative quotient is
// below every cap (cap >= 1), and a ReLU leaves 0 of it
__device__ __forceinline__ u64 slot_act_value(long long m, const SlotActArgs &a)
{
    const bool neg = m < 0;
    const u64 mag = neg ? 0 - (u64)m : (u64)m;
    u64 qv = slot_quotient(mag + ((a.D - (neg ? 1 : 0)) >> 1), a.D, a.recip);
    if (neg) return a.relu || !qv ? 0 : a.t - qv;
    if (a.cap && qv > a.cap) qv = a.cap;
    return qv;
}

// PAIRS: the 16-byte slots of the image one lane owns at most (on the device 4 up to n = 8192 and 8 at n = 16384, where the workgroup stops at 1024 threads; the
// CPU check, one thread per workgroup, passes n / 2).
// PAIRS = 0 is the kernel of a window of ONE row (client_relu): no running maximum to keep, the activation sits between the two gap-1 stages in one pointwise
// loop exactly as the rescale's division does, at that kernel's register count.
// Barriers.  The fill and the two pointwise loops give a lane the same slots s = 2 tid + 2 k nt of the image, and ntt_row_passes returns synchronised.  So a
// window row needs ONE barrier of its own, between its fill and its passes: the fold behind the passes reads only the lane's own slots, and the next row's fill
// overwrites exactly those -- what other lanes read of them they read inside the passes, in front of the barrier that ends them.  For the same reason the last
// fold, the activation and the store of the inverse transform's input run without one; the kernel's last barrier of its own stands in front of the inverse passes.
template <bool LAZY, int PAIRS>
__device__ __forceinline__ void slots_act_body(const SlotActArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 t = a.t, t2 = t + t, one_s = a.one_s, half = (t - 1) >> 1;
    const bool fuse1 = ntt_fused_stage(a.logn);
    const ulonglong2 *F1 = a.Wf + (n >> 1), *I1 = a.Wi + (n >> 1);
    if (PAIRS == 0) {                                       // one input row per output row, the same row index: the rescale's structure
        const u64 *src = a.plain_in + item * (size_t)n;
        for (int s = 2 * tid; s < n; s += 2 * nt) {
            const ulonglong2 p = ld2(src + s);
            sm_store_pair64(sm, s, mulmod_shoup(p.x, 1, one_s, t), mulmod_shoup(p.y, 1, one_s, t));
        }
        __syncthreads();
        ntt_row_passes<false, LAZY, 3, true>(sm, a.Wf, n, a.logn, t, t2);
        for (int s = 2 * tid; s < n; s += 2 * nt) {          // a lane owns its 16-byte slot of the image: no barrier inside this loop
            ulonglong2 v = sm_load_pair64(sm, s);
            if (fuse1) fwd_pair_stage<LAZY>(v, F1[s >> 1], t, t2);
            const u64 x = mulmod_shoup(v.x, 1, one_s, t), y = mulmod_shoup(v.y, 1, one_s, t);
            v.x = slot_act_value(x > half ? (long long)x - (long long)t : (long long)x, a);
            v.y = slot_act_value(y > half ? (long long)y - (long long)t : (long long)y, a);
            if (fuse1) inv_pair_stage<LAZY>(v, I1[s >> 1], t, t2);
            sm_store_pair64(sm, s, v.x, v.y);
        }
        __syncthreads();
        ntt_row_passes<true, LAZY, 3, true>(sm, a.Wi, n, a.logn, t, t2);
        u64 *dst = a.plain_out + item * (size_t)n;
        for (int s = 2 * tid; s < n; s += 2 * nt) {
            const ulonglong2 r = sm_load_pair64(sm, s);
            st2(dst + s, mulmod_shoup(r.x, 1, one_s, t), mulmod_shoup(r.y, 1, one_s, t));
        }
        return;
    }
    const size_t per = (size_t)a.xo * a.yo, pl = item / per, ij = item - pl * per;
    const int i = (int)(ij / a.yo), j = (int)(ij - (size_t)i * a.yo);
    long long mx[2 * PAIRS + 1];                            // the running maxima of the lane's slots, centred
#pragma unroll
    for (int k = 0; k < 2 * PAIRS; k++) mx[k] = -0x7fffffffffffffffLL - 1;
    // the window's rows: yf consecutive rows of the tensor, xf times at a distance of yd rows
    const u64 *win = a.plain_in + ((pl * a.xd + (size_t)(i * a.xs)) * a.yd + (size_t)(j * a.ys)) * (size_t)n;
    for (int wa = 0; wa < a.xf; wa++, win += (size_t)a.yd * n) for (int wb = 0; wb < a.yf; wb++) {
        const u64 *src = win + (size_t)wb * n;
        for (int s = 2 * tid; s < n; s += 2 * nt) {
            const ulonglong2 p = ld2(src + s);
            sm_store_pair64(sm, s, mulmod_shoup(p.x, 1, one_s, t), mulmod_shoup(p.y, 1, one_s, t));
        }
        __syncthreads();
        ntt_row_passes<false, LAZY, 3, true>(sm, a.Wf, n, a.logn, t, t2);
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            const int s = 2 * tid + 2 * k * nt;
            if (s < n) {                                     // (no break: eight independent conditions, not eight nested ones)
                ulonglong2 v = sm_load_pair64(sm, s);
                if (fuse1) fwd_pair_stage<LAZY>(v, F1[s >> 1], t, t2);
                const u64 x = mulmod_shoup(v.x, 1, one_s, t), y = mulmod_shoup(v.y, 1, one_s, t);   // below (1 + 4 log2 n) t (lazy) / 4 t (strict) -> canonical
                const long long cx = x > half ? (long long)x - (long long)t : (long long)x, cy = y > half ? (long long)y - (long long)t : (long long)y;
                mx[2 * k] = cx > mx[2 * k] ? cx : mx[2 * k];
                mx[2 * k + 1] = cy > mx[2 * k + 1] ? cy : mx[2 * k + 1];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PAIRS; k++) {
        const int s = 2 * tid + 2 * k * nt;
        if (s < n) {
            ulonglong2 v;
            v.x = slot_act_value(mx[2 * k], a); v.y = slot_act_value(mx[2 * k + 1], a);
            if (fuse1) inv_pair_stage<LAZY>(v, I1[s >> 1], t, t2);
            sm_store_pair64(sm, s, v.x, v.y);
        }
    }
    __syncthreads();
    ntt_row_passes<true, LAZY, 3, true>(sm, a.Wi, n, a.logn, t, t2);
    u64 *dst = a.plain_out + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // below 16 t (lazy) / 2 t (strict)
        st2(dst + s, mulmod_shoup(r.x, 1, one_s, t), mulmod_shoup(r.y, 1, one_s, t));
    }
}

// ---- several plain moduli: the slots of r plaintexts mod t_0 .. t_{r-1}, lifted by the Chinese remainder theorem to integers mod T = t_0 ... t_{r-1} < 2^63 --------
// One workgroup per item as above, ONE row image in LDS, the moduli visited one after the other.  A lane keeps the running value of the positions it owns -- the
// pairs s = 2 tid + 2 k nt, the ones the pointwise loops of the kernels above give it -- in registers and folds modulus j in by Garner's mixed-radix step:
//     x_0 = a_0,   x_j = x_{j-1} + P_{j-1} ((a_j - x_{j-1}) P_{j-1}^-1 mod t_j),   P_j = t_0 ... t_j.
// Bounds: 0 <= x_{j-1} < P_{j-1} and the digit is below t_j, so x_j <= P_{j-1} - 1 + P_{j-1} (t_j - 1) = P_j - 1 < T < 2^63: one u64, no carry.  x_{j-1} mod t_j is the
// Shoup reduction of slot_residue (any 64-bit word -> canonical); the digit is one Shoup product with the constant P_{j-1}^-1 mod t_j.
// Any t_j >= 2 n + 1 >= 129, so with two moduli or more every t_j < 2^63 / 129 < 2^57: only the lazy butterflies occur for r >= 2, the strict ones at r = 1 alone.
#ifndef CRC_SLOTS_CRT_MAX
#define CRC_SLOTS_CRT_MAX 4                                 // (crcnn_hip.h)
#endif
struct SlotCrtMod {
    const u64 *plain_in; u64 *plain_out;                    // row tensor of this modulus, [count][n] (act: the same pointer is allowed)
    const ulonglong2 *Wf, *Wi;                              // t_j's forward / inverse tables
    u64 t, one_s;
    u64 P;                                                  // t_0 ... t_{j-1} (1 for j = 0)
    u64 Pinv, Pinv_s;                                       // P^-1 mod t_j and its Shoup companion (unused for j = 0)
};
struct SlotCrtArgs {
    SlotCrtMod m[CRC_SLOTS_CRT_MAX];
    int r;
    long long *vals_out; const u32 *idx;                    // decompose: as SlotArgs (idx depends on n only)
    size_t count, item_stride, slot_stride;
    int n, logn, slots;
    u64 T, half;                                            // t_0 ... t_{r-1} and (T - 1) / 2
    u64 D, recip;                                           // act: as SlotActArgs
    int relu; u64 cap;                                      // cap = 0: none; otherwise 1 <= cap <= (T - 1) / 2
};

// canonical a mod t_j -> the running value with modulus j folded in
__device__ __forceinline__ u64 slot_crt_fold(u64 x, u64 a, const SlotCrtMod &m)
{
    const u64 xr = mulmod_shoup(x, 1, m.one_s, m.t);
    const u64 d = a >= xr ? a - xr : a + m.t - xr;
    return x + m.P * mulmod_shoup(d, m.Pinv, m.Pinv_s, m.t);
}
// centred V -> act(V) = min(max(floor(V / D + 1/2), 0 if relu), cap if cap), as an integer.  |V| <= (T - 1) / 2 < 2^62 and D <= 2^62: the sums stay below 2^63
__device__ __forceinline__ long long slot_crt_act_value(long long m, const SlotCrtArgs &a)
{
    const bool neg = m < 0;
    const u64 mag = neg ? 0 - (u64)m : (u64)m;
    u64 qv = slot_quotient(mag + ((a.D - (neg ? 1 : 0)) >> 1), a.D, a.recip);
    if (neg) return a.relu ? 0 : -(long long)qv;
    if (a.cap && qv > a.cap) qv = a.cap;
    return (long long)qv;
}

// The r forward transforms and the Garner fold of one item into x[2 PAIRS], canonical mod T.  FUSE1 as in the bodies above: off for decompose (drained in slot
// order), on for the activation (position order).  Barriers as in slots_act_body: the fill and the fold give a lane the same slots of the image and
// ntt_row_passes returns synchronised, so a modulus needs ONE barrier of its own, between its fill and its passes.
template <bool LAZY, int PAIRS, bool FUSE1>
__device__ __forceinline__ void slots_crt_lift(const SlotCrtArgs &a, size_t item, u64 *sm, u64 (&x)[2 * PAIRS])
{
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const bool fuse1 = FUSE1 && ntt_fused_stage(a.logn);
    for (int j = 0; j < a.r; j++) {
        const SlotCrtMod &m = a.m[j];
        const u64 t = m.t, t2 = t + t, one_s = m.one_s;
        const u64 *src = m.plain_in + item * (size_t)n;
        for (int s = 2 * tid; s < n; s += 2 * nt) {
            const ulonglong2 p = ld2(src + s);
            sm_store_pair64(sm, s, mulmod_shoup(p.x, 1, one_s, t), mulmod_shoup(p.y, 1, one_s, t));
        }
        __syncthreads();
        ntt_row_passes<false, LAZY, 3, FUSE1>(sm, m.Wf, n, a.logn, t, t2);
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            const int s = 2 * tid + 2 * k * nt;
            if (s < n) {
                ulonglong2 v = sm_load_pair64(sm, s);
                if (fuse1) fwd_pair_stage<LAZY>(v, m.Wf[(n >> 1) + (s >> 1)], t, t2);
                const u64 ax = mulmod_shoup(v.x, 1, one_s, t), ay = mulmod_shoup(v.y, 1, one_s, t);     // below (1 + 4 log2 n) t (lazy) / 4 t (strict) -> canonical
                x[2 * k] = j ? slot_crt_fold(x[2 * k], ax, m) : ax;
                x[2 * k + 1] = j ? slot_crt_fold(x[2 * k + 1], ay, m) : ay;
            }
        }
    }
}

// Each lane writes its centred values over its own slots of the image; one barrier; the drain in slot order through idx, with the caller's strides.
template <bool LAZY, int PAIRS>
__device__ __forceinline__ void slots_crt_decompose_body(const SlotCrtArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    u64 x[2 * PAIRS];
    slots_crt_lift<LAZY, PAIRS, false>(a, item, sm, x);
#pragma unroll
    for (int k = 0; k < PAIRS; k++) {
        const int s = 2 * tid + 2 * k * nt;
        if (s < n) sm_store_pair64(sm, s, x[2 * k] > a.half ? x[2 * k] - a.T : x[2 * k], x[2 * k + 1] > a.half ? x[2 * k + 1] - a.T : x[2 * k + 1]);
    }
    __syncthreads();
    long long *out = a.vals_out + item * a.item_stride;
    for (int i = tid; i < a.slots; i += nt) out[(size_t)i * a.slot_stride] = (long long)sm[lpad((int)a.idx[i])];
}

// The lift in position order, the activation on the centred integer, then for every modulus: the residue, t_j's inverse passes, the canonical store to output
// row j.  The workgroup has read all r input rows before its first store, so input row j may be output row j.  The store of modulus j reads, and the fill of
// modulus j + 1 writes, the lane's own slots: one barrier per modulus, in front of the inverse passes.
template <bool LAZY, int PAIRS>
__device__ __forceinline__ void slots_crt_act_body(const SlotCrtArgs &a, u64 *sm)
{
    size_t item;
    if (!slot_item(a.count, item)) return;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const bool fuse1 = ntt_fused_stage(a.logn);
    u64 x[2 * PAIRS];
    slots_crt_lift<LAZY, PAIRS, true>(a, item, sm, x);
#pragma unroll
    for (int k = 0; k < 2 * PAIRS; k++) {
        if (2 * tid + 2 * (k >> 1) * nt < n) x[k] = (u64)slot_crt_act_value((long long)(x[k] > a.half ? x[k] - a.T : x[k]), a);
    }
    for (int j = 0; j < a.r; j++) {
        const SlotCrtMod &m = a.m[j];
        const u64 t = m.t, t2 = t + t, one_s = m.one_s;
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            const int s = 2 * tid + 2 * k * nt;
            if (s < n) {
                ulonglong2 v;
                v.x = slot_residue((long long)x[2 * k], t, one_s); v.y = slot_residue((long long)x[2 * k + 1], t, one_s);
                if (fuse1) inv_pair_stage<LAZY>(v, m.Wi[(n >> 1) + (s >> 1)], t, t2);
                sm_store_pair64(sm, s, v.x, v.y);
            }
        }
        __syncthreads();
        ntt_row_passes<true, LAZY, 3, true>(sm, m.Wi, n, a.logn, t, t2);
        u64 *dst = m.plain_out + item * (size_t)n;
        for (int s = 2 * tid; s < n; s += 2 * nt) {
            const ulonglong2 r = sm_load_pair64(sm, s);                    // below 16 t (lazy) / 2 t (strict)
            st2(dst + s, mulmod_shoup(r.x, 1, one_s, t), mulmod_shoup(r.y, 1, one_s, t));
        }
    }
}
