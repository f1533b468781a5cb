// slots_device.h -- device side of slot batching (kernels_slots.hip): argument block, block -> item order, the bodies of slots_compose_kernel and
// slots_decompose_kernel, and of slots_rescale_kernel.  A header so that tests/cpp/slots_kernel_check.cpp and slots_rescale_kernel_check.cpp can run the same
// text on the CPU, one thread per workgroup, under sanitizers.
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
