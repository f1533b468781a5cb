// slots_device.h -- device side of slot batching (kernels_slots.hip): argument block, block -> item order, the bodies of slots_compose_kernel and
// slots_decompose_kernel.  A header so that tests/cpp/slots_kernel_check.cpp can run the same text on the CPU, one thread per workgroup, under sanitizers.
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

__device__ __forceinline__ bool slot_item(const SlotArgs &a, size_t &item)
{
    size_t grp; unsigned member;
    if (!xcd_group(blockIdx.x, CRC_SLOT_GROUP, (a.count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP, grp, member)) return false;
    item = grp * CRC_SLOT_GROUP + member;
    return item < a.count;
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
    if (!slot_item(a, item)) return;
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
    if (!slot_item(a, item)) return;
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
