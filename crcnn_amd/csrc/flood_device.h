// flood_device.h -- device side of noise flooding (kernels_flood.hip): the sampler and the kernel that joins the flood to the tensor inside one row transform.
// A header so that tests/cpp/flood_kernel_check.cpp can run the same text on the CPU, one thread per workgroup, under sanitizers.
//
// A size-2 ciphertext (c0, c1) under the public key (p0, p1) becomes  c0' = c0 + p0 u + e1,  c1' = c1 + p1 u + e2  with u uniform ternary, e2 the encryptor's
// clipped normal and e1 UNIFORM on [-2^B, 2^B) (B = flood_bits, up to 126): a fresh encryption of zero whose error drowns whatever the evaluation left.
//   flood_sample_kernel   one lane per (ciphertext, coefficient pair), one ChaCha20 block (chacha.h, CHACHA_DOM_FLOOD): the ternary rows U [count][k][n] and the
//                         residues of e1, e2 E [count][2][k][n] into work space.  e1 = x - 2^B with x of B + 1 bits, reduced from a 128-bit word (mod128_any)
//   (the row transform of kernels.hip takes U to NTT form in place)
//   flood_join_kernel     one workgroup per row (ciphertext, polynomial p, modulus i); the tensor row is read once and written once, in its own form:
//       NTT form:          the image is the E row, transformed forward; the drain adds U . p_p and the tensor row          (no inverse transform anywhere)
//       coefficient form:  the image is U . p_p, transformed back; the drain adds the E row (residues: e1 is too wide for bytes) and the tensor row
#pragma once
#include "ntt_device.h"
#include "chacha.h"
#include "enc_sampler.h"

#ifndef CRC_MAXK
#define CRC_MAXK 8
#endif

struct FloodArgs {                                      // by value in the kernels' argument block
    u64 *ct;                                            // [count][2][k][n], flooded in place
    const u64 *pk;                                      // [2][k][n], NTT form
    u64 *U, *E;                                         // work space: [count][k][n] and [count][2][k][n]
    const ulonglong2 *W;                                // [k][n] {root power, Shoup companion}: forward tables (NTT-form tensor), inverse-div-2 (coefficient form)
    size_t count;
    int n, logn, k, flood_bits;
    u64 stream_base;
    ModParams mods[CRC_MAXK];
    u64 one_s[CRC_MAXK];                                // floor(2^64 / q_i): mulmod_shoup(v, 1, one_s, q) is v mod q for any 64-bit v
    u64 pow2b[CRC_MAXK];                                // 2^B mod q_i
    ChaChaKey key;
    EncCdt cdt;
};

// grid: count * ceil(n / 2 / blockDim) blocks
__device__ __forceinline__ void flood_sample_body(const FloodArgs &a)
{
    const int pairs = a.n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (m >= a.count || pr >= pairs) return;
    const int s = 2 * pr, k = a.k;
    const size_t n = (size_t)a.n;
    const u64 sid = a.stream_base + m;
    u32 b[16];
    chacha20_block(a.key, 0, (u32)sid, (u32)(sid >> 32), ((u32)CHACHA_DOM_FLOOD << 24) | (u32)s, b);
    // x keeps the low B + 1 bits of the 128-bit word: B + 1 <= 64 leaves the low word alone, else the high word keeps B - 63 <= 63 bits
    const int xb = a.flood_bits + 1;
    const u64 mlo = xb >= 64 ? ~(u64)0 : ((u64)1 << xb) - 1, mhi = xb > 64 ? ((u64)1 << (xb - 64)) - 1 : 0;
    u32 tv[2]; int e2[2]; u64 xl[2], xh[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const u32 *w = b + 8 * c;
        tv[c] = ternary_field(w[0], w[1]);
        e2[c] = cdt_noise(w[2], w[3], w[7] >> 31, a.cdt);
        xl[c] = ((u64)w[4] | ((u64)w[5] << 32)) & mlo;
        xh[c] = ((u64)w[6] | ((u64)w[7] << 32)) & mhi;
    }
    for (int i = 0; i < k; i++) {
        const ModParams md = a.mods[i];
        const u64 q = md.q, qm1 = q - 1;
        st2(a.U + (m * k + i) * n + s, tv[0] == 0 ? 0 : (tv[0] == 1 ? 1 : qm1), tv[1] == 0 ? 0 : (tv[1] == 1 ? 1 : qm1));
        u64 r1[2], r2[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            r1[c] = submod(mod128_any(xl[c], xh[c], md), a.pow2b[i], q);
            r2[c] = e2[c] >= 0 ? (u64)e2[c] : q - (u64)(-e2[c]);
        }
        st2(a.E + ((m * 2) * k + i) * n + s, r1[0], r1[1]);
        st2(a.E + ((m * 2 + 1) * k + i) * n + s, r2[0], r2[1]);
    }
}

// grid: xcd_grid(count * k, 2) -- the two polynomials of a (ciphertext, modulus) read the same U row, so they share an XCD; LDS: n words
template <bool INV, bool LAZY>
__device__ __forceinline__ void flood_join_body(const FloodArgs &a, u64 *sm)
{
    size_t grp; unsigned p;
    if (!xcd_group(blockIdx.x, 2u, a.count * (size_t)a.k, grp, p)) return;
    const size_t m = grp / (size_t)a.k;
    const int i = (int)(grp - m * (size_t)a.k);
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const ModParams md = a.mods[i];
    const u64 q = md.q, one_s = a.one_s[i];
    const size_t row = ((m * 2 + p) * (size_t)a.k + i) * (size_t)n;
    const u64 *u = a.U + grp * (size_t)n, *key = a.pk + ((size_t)p * a.k + i) * (size_t)n, *e = a.E + row;
    u64 *c = a.ct + row;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        if (INV) { const ulonglong2 uv = ld2(u + s), kv = ld2(key + s); sm_store_pair64(sm, s, mulmod(uv.x, kv.x, md), mulmod(uv.y, kv.y, md)); }
        else { const ulonglong2 v = ld2(e + s); sm_store_pair64(sm, s, v.x, v.y); }
    }
    __syncthreads();
    ntt_row_passes<INV, LAZY, 3, false>(sm, a.W + (size_t)i * n, n, a.logn, q, q + q);
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // forward: below (1 + 4 log2 n) q (lazy) / 4 q (strict); inverse: below 16 q / 2 q
        u64 x = mulmod_shoup(r.x, 1, one_s, q), y = mulmod_shoup(r.y, 1, one_s, q);
        if (INV) { const ulonglong2 ev = ld2(e + s); x = addmod(x, ev.x, q); y = addmod(y, ev.y, q); }
        else { const ulonglong2 uv = ld2(u + s), kv = ld2(key + s); x = addmod(x, mulmod(uv.x, kv.x, md), q); y = addmod(y, mulmod(uv.y, kv.y, md), q); }
        const ulonglong2 cv = ld2(c + s);
        st2(c + s, addmod(cv.x, x, q), addmod(cv.y, y, q));
    }
}
