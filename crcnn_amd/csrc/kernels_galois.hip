// kernels_galois.hip -- the coefficient automorphism of Evaluator::apply_galois (evaluator.cpp:1587-1786) in the form the key switch takes.
//
// sigma_g on a coefficient row mod q (util::apply_galois, util/polyarithsmallmod.h:313-360): out[(i g) mod n] = in[i] where bit log2 n of i g is clear,
// q - in[i] (0 stays 0) where it is set.  SEAL then switches sigma(c1) with relinearisation's key switch and adds sigma(c0) to the first polynomial, so one pass
// writes what k_relinearize(..., c2_premul = true) reads: a size-3 row set whose third polynomial is sigma(c1) (q/q_i)^-1 and whose first two are what the key
// switch's tail adds.
//
// Written as a gather: with h = g^-1 mod 2n and r = (j h) mod 2n, out[j] = in[r] for r < n and -in[r - n] otherwise (i = r or r - n is the one index with
// i g = j or j + n mod 2n).  A thread owns the coefficients j, j + 1: its stores are 16 bytes wide and coalesced, only the 8-byte reads are strided (by the
// odd h, so the 64 lanes of a wave touch 64 different 128-byte lines of a row that sits in L2: 16-128 KiB).  j h < n 2n <= 2^29: 32-bit index arithmetic.
#include "kernels.h"
#include "ntt_device.h"

// x [count][2][k][n] coefficient form -> x3 [count][3][k][n]:
//   poly 0: sigma(c0)              accumulate: sigma(c0) + c0
//   poly 1: 0                      accumulate: c1
//   poly 2: sigma(c1) (q/q_i)^-1 mod q_i            (what relin_premul_kernel makes of a third polynomial)
// grid: count k max(1, n / 512) workgroups of 256 threads; a workgroup owns 512 consecutive coefficients of one (ciphertext, modulus) row pair
__global__ void __launch_bounds__(256) galois_permute_kernel(const u64 *x, u64 *x3, const ModParams *mods, const BehzParams *bp, int n, int k, int blocks_per_row,
                                                            u32 h, int accumulate)
{
    const u32 row = blockIdx.x / (u32)blocks_per_row, part = blockIdx.x - row * (u32)blocks_per_row;      // row = ct k + i
    const u32 ct = row / (u32)k; const int i = (int)(row - ct * (u32)k);
    const u32 j = (part * 256u + threadIdx.x) * 2u;
    if (j >= (u32)n) return;                                   // n < 512: the tail of the one workgroup of a row
    const u64 q = mods[i].q, inv = bp->inv_qhat[i], invs = bp->inv_qhat_s[i];
    const size_t kn = (size_t)k * n;
    const u64 *c0 = x + (size_t)ct * 2 * kn + (size_t)i * n, *c1 = c0 + kn;
    u64 *o0 = x3 + (size_t)ct * 3 * kn + (size_t)i * n, *o1 = o0 + kn, *o2 = o1 + kn;
    const u32 m2 = 2u * (u32)n - 1u, un = (u32)n;
    const u32 ra = (j * h) & m2, rb = (ra + h) & m2;           // (j + 1) h = j h + h
    const u32 ia = ra & (un - 1u), ib = rb & (un - 1u);
    u64 a0 = c0[ia], b0 = c0[ib], a1 = c1[ia], b1 = c1[ib];
    if (ra >= un) { a0 = negmod(a0, q); a1 = negmod(a1, q); }
    if (rb >= un) { b0 = negmod(b0, q); b1 = negmod(b1, q); }
    ulonglong2 p1{0, 0};
    if (accumulate) {
        const ulonglong2 s0 = ld2(c0 + j);
        a0 = addmod(a0, s0.x, q); b0 = addmod(b0, s0.y, q);
        p1 = ld2(c1 + j);
    }
    st2(o0 + j, a0, b0);
    st2(o1 + j, p1.x, p1.y);
    st2(o2 + j, mulmod_shoup(a1, inv, invs, q), mulmod_shoup(b1, inv, invs, q));
}

// g: a valid Galois element (odd, 1 <= g < 2n: the caller checks); x and x3 16-byte aligned and disjoint
int k_galois_permute(crc_ctx *c, const u64 *x, size_t cnt, u64 g, bool accumulate, u64 *x3, hipStream_t st)
{
    if (cnt == 0) return CRC_OK;
    const u64 two_n = 2 * (u64)c->n;
    u64 h = 1;                                                  // g^-1 mod 2n = g^(n - 1): the odd residues mod 2n are a group of order n and exponent n / 2
    for (u64 e = (u64)c->n - 1, b = g % two_n; e; e >>= 1, b = b * b % two_n) if (e & 1) h = h * b % two_n;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = cnt * (size_t)c->k * bpr;
    if (blocks > 0x7fffffffull) return CRC_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(galois_permute_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, x3, c->d_mods, c->d_behz, c->n, c->k, bpr, (u32)h, accumulate ? 1 : 0);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
