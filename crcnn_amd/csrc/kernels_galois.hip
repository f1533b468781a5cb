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
//
// Below it: the same automorphism on NTT-FORM rows, where it is an index gather alone (galois_permute_ntt_kernel), and that gather folded into a sum of
// plaintext products (galois_diag_mac_kernel) -- the hoisted rotations and the diagonal product of abi.hip.
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
    const u64 q = mods[i].q, inv = bp->ksk_inv_qhat[i], invs = bp->ksk_inv_qhat_s[i];
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

// ---- the automorphism on NTT-form rows ----
// A row in NTT form holds X[i] = p(psi^(2 brev(i) + 1)) (brev: the bit reversal over log2 n bits; psi the modulus' primitive 2n-th root), so
// NTT(sigma_g(p))[i] = p(psi^(g (2 brev(i) + 1))) = X[pi_g(i)] with 2 brev(pi_g(i)) + 1 = g (2 brev(i) + 1) mod 2n: an index gather that knows nothing of the modulus, with
// no negation and no transform.  32-bit index arithmetic: the product is taken mod 2n, a power of two, so a wrap at 2^32 changes nothing.  pi_g(i) < n for every i < n,
// because an odd residue below 2n minus one, halved, is below n and the reversal keeps log2 n bits.
__device__ __forceinline__ u32 galois_ntt_src(u32 i, u32 g, u32 m2, int sh)
{
    const u32 e = (g * (2u * (__brev(i) >> sh) + 1u)) & m2;         // odd, < 2n
    return __brev(e >> 1) >> sh;
}
// in, out [rows][n]; grid: rows max(1, n / 512) workgroups of 256 threads, a thread owns the outputs i, i + 1 (one 16-byte store; the 8-byte reads are scattered
// over a row that sits in L2)
__global__ void __launch_bounds__(256) galois_permute_ntt_kernel(const u64 *in, u64 *out, int n, int logn, int blocks_per_row, u32 g)
{
    const size_t row = blockIdx.x / (u32)blocks_per_row; const u32 part = blockIdx.x - (u32)row * (u32)blocks_per_row;
    const u32 i = (part * 256u + threadIdx.x) * 2u;
    if (i >= (u32)n) return;                                   // n < 512: the tail of the one workgroup of a row
    const u32 m2 = 2u * (u32)n - 1u; const int sh = 32 - logn;
    const u64 *src = in + row * (size_t)n;
    st2(out + row * (size_t)n + i, src[galois_ntt_src(i, g, m2, sh)], src[galois_ntt_src(i + 1u, g, m2, sh)]);
}
int k_galois_permute_ntt(crc_ctx *c, const u64 *in, size_t rows, u64 g, u64 *out, hipStream_t st)
{
    if (rows == 0) return CRC_OK;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = rows * bpr;
    if (blocks > 0x7fffffffull) return CRC_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(galois_permute_ntt_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, out, c->n, c->logn, bpr, (u32)g);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}

// ---- the diagonal product: y = Sum_r P_r (*) sigma_{g_r}(Z_r), the gather of the kernel above folded into the product ----
// Z_r [cnt][2][k][n]: NTT-form ciphertexts (the key switch's results before their automorphism), P_r [k][n]: NTT-form plaintext rows, y [cnt][2][k][n].
// y[s] = Sum_r P_r[s] Z_r[pi_r(s)] mod q_j, so the R permuted ciphertexts are never written.  The products are summed as 128-bit integers and reduced once: with
// canonical operands a product is below q^2, the launcher keeps R q^2 + q below 2^128 (R <= 32 for moduli of up to 61 bits), and barrett128 is exact for every
// 128-bit value -- the canonical residue of the sum, which is what R canonical products added mod q give.
struct GaloisDiagArgs { const u64 *z[GALOIS_DIAG_MAX]; const u64 *p[GALOIS_DIAG_MAX]; u32 g[GALOIS_DIAG_MAX]; };
__global__ void __launch_bounds__(256) galois_diag_mac_kernel(GaloisDiagArgs a, int R, u64 *y, const ModParams *mods, int n, int logn, int k, int blocks_per_row,
                                                              int accumulate)
{
    const size_t row = blockIdx.x / (u32)blocks_per_row; const u32 part = blockIdx.x - (u32)row * (u32)blocks_per_row;      // row = (ct 2 + poly) k + j
    const u32 s = (part * 256u + threadIdx.x) * 2u;
    if (s >= (u32)n) return;
    const int j = (int)(row % (size_t)k);
    const ModParams m = mods[j];
    const u32 m2 = 2u * (u32)n - 1u; const int sh = 32 - logn;
    unsigned __int128 acc0 = 0, acc1 = 0;
    u64 *yo = y + row * (size_t)n + s;
    if (accumulate) { const ulonglong2 v = ld2(yo); acc0 = v.x; acc1 = v.y; }
    for (int r = 0; r < R; r++) {
        const u64 *zr = a.z[r] + row * (size_t)n;
        const ulonglong2 w = ld2(a.p[r] + (size_t)j * n + s);
        const u32 g = a.g[r];
        u64 lo, hi;
        mul64wide(w.x, zr[galois_ntt_src(s, g, m2, sh)], lo, hi); acc0 += ((unsigned __int128)hi << 64) | lo;
        mul64wide(w.y, zr[galois_ntt_src(s + 1u, g, m2, sh)], lo, hi); acc1 += ((unsigned __int128)hi << 64) | lo;
    }
    st2(yo, barrett128((u64)acc0, (u64)(acc0 >> 64), m), barrett128((u64)acc1, (u64)(acc1 >> 64), m));
}
// the elements one launch may sum: R q_max^2 + q_max < 2^128
static int diag_group(const crc_ctx *c)
{
    int bits = 0;
    for (int i = 0; i < c->k; i++) if ((int)c->tabs[i].m.bits > bits) bits = c->tabs[i].m.bits;
    const int room = 127 - 2 * bits;
    return room >= 5 ? GALOIS_DIAG_MAX : room > 0 ? 1 << room : 1;
}
int k_galois_diag_mac(crc_ctx *c, const u64 *const *z, const u64 *const *p, const u64 *g, int R, size_t cnt, bool accumulate, u64 *y, hipStream_t st)
{
    if (cnt == 0 || R < 1) return CRC_OK;
    if (R > GALOIS_DIAG_MAX) return CRC_ERR_INVALID_ARGUMENT;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = cnt * 2 * (size_t)c->k * bpr;
    if (blocks > 0x7fffffffull) return CRC_ERR_INVALID_ARGUMENT;
    for (int r0 = 0, per = diag_group(c); r0 < R; r0 += per) {
        GaloisDiagArgs a{};
        const int rn = R - r0 < per ? R - r0 : per;
        for (int r = 0; r < rn; r++) { a.z[r] = z[r0 + r]; a.p[r] = p[r0 + r]; a.g[r] = (u32)g[r0 + r]; }
        hipLaunchKernelGGL(galois_diag_mac_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, rn, y, c->d_mods, c->n, c->logn, c->k, bpr,
                           accumulate || r0 ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// ---- baby-step / giant-step: G inner sums over the same B rotated inputs, and the sum of the G rotated results ----
// u_j[s] = Sum_b P[j][b][s] Z_b[pi_b(s)] mod q for GALOIS_MULTI_JT giant indices j per thread: Z_b[pi_b(s)] is gathered once and multiplied into JT pairs of 128-bit
// accumulators, so the B rotated inputs are read ceil(G / JT) times instead of G times.  One barrett128 per output, the bound and the accumulate continuation of
// galois_diag_mac_kernel.  p: &P[0][b0] of P [G][Bt][k][n] (pj = Bt k n words from one giant index to the next), u [G][cnt][2][k][n] (uj = cnt 2 k n words).
// grid: (cnt 2 k max(1, n / 512), ceil(G / JT)); a last tile with fewer than JT outputs computes its missing ones on the last giant index and does not store them
struct GaloisMultiArgs { const u64 *z[GALOIS_DIAG_MAX]; u32 g[GALOIS_DIAG_MAX]; };
template <int JT>
__global__ void __launch_bounds__(256, 8) galois_diag_mac_multi_kernel(GaloisMultiArgs a, int R, const u64 *p, size_t pj, int G, u64 *u, size_t uj, const ModParams *mods,
                                                                    int n, int logn, int k, int blocks_per_row, int accumulate)
{
    const size_t row = blockIdx.x / (u32)blocks_per_row; const u32 part = blockIdx.x - (u32)row * (u32)blocks_per_row;      // row = (ct 2 + poly) k + i
    const u32 s = (part * 256u + threadIdx.x) * 2u;
    if (s >= (u32)n) return;
    const int i = (int)(row % (size_t)k);
    const ModParams m = mods[i];
    const u32 m2 = 2u * (u32)n - 1u; const int sh = 32 - logn;
    const int j0 = (int)blockIdx.y * JT;
    unsigned __int128 acc0[JT], acc1[JT];
    size_t po[JT];                                                         // (uniform: the tile's giant rows of P from the thread's own pointer)
    u64 *uo = u + (size_t)j0 * uj + row * (size_t)n + s;
#pragma unroll
    for (int t = 0; t < JT; t++) {
        po[t] = (size_t)(j0 + t < G ? t : G - 1 - j0) * pj;
        acc0[t] = 0; acc1[t] = 0;
        if (accumulate && j0 + t < G) { const ulonglong2 v = ld2(uo + (size_t)t * uj); acc0[t] = v.x; acc1[t] = v.y; }
    }
    const u64 *pr = p + (size_t)j0 * pj + (size_t)i * n + s;
    for (int r = 0; r < R; r++, pr += (size_t)k * n) {                      // (k n words from one baby row of P to the next)
        const u64 *zr = a.z[r] + row * (size_t)n;
        const u32 g = a.g[r];
        const u64 za = zr[galois_ntt_src(s, g, m2, sh)], zb = zr[galois_ntt_src(s + 1u, g, m2, sh)];
#pragma unroll
        for (int t = 0; t < JT; t++) {
            const ulonglong2 w = ld2(pr + po[t]);
            u64 lo, hi;
            mul64wide(w.x, za, lo, hi); acc0[t] += ((unsigned __int128)hi << 64) | lo;
            mul64wide(w.y, zb, lo, hi); acc1[t] += ((unsigned __int128)hi << 64) | lo;
        }
    }
#pragma unroll
    for (int t = 0; t < JT; t++)
        if (j0 + t < G) st2(uo + (size_t)t * uj, barrett128((u64)acc0[t], (u64)(acc0[t] >> 64), m), barrett128((u64)acc1[t], (u64)(acc1[t] >> 64), m));
}
// z: the B key-switch results of the pass, g their elements; p = P [G][B][k][n]; u [G][cnt] (+)= the G inner sums
int k_galois_diag_mac_multi(crc_ctx *c, const u64 *const *z, const u64 *g, int b0, int R, int B, const u64 *p, int G, size_t cnt, bool accumulate, u64 *u,
                            hipStream_t st)
{
    if (cnt == 0 || R < 1 || G < 1) return CRC_OK;
    if (R > GALOIS_DIAG_MAX || G > GALOIS_BSGS_MAX) return CRC_ERR_INVALID_ARGUMENT;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = cnt * 2 * (size_t)c->k * bpr, rowp = (size_t)c->k * c->n;
    if (blocks > 0x7fffffffull) return CRC_ERR_INVALID_ARGUMENT;
    const dim3 grid((unsigned)blocks, (unsigned)((G + GALOIS_MULTI_JT - 1) / GALOIS_MULTI_JT));
    for (int r0 = 0, per = diag_group(c); r0 < R; r0 += per) {
        GaloisMultiArgs a{};
        const int rn = R - r0 < per ? R - r0 : per;
        for (int r = 0; r < rn; r++) { a.z[r] = z[r0 + r]; a.g[r] = (u32)g[r0 + r]; }
        hipLaunchKernelGGL(galois_diag_mac_multi_kernel<GALOIS_MULTI_JT>, grid, dim3(256), 0, st, a, rn, p + (size_t)(b0 + r0) * rowp, (size_t)B * rowp, G, u,
                           cnt * 2 * rowp, c->d_mods, c->n, c->logn, c->k, bpr, accumulate || r0 ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// y[s] (+)= Sum_j Z_j[pi_{g_j}(s)] mod q: the gather of galois_permute_ntt_kernel summed over up to GALOIS_DIAG_MAX NTT-form ciphertexts (g_j = 1: Z_j itself), so the
// rotated ciphertexts are never written.  Canonical operands, one conditional subtraction per term: the canonical residue of the sum
struct GaloisSumArgs { const u64 *z[GALOIS_DIAG_MAX]; u32 g[GALOIS_DIAG_MAX]; };
__global__ void __launch_bounds__(256) galois_sum_permuted_kernel(GaloisSumArgs a, int R, u64 *y, const ModParams *mods, int n, int logn, int k, int blocks_per_row,
                                                                  int accumulate)
{
    const size_t row = blockIdx.x / (u32)blocks_per_row; const u32 part = blockIdx.x - (u32)row * (u32)blocks_per_row;
    const u32 s = (part * 256u + threadIdx.x) * 2u;
    if (s >= (u32)n) return;
    const u64 q = mods[(int)(row % (size_t)k)].q;
    const u32 m2 = 2u * (u32)n - 1u; const int sh = 32 - logn;
    u64 *yo = y + row * (size_t)n + s;
    ulonglong2 acc{0, 0};
    if (accumulate) acc = ld2(yo);
    for (int r = 0; r < R; r++) {
        const u64 *zr = a.z[r] + row * (size_t)n;
        const u32 g = a.g[r];
        acc.x = addmod(acc.x, zr[galois_ntt_src(s, g, m2, sh)], q);
        acc.y = addmod(acc.y, zr[galois_ntt_src(s + 1u, g, m2, sh)], q);
    }
    st2(yo, acc.x, acc.y);
}
int k_galois_sum_permuted(crc_ctx *c, const u64 *const *z, const u64 *g, int R, size_t cnt, bool accumulate, u64 *y, hipStream_t st)
{
    if (cnt == 0 || R < 1) return CRC_OK;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = cnt * 2 * (size_t)c->k * bpr;
    if (blocks > 0x7fffffffull) return CRC_ERR_INVALID_ARGUMENT;
    for (int r0 = 0; r0 < R; r0 += GALOIS_DIAG_MAX) {
        GaloisSumArgs a{};
        const int rn = R - r0 < GALOIS_DIAG_MAX ? R - r0 : (int)GALOIS_DIAG_MAX;
        for (int r = 0; r < rn; r++) { a.z[r] = z[r0 + r]; a.g[r] = (u32)g[r0 + r]; }
        hipLaunchKernelGGL(galois_sum_permuted_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, rn, y, c->d_mods, c->n, c->logn, c->k, bpr,
                           accumulate || r0 ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// ---- the packed convolution: y[co] = Sum_ci Sum_tau w[co][ci][tau] sigma_{g_tau}(Z_tau[ci]) with SCALAR weights ----
// The multi kernel above with its P row loads replaced by one residue per (modulus, output channel, input channel, tap): a constant plaintext's NTT-form row holds
// the same word at every position.  z[r]: the pass' key-switch results for tap r, ch NTT-form ciphertexts that are the flat ciphertexts o .. o + ch - 1 of
// x [Cin][count] (flat index ci count + ct), so a pass may begin and end inside a channel.  A workgroup owns 512 positions of one output row (ct, poly, modulus i) and
// JT output channels; it walks the pass' input channels that hold a ciphertext of ITS ct -- ci count + ct in [o, o + ch), cut to the launch's [cA, cB) -- and the R
// taps, gathers Z_r[pi_r(s)] once and multiplies it into JT pairs of 128-bit accumulators.  The weights w [k][Cout][Cin][T] (w points at tap r0 of the launch) are
// uniform over the workgroup: their addresses depend on blockIdx and loop counters alone, so they come over the scalar path and hold no VGPR.  One barrett128 per
// output; the launcher keeps (cB - cA) R q_max^2 + q_max below 2^128.  A row is first written by the launch that holds its channel 0 and tap 0 (first = the launch
// starts at tap 0) and accumulated into by every other; a workgroup with no channel of its ct in the launch leaves its row alone.  A last tile with fewer than JT
// outputs computes its missing ones with the weights of channel Cout - 1 and does not store them.
// grid: (count 2 k max(1, n / 512), ceil(Cout / JT))
// EPI (crc_conv_slots_bias_mask_forms): an epilogue on the launch's own reduced sum, y = y_old + mask (.) (barrett128(Sum) [+ bias on polynomial 0, in the launch
// that first writes the row]).  Exact arithmetic in Z_q on canonical residues, so mask (.) (A + B) = mask (.) A + mask (.) B over the launches of a row: y_old, which
// earlier launches have masked already, stays outside the product, and the bias enters with the one launch that does not accumulate.  bias [k][Cout] (or null) is
// uniform over the workgroup like the weights; mask [k][n] (or null) is one 16-byte load at the row's own position, issued after the tap loop, when the gather's
// registers are dead, as is the read of y_old.  EPI = false is the kernel without any of this: bias and mask are not looked at
struct GaloisConvArgs { const u64 *z[GALOIS_DIAG_MAX]; u32 g[GALOIS_DIAG_MAX]; };
template <int JT, bool EPI>
__global__ void __launch_bounds__(256, JT <= 4 ? 8 : 4) galois_conv_mac_kernel(GaloisConvArgs a, int R, const u64 *__restrict__ w, int T, int Cin, int Cout, size_t o,
                                                                             size_t ch, size_t count, int cA, int cB, int first, u64 *y, const ModParams *mods, int n,
                                                                             int logn, int k, int blocks_per_row, const u64 *__restrict__ bias,
                                                                             const u64 *__restrict__ mask)
{
    const size_t row = blockIdx.x / (u32)blocks_per_row; const u32 part = blockIdx.x - (u32)row * (u32)blocks_per_row;      // row = (ct 2 + poly) k + i
    const u32 s = (part * 256u + threadIdx.x) * 2u;
    if (s >= (u32)n) return;
    const size_t ct = row / (2u * (u32)k); const u32 pk = (u32)(row - ct * 2u * (u32)k);                                    // pk = poly k + i
    const int i = (int)(pk >= (u32)k ? pk - (u32)k : pk);
    const size_t end = o + ch;
    int lo = o > ct ? (int)((o - ct + count - 1) / count) : 0, hi = end > ct ? (int)((end - ct + count - 1) / count) : 0;   // ci count + ct in [o, end)
    if (lo < cA) lo = cA;
    if (hi > cB) hi = cB;
    if (lo >= hi) return;
    const bool accumulate = !(first && lo == 0);
    const ModParams m = mods[i];
    const u32 m2 = 2u * (u32)n - 1u; const int sh = 32 - logn;
    const int j0 = (int)blockIdx.y * JT;
    unsigned __int128 acc0[JT], acc1[JT];
    const u64 *wt[JT];                                                     // (uniform: w[i][co][0][r0 ..])
    const size_t yj = count * 2 * (size_t)k * n;                           // words from one output channel to the next
    u64 *yo = y + (size_t)j0 * yj + row * (size_t)n + s;
#pragma unroll
    for (int t = 0; t < JT; t++) {
        wt[t] = w + ((size_t)i * Cout + (j0 + t < Cout ? j0 + t : Cout - 1)) * Cin * (size_t)T;
        acc0[t] = 0; acc1[t] = 0;
        if (!EPI && accumulate && j0 + t < Cout) { const ulonglong2 v = ld2(yo + (size_t)t * yj); acc0[t] = v.x; acc1[t] = v.y; }
    }
    for (int ci = lo; ci < hi; ci++) {
        const size_t zo = (((size_t)ci * count + ct - o) * 2 * (size_t)k + pk) * n, wo = (size_t)ci * T;
        for (int r = 0; r < R; r++) {
            const u64 *zr = a.z[r] + zo;
            const u32 g = a.g[r];
            const u64 za = zr[galois_ntt_src(s, g, m2, sh)], zb = zr[galois_ntt_src(s + 1u, g, m2, sh)];
#pragma unroll
            for (int t = 0; t < JT; t++) {
                const u64 wv = wt[t][wo + r];
                u64 l, h;
                mul64wide(wv, za, l, h); acc0[t] += ((unsigned __int128)h << 64) | l;
                mul64wide(wv, zb, l, h); acc1[t] += ((unsigned __int128)h << 64) | l;
            }
        }
    }
    if (!EPI) {
#pragma unroll
        for (int t = 0; t < JT; t++)
            if (j0 + t < Cout) st2(yo + (size_t)t * yj, barrett128((u64)acc0[t], (u64)(acc0[t] >> 64), m), barrett128((u64)acc1[t], (u64)(acc1[t] >> 64), m));
        return;
    }
    const bool biased = bias && !accumulate && pk < (u32)k;                // polynomial 0 of a row that this launch writes first
    ulonglong2 mk{1, 1};
    if (mask) mk = ld2(mask + (size_t)i * n + s);
#pragma unroll
    for (int t = 0; t < JT; t++) {
        if (j0 + t >= Cout) continue;
        u64 r0 = barrett128((u64)acc0[t], (u64)(acc0[t] >> 64), m), r1 = barrett128((u64)acc1[t], (u64)(acc1[t] >> 64), m);
        if (biased) { const u64 b = bias[(size_t)i * Cout + j0 + t]; r0 = addmod(r0, b, m.q); r1 = addmod(r1, b, m.q); }
        if (mask) { r0 = mulmod(r0, mk.x, m); r1 = mulmod(r1, mk.y, m); }
        if (accumulate) { const ulonglong2 v = ld2(yo + (size_t)t * yj); r0 = addmod(r0, v.x, m.q); r1 = addmod(r1, v.y, m.q); }
        st2(yo + (size_t)t * yj, r0, r1);
    }
}
// the terms one reduction may sum: terms q_max^2 + q_max < 2^128 (diag_group's rule without its cap of one launch's pointers)
static int conv_terms(const crc_ctx *c)
{
    int bits = 0;
    for (int i = 0; i < c->k; i++) if ((int)c->tabs[i].m.bits > bits) bits = c->tabs[i].m.bits;
    const int room = 127 - 2 * bits;
    return room >= 20 ? 1 << 20 : room > 0 ? 1 << room : 1;
}
template <int JT>
static void conv_launch(crc_ctx *c, const GaloisConvArgs &a, int rn, const u64 *w, int T, int Cin, int Cout, size_t o, size_t ch, size_t count, int cA, int cB,
                        bool first, u64 *y, unsigned blocks, int bpr, const u64 *bias, const u64 *mask, hipStream_t st)
{
    const dim3 grid(blocks, (unsigned)((Cout + JT - 1) / JT));
    if (bias || mask)
        hipLaunchKernelGGL((galois_conv_mac_kernel<JT, true>), grid, dim3(256), 0, st, a, rn, w, T, Cin, Cout, o, ch, count, cA, cB, first ? 1 : 0, y, c->d_mods, c->n,
                           c->logn, c->k, bpr, bias, mask);
    else
        hipLaunchKernelGGL((galois_conv_mac_kernel<JT, false>), grid, dim3(256), 0, st, a, rn, w, T, Cin, Cout, o, ch, count, cA, cB, first ? 1 : 0, y, c->d_mods, c->n,
                           c->logn, c->k, bpr, bias, mask);
}
// z: the R <= GALOIS_DIAG_MAX key-switch results of the pass [o, o + ch) of the flat input [Cin][count], g their elements; w: &d_w[0][0][0][r0] of [k][Cout][Cin][T];
// first: r0 = 0; y [Cout][count]; jt: 2 | 4 | 8; bias [k][Cout] and mask [k][n], either may be null: the epilogue instantiation where one is given
int k_galois_conv_mac(crc_ctx *c, const u64 *const *z, const u64 *g, int R, const u64 *w, int T, int Cin, int Cout, size_t o, size_t ch, size_t count, bool first,
                      u64 *y, int jt, const u64 *bias, const u64 *mask, hipStream_t st)
{
    if (count == 0 || ch == 0 || R < 1) return CRC_OK;
    if (R > GALOIS_DIAG_MAX || Cin < 1 || Cout < 1 || o + ch > (size_t)Cin * count || (jt != 2 && jt != 4 && jt != 8)) return CRC_ERR_INVALID_ARGUMENT;
    const int bpr = c->n > 512 ? c->n / 512 : 1;
    const size_t blocks = count * 2 * (size_t)c->k * bpr;
    if (blocks > 0x7fffffffull || (size_t)(Cout + 1) / 2 > 65535) return CRC_ERR_INVALID_ARGUMENT;
    const int terms = conv_terms(c), per = R < terms ? R : terms, cper = terms / per;      // taps per launch; channels per launch (>= 1)
    const int c_lo = (int)(o / count), c_hi = (int)((o + ch - 1) / count) + 1;             // the pass' channels
    for (int r0 = 0; r0 < R; r0 += per) {
        GaloisConvArgs a{};
        const int rn = R - r0 < per ? R - r0 : per;
        for (int r = 0; r < rn; r++) { a.z[r] = z[r0 + r]; a.g[r] = (u32)g[r0 + r]; }
        for (int cA = c_lo; cA < c_hi; cA += cper) {
            const int cB = c_hi - cA < cper ? c_hi : cA + cper;
            const bool f = first && r0 == 0;
            if (jt == 2) conv_launch<2>(c, a, rn, w + r0, T, Cin, Cout, o, ch, count, cA, cB, f, y, (unsigned)blocks, bpr, bias, mask, st);
            else if (jt == 4) conv_launch<4>(c, a, rn, w + r0, T, Cin, Cout, o, ch, count, cA, cB, f, y, (unsigned)blocks, bpr, bias, mask, st);
            else conv_launch<8>(c, a, rn, w + r0, T, Cin, Cout, o, ch, count, cA, cB, f, y, (unsigned)blocks, bpr, bias, mask, st);
            HIPCHK(hipGetLastError());
        }
    }
    return CRC_OK;
}
