// kernels_relin64.hip -- relinearisation's key switching over TWO fp64 NTT primes instead of the k coefficient moduli.
//
// Reference: Evaluator::relinearize_one_step (evaluator.cpp:934-1069).  For every target modulus q_j and output polynomial the reference forms
//     R_j = sum_{i < k} sum_{d < L_i}  e_{i,d} (*) key_{i,d}[j]  mod q_j  ((*) = negacyclic product, e_{i,d} = digit d of c2 (q/q_i)^-1 mod q_i) with 4 k^2
//     forward transforms over the 55-bit primes (every digit polynomial under every q_j), 2 k inverse ones, and adds c0, c1.  The digits are below 2^dbc (16
//     bits) and the key residues below q_j, so over the INTEGERS |R_j| <= n D 2^dbc q_j / 2 (keys taken as centred residues) < 2^90: R_j is a fixed integer
//     polynomial, and its residue mod q_j -- all the reference needs -- can be had from its residues modulo ANY primes whose product exceeds 2 |R_j|.  We take
//     the two fp64 primes of the context (p_0 p_1 ~ 2^94, f64mod.h): 2 D forward transforms of 16-bit polynomials and 2 * 2k inverse ones per ciphertext in
//     6-flop fp64 arithmetic, the keys re-expressed once per call (inverse transform mod q_j, centre, reduce mod p_m, forward transform mod p_m, times n^-1), a
//     CRT lift per coefficient.  Same element of Z_q, hence the same bits (goldens: tests/golden/ops_*.npz ref_relin*, layers / nets).
//   K1 relin_digits_f64_kernel : one workgroup per (ciphertext, i): the L_i digits of row c2'_i, each transformed under p_0 and p_1 in LDS  -> E  [ct][g][m][n]
//   K2 relin_mac_f64_kernel  : per slot: A[ct][poly][j][m] = sum_g E[ct][g][m] Kf[g][poly][j][m]  (lazy sum of reduced products, < 42 p)  -> A  [ct][2k][m][n]
//   K3 relin_inv_crt_kernel    : one workgroup per (ciphertext, poly, j): both inverse transforms, CRT lift, mod q_j, + c_poly; coefficient form out, or the
//                                forward transform over q_j in the same LDS image for an NTT-resident result
#include "kernels.h"
#include "ntt_device.h"

#include "ntt_f64.h"
#include "f64_launch.h"


struct Relin64Tab { unsigned char L[CRC_MAXK], g0[CRC_MAXK]; };

// ---- key preparation (once per call) ------------------------------------------------------------------------------------------------------------------------
// evaluation keys as SEAL hands
// them over (NTT form over q_j, residues possibly lazy / non-canonical) -> canonical
__global__ void __launch_bounds__(256) evk_canon_kernel(const u64 *evk, u64 *out, const ModParams *mods, int n, int k)
{
    const size_t row = blockIdx.x;
    const ModParams m = mods[row % k];
    const u64 *src = evk + row * (size_t)n; u64 *dst = out + row * (size_t)n;
    for (int s = threadIdx.x; s < n; s += blockDim.x) dst[s] = barrett128(src[s], 0, m);
}
// kc: the keys in coefficient form over q_j, rows [2 g + poly][j] (blob order)  ->  Kf [g][poly k + j][m][n]: centred residue mod p_m, forward transform, times
// n^-1
template <int RB>
__global__ void __launch_bounds__(RB == 5 ? 512 : 1024) relin_keys_f64_kernel(const u64 *kc, double *Kf, const ModParams *mods, const double *Wf,
    F64Params fp, int n, int logn, int k)
{
    extern __shared__ double smd[];
    const int m = blockIdx.x % CRC_NF64; const size_t row = blockIdx.x / CRC_NF64;       // row = (2 g + poly) k + j
    const int j = (int)(row % k); const size_t gp = row / k; const size_t g = gp >> 1; const int poly = (int)(gp & 1);
    const u64 q = mods[j].q;
    const F64Mod md = fp.m[m];
    const double *W = Wf + (size_t)m * n;
    const u64 *src = kc + row * (size_t)n;
    auto cen = [&](u64 v) { return f64_from_i64(v > (q >> 1) ? (long long)v - (long long)q : (long long)v, md); };
    for (int s = 2 * threadIdx.x; s < n; s += 2 * blockDim.x) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src + s);
        sm_store_pair<RB>(smd, s, cen(v.x), cen(v.y));
    }
    __syncthreads();
    ntt_row_passes_f64<false, RB>(smd, W, n, logn, md);
    double *dst = Kf + (((g * 2 * k + (size_t)poly * k + j) * CRC_NF64) + m) * (size_t)n;
    for (int s = 2 * threadIdx.x; s < n; s += 2 * blockDim.x) {
        const d2 v = f64_stage_out<false, RB>(sm_load_pair<RB>(smd, s), W, n, logn, s, md);
        *reinterpret_cast<d2 *>(dst + s) = d2{f64_reduce(f64_mulmod_const(v.x, fp.ninv[m], fp.ninv_q[m], md.p), md), f64_reduce(f64_mulmod_const(v.y,
            fp.ninv[m], fp.ninv_q[m], md.p), md)};
    }
}

// ---- K1: digits of c2' under both primes --------------------------------------------------------------------------------------------------------------------
// src: size-`src_size` ciphertexts, poly `src_poly` = c2 (q/q_i)^-1 mod q_i (evaluator.cpp:984-985); E [ct][g][m][n], unreduced (|.| < 14 p) The source row is
// read ONCE and waits in registers (NPT points per thread) through the 2 L_i transforms cut from it: round 3 read it again in front of every transform, 8 times
// at 16-bit digits, and the L2 had long been swept by then (20 row reads per ciphertext for 3 rows at (8192, 3))
template <int RB, int NPT>
__global__ void __launch_bounds__(RB == 5 ? 512 : 1024, 4) relin_digits_f64_kernel(const u64 *src, int src_size, int src_poly, double *E, const double *Wf,
    F64Params fp, int n, int logn,
                                                                                                         int k, int D, int dbc, Relin64Tab tab)
{
    extern __shared__ double smd[];
    const size_t ct = blockIdx.x / k; const int i = blockIdx.x % k;
    const int tid = threadIdx.x, nt = blockDim.x;
    const u64 *row = src + ((ct * src_size + src_poly) * k + i) * (size_t)n;
    const u64 mask = (1ULL << dbc) - 1;
    const int L = tab.L[i], g0 = tab.g0[i];
    u64 r[NPT];
#pragma unroll
    for (int u = 0; u < NPT / 2; u++) {
        const int s = 2 * (tid + u * nt);
        if (s < n) { const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + s); r[2 * u] = v.x; r[2 * u + 1] = v.y; }
    }
    for (int d = 0; d < L; d++) {
        const int sh = d * dbc;
        for (int m = 0; m < CRC_NF64; m++) {
            double *dst = E + ((ct * D + g0 + d) * CRC_NF64 + m) * (size_t)n;
#pragma unroll
            for (int u = 0; u < NPT / 2; u++) {
                const int s = 2 * (tid + u * nt);
                if (s < n) sm_store_pair<RB>(smd, s, (double)(u32)((r[2 * u] >> sh) & mask), (double)(u32)((r[2 * u + 1] >> sh) & mask));
            }
            __syncthreads();
            ntt_row_passes_f64<false, RB>(smd, Wf + (size_t)m * n, n, logn, fp.m[m]);
            f64_drain<false, RB, NPT / 4>(smd, Wf + (size_t)m * n, n, logn, fp.m[m], [&](int s, d2 v) { *reinterpret_cast<d2 *>(dst + s) = v; });
            __syncthreads();
        }
    }
}

// K1 for a Square layer with a sum pooling behind it: one workgroup per (POOLED ciphertext, i).  Sum_w relin(ct_w) = Sum_w c0_w + Sum_g (Sum_w digit_g(c2'_w))
// (*) key_g: the digit polynomials of the window's ciphertexts are added (integers below W 2^dbc) and transformed once -- the same element of Z_q as
// relinearising every ciphertext and adding the results (evaluator.cpp:934-1069 + poolingLayer.cpp:22-44), hence the same bits, with xo yo / (xd yd) of the
// transforms, inner products and inverse transforms.  Up to four digits per residue (16-bit digits of a 55..64-bit modulus), two 32-bit fields per register
// word. ONE: all digit sums of a value in one word -- fields of F = dbc + log2 W bits (the top digit of a 55-bit residue has 7 bits: 3 x 18 + 9 = 63 bits for a
// 2 x 2 window) -- so the window's sums take the registers the unpooled kernel spends on its one source row; otherwise two words of two 32-bit fields each
template <int RB, int NPT, bool ONE>
__global__ void __launch_bounds__(RB == 5 ? 512 : 1024, 4) relin_digits_pool_f64_kernel(const u64 *src, int src_size, int src_poly, double *E,
    const double *Wf, F64Params fp, int n, int logn,
                                                                                                              int k, int D, int dbc, Relin64Tab tab,
                                                                                                                  PoolGeom pg, int F)
{
    extern __shared__ double smd[];
    const size_t o = blockIdx.x / k; const int i = blockIdx.x % k;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t per = (size_t)pg.xo * pg.yo, plane = o / per; const int rem = (int)(o % per), ox = rem / pg.yo, oy = rem % pg.yo;
    const size_t ct0 = (plane * pg.xd + (size_t)ox * pg.xs) * pg.yd + (size_t)oy * pg.ys;
    const u64 mask = (1ULL << dbc) - 1;
    const int L = tab.L[i], g0 = tab.g0[i];
    u64 lo[NPT], hi[ONE ? 2 : NPT];
#pragma unroll
    for (int u = 0; u < NPT; u++) { lo[u] = 0; if (!ONE) hi[u] = 0; }
    // (a fourth field exists only where 3 F < 64: with three digits per residue the host's test bounds (L - 1) F alone, and a shift by 64 or more is undefined)
    const bool four = 3 * F < 64;
    auto spread = [&](u64 v) {
        u64 w = (v & mask) | (((v >> dbc) & mask) << F) | (((v >> (2 * dbc)) & mask) << (2 * F));
        if (four) w |= (v >> (3 * dbc)) << (3 * F);
        return w;
    };
    for (int kx = 0; kx < pg.xf; kx++) for (int ky = 0; ky < pg.yf; ky++) {
        const u64 *row = src + (((ct0 + (size_t)kx * pg.yd + ky) * src_size + src_poly) * k + i) * (size_t)n;
#pragma unroll
        for (int u = 0; u < NPT / 2; u++) {
            const int s = 2 * (tid + u * nt);
            if (s < n) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + s);
                if (ONE) { lo[2 * u] += spread(v.x); lo[2 * u + 1] += spread(v.y); }
                else {
                    lo[2 * u] += (v.x & mask) | (((v.x >> dbc) & mask) << 32);          hi[(2 * u) % (ONE ? 2 :
                        NPT)] += ((v.x >> (2 * dbc)) & mask) | (((v.x >> (3 * dbc)) & mask) << 32);
                    lo[2 * u + 1] += (v.y & mask) | (((v.y >> dbc) & mask) << 32);      hi[(2 * u + 1) % (ONE ? 2 :
                        NPT)] += ((v.y >> (2 * dbc)) & mask) | (((v.y >> (3 * dbc)) & mask) << 32);
                }
            }
        }
    }
    const u64 fmask = (1ULL << F) - 1;
    for (int d = 0; d < L; d++) {
        for (int m = 0; m < CRC_NF64; m++) {
            double *dst = E + ((o * D + g0 + d) * CRC_NF64 + m) * (size_t)n;
#pragma unroll
            for (int u = 0; u < NPT / 2; u++) {
                const int s = 2 * (tid + u * nt);
                if (s < n) {
                    if (ONE) sm_store_pair<RB>(smd, s, (double)(u32)((lo[2 * u] >> (d * F)) & fmask), (double)(u32)((lo[2 * u + 1] >> (d * F)) & fmask));
                    else {
                        const u64 f0 = d < 2 ? lo[2 * u] : hi[(2 * u) % (ONE ? 2 : NPT)], f1 = d < 2 ? lo[2 * u + 1] : hi[(2 * u + 1) % (ONE ? 2 : NPT)];
                        sm_store_pair<RB>(smd, s, (double)(u32)(d & 1 ? f0 >> 32 : f0), (double)(u32)(d & 1 ? f1 >> 32 : f1));
                    }
                }
            }
            __syncthreads();
            ntt_row_passes_f64<false, RB>(smd, Wf + (size_t)m * n, n, logn, fp.m[m]);
            f64_drain<false, RB, NPT / 4>(smd, Wf + (size_t)m * n, n, logn, fp.m[m], [&](int s, d2 v) { *reinterpret_cast<d2 *>(dst + s) = v; });
            __syncthreads();
        }
    }
}

// K1 with ONE workgroup barrier per transform (round 5; ntt_f64.h, wave-local passes): n = 8192 (CS = 3) or 16384 (CS = 4), n / 16 threads.  The source row --
// or the digit sums of a pooling window, all four of a value in one word (relin_digits_pool_f64_kernel<.., ONE>) -- is held in the cross layout, every digit is
// cut straight into the registers the cross pass works on (no fill), and the transformed block leaves through the wave's own drain.  POOL: one workgroup per
// (pooled ciphertext, i); otherwise per (ciphertext, i).
template <int CS, bool POOL>
__global__ void __launch_bounds__(CS == 2 ? 256 : CS == 3 ? 512 : 1024, 4) relin_digits_wave_kernel(const u64 *src, int src_size, int src_poly, double *E, const double *Wf,
    F64Params fp, int n,
                                                                                int k, int D, int dbc, Relin64Tab tab, PoolGeom pg, int F)
{
    extern __shared__ double smd[];
    const size_t o = blockIdx.x / k; const int i = blockIdx.x % k;
    const u64 mask = (1ULL << dbc) - 1;
    const int L = tab.L[i], g0 = tab.g0[i];
    u64 r[16];
    auto load_row = [&](const u64 *row, bool first) {
        if (CS == 2 || CS == 3) {                                   // pairs: 16-byte loads (CS = 2: two pairs per block offset)
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + f64_cross_point<CS == 2 ? 2 : 3>(2 * c));
                if (!POOL) { r[2 * c] = v.x; r[2 * c + 1] = v.y; continue; }
                const bool four = 3 * F < 64;
                auto spread = [&](u64 x) {
                    u64 w = (x & mask) | (((x >> dbc) & mask) << F) | (((x >> (2 * dbc)) & mask) << (2 * F));
                    if (four) w |= (x >> (3 * dbc)) << (3 * F);
                    return w;
                };
                r[2 * c] = (first ? 0 : r[2 * c]) + spread(v.x); r[2 * c + 1] = (first ? 0 : r[2 * c + 1]) + spread(v.y);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const u64 x = row[f64_cross_point<4>(c)];
                if (!POOL) { r[c] = x; continue; }
                const bool four = 3 * F < 64;
                u64 w = (x & mask) | (((x >> dbc) & mask) << F) | (((x >> (2 * dbc)) & mask) << (2 * F));
                if (four) w |= (x >> (3 * dbc)) << (3 * F);
                r[c] = (first ? 0 : r[c]) + w;
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (four loads in flight, not sixteen: the sums already take 32 registers)
            }
        }
    };
    if (POOL) {
        const size_t per = (size_t)pg.xo * pg.yo, plane = o / per; const int rem = (int)(o % per), ox = rem / pg.yo, oy = rem % pg.yo;
        const size_t ct0 = (plane * pg.xd + (size_t)ox * pg.xs) * pg.yd + (size_t)oy * pg.ys;
        for (int kx = 0; kx < pg.xf; kx++) for (int ky = 0; ky < pg.yf; ky++)
            load_row(src + (((ct0 + (size_t)kx * pg.yd + ky) * src_size + src_poly) * k + i) * (size_t)n, kx == 0 && ky == 0);
    } else load_row(src + ((o * src_size + src_poly) * k + i) * (size_t)n, true);
    const int fw = POOL ? F : dbc;                           // width of a digit field in the held words
    const u64 fmask = (1ULL << fw) - 1;
    for (int d = 0; d < L; d++) {
        for (int m = 0; m < CRC_NF64; m++) {
            double *dst = E + ((o * D + g0 + d) * CRC_NF64 + m) * (size_t)n;
            const double *W = Wf + (size_t)m * n;
            f64_wave_forward<CS, 3>(smd, W, n, fp.m[m], [&](int q) { return (double)(u32)((r[q] >> (d * fw)) & fmask); });
            f64_local_drain<3>(smd, W, n, fp.m[m], [&](int s, d2 pr) { *reinterpret_cast<d2 *>(dst + s) = pr; });
            __syncthreads();
        }
    }
}

// ---- K2: slot-wise inner products ---------------------------------------------------------------------------------------------------------------------------
// A[ct][pj][m][s] = sum_g Kf[g][pj][m][s] E[ct][g][m][s]: every product reduced below 0.875 p, the sum of D <= 48 of them stays below 2^53 (exact); CT
// ciphertexts share every key value a thread loads A thread owns one slot of one prime for CT ciphertexts x PJ of the 2k key columns (PJS = 2k / PJ thread
// groups share the E values through L2): per digit CT + PJ loads feed CT PJ products -- the kernel is bound by L2 bandwidth on the key and digit values, not by
// the 7 flops per product
template <int K, int CT, int PJ>
__global__ void __launch_bounds__(256, CT * PJ <= 36 ? 4 : 1) relin_mac_f64_kernel(const double *E, const double *Kf, double *A, F64Params fp, int n, int D,
    size_t cnt)
{
    constexpr int PJS = 2 * K / PJ;
    const int sblocks = n / blockDim.x;
    // ciphertext group fastest: the workgroups that are resident together work on the SAME key tile (D x PJ values for 256 slots, 0.1-0.5 MiB: one L2 fill per
    // XCD) and stream only their own digit values -- with the slot block fastest every ciphertext group pulled the whole key set (9-17 MB, more than an L2)
    // again
    const unsigned groups = (unsigned)((cnt + CT - 1) / CT);
    unsigned b = blockIdx.x;
    const size_t ct0 = (size_t)(b % groups) * CT; b /= groups;
    const int s = (b % sblocks) * blockDim.x + threadIdx.x; b /= sblocks;
    const int pj0 = (b % PJS) * PJ; b /= PJS;
    const int m = b % CRC_NF64;
    const F64Mod md = fp.m[m];
    double acc[CT][PJ];
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int pj = 0; pj < PJ; pj++) acc[c][pj] = 0.0;
    const size_t nn = (size_t)n;
    // (round 5) the digit values of g + 1 -- the operand that comes from HBM; the key tile is L2-resident -- are requested before the CT x PJ products of digit
    // g are formed: the kernel waits on memory half of its time (profiles/r05_pmc_square_pool_8192_issue.json) and every iteration started with an exposed
    // round trip
    constexpr bool AHEAD = CT * PJ <= 36;                 // (the wider tiles have no registers to spare)
    double e[CT];
    auto fetch = [&](int g, double (&ev)[CT]) {
#pragma unroll
        for (int c = 0; c < CT; c++) ev[c] = ct0 + c < cnt ? E[(((ct0 + c) * D + g) * CRC_NF64 + m) * nn + s] : 0.0;
    };
    fetch(0, e);
    for (int g = 0; g < D; g++) {
        double en[CT];
        if (AHEAD && g + 1 < D) fetch(g + 1, en);
        const double *kr = Kf + (((size_t)g * 2 * K + pj0) * CRC_NF64 + m) * nn + s;
#pragma unroll
        for (int pj = 0; pj < PJ; pj++) {
            const double kv = kr[(size_t)pj * CRC_NF64 * nn];
#pragma unroll
            for (int c = 0; c < CT; c++) acc[c][pj] += f64_mulmod(kv, e[c], md);
        }
        if (g + 1 < D) {
            if (!AHEAD) fetch(g + 1, en);
#pragma unroll
            for (int c = 0; c < CT; c++) e[c] = en[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CT; c++)
        if (ct0 + c < cnt)
#pragma unroll
            for (int pj = 0; pj < PJ; pj++) A[(((ct0 + c) * 2 * K + pj0 + pj) * CRC_NF64 + m) * nn + s] = acc[c][pj];
}

// K2 for RT keys at once (the hoisted rotations: several keys are applied to the digits of ONE ciphertext): the products of RT key tiles per digit value
// loaded, so a call over R keys streams E from HBM R / RT times instead of R times.  The tile is CT x PJ x RT sums, kept within the 36 doubles the look-ahead
// path of the kernel above affords (CT shrinks as RT grows: the key tiles, RT of them now, still come from L2).  Every sum adds the same reduced products in
// the same order as the kernel above: the same doubles.  A of key r: A + r a_stride
struct RelinMultiKeys { const double *kf[2]; };
template <int K, int CT, int PJ, int RT>
__global__ void __launch_bounds__(256, 4) relin_mac_multi_f64_kernel(const double *E, RelinMultiKeys keys, double *A, size_t a_stride, F64Params fp, int n, int D,
    size_t cnt)
{
    static_assert(CT * PJ * RT <= 36 && RT <= 2, "the tile must fit the look-ahead path's register budget");
    constexpr int PJS = 2 * K / PJ;
    const int sblocks = n / blockDim.x;
    const unsigned groups = (unsigned)((cnt + CT - 1) / CT);            // ciphertext group fastest, as above: resident workgroups share their key tiles
    unsigned b = blockIdx.x;
    const size_t ct0 = (size_t)(b % groups) * CT; b /= groups;
    const int s = (b % sblocks) * blockDim.x + threadIdx.x; b /= sblocks;
    const int pj0 = (b % PJS) * PJ; b /= PJS;
    const int m = b % CRC_NF64;
    const F64Mod md = fp.m[m];
    double acc[RT][CT][PJ];
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
        for (int c = 0; c < CT; c++)
#pragma unroll
            for (int pj = 0; pj < PJ; pj++) acc[r][c][pj] = 0.0;
    const size_t nn = (size_t)n;
    double e[CT];
    auto fetch = [&](int g, double (&ev)[CT]) {
#pragma unroll
        for (int c = 0; c < CT; c++) ev[c] = ct0 + c < cnt ? E[(((ct0 + c) * D + g) * CRC_NF64 + m) * nn + s] : 0.0;
    };
    fetch(0, e);
    for (int g = 0; g < D; g++) {
        double en[CT];
        if (g + 1 < D) fetch(g + 1, en);
        const size_t ko = (((size_t)g * 2 * K + pj0) * CRC_NF64 + m) * nn + s;
#pragma unroll
        for (int r = 0; r < RT; r++)
#pragma unroll
            for (int pj = 0; pj < PJ; pj++) {
                const double kv = keys.kf[r][ko + (size_t)pj * CRC_NF64 * nn];
#pragma unroll
                for (int c = 0; c < CT; c++) acc[r][c][pj] += f64_mulmod(kv, e[c], md);
            }
        if (g + 1 < D) {
#pragma unroll
            for (int c = 0; c < CT; c++) e[c] = en[c];
        }
    }
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
        for (int c = 0; c < CT; c++)
            if (ct0 + c < cnt)
#pragma unroll
                for (int pj = 0; pj < PJ; pj++) A[r * a_stride + (((ct0 + c) * 2 * K + pj0 + pj) * CRC_NF64 + m) * nn + s] = acc[r][c][pj];
}

// K2 with ONE KEY PER STEP of the batch (the dense layer over channel planes rotates its outputs: R inner sums, each switched under its own key, in one launch):
// the batch is [steps][per] ciphertexts, ciphertext i = j per + ct takes the prepared key keys[j] -- a table of pointers in device memory, R runs into the hundreds.
//     A[i][pj][m][s] = Sum_g Kf_{keys[j]}[g][pj][m][s] E[i][g][m][s],  g ascending, every product f64_mulmod: relin_mac_f64_kernel's sums, the same doubles.
// CT ciphertexts OF ONE STEP share every key value a thread loads; a ciphertext index past the step's `per` loads nothing and stores nothing.  At per = 1 nothing
// is shared at all and the kernel is a stream of key values from HBM, every one used once: CT = 1, and SV = 2 slots per thread (16-byte loads; n >= 512).  The digit
// values of g + 1 are requested before the products of digit g are formed, as above.
// Index order: the ciphertext groups of a step fastest, so that the workgroups resident together and working on one key read the SAME key tile (D x PJ values
// for 256 SV slots) and each tile comes from HBM once; the step slowest, so that at most a few keys are being read at any time and no key is touched again once its
// workgroups have gone -- every prepared key is streamed exactly once
template <int SV> struct f64_vec { double v[SV]; };
template <int SV> __device__ __forceinline__ f64_vec<SV> f64_vec_load(const double *p)
{
    f64_vec<SV> r;
    if constexpr (SV == 2) { const d2 t = *reinterpret_cast<const d2 *>(p); r.v[0] = t.x; r.v[1] = t.y; }
    else r.v[0] = *p;
    return r;
}
template <int K, int CT, int PJ, int SV>
__global__ void __launch_bounds__(256, 4) relin_mac_keyed_f64_kernel(const double *E, const double *const *keys, double *A, F64Params fp, int n, int D,
    unsigned steps, unsigned per)
{
    static_assert(CT * PJ * SV <= 36 && (SV == 1 || SV == 2), "the tile must fit the look-ahead path's register budget");
    constexpr int PJS = 2 * K / PJ;
    const int sblocks = n / ((int)blockDim.x * SV);
    const unsigned groups = (per + CT - 1) / CT;
    unsigned b = blockIdx.x;
    const unsigned ct0 = (b % groups) * CT; b /= groups;
    const int s = ((b % sblocks) * blockDim.x + threadIdx.x) * SV; b /= sblocks;
    const int pj0 = (b % PJS) * PJ; b /= PJS;
    const int m = b % CRC_NF64; b /= CRC_NF64;
    const unsigned j = b;                                                 // the step: uniform over the workgroup, so is its key pointer
    if (j >= steps) return;
    const double *Kf = keys[j];
    const size_t i0 = (size_t)j * per + ct0;                              // first ciphertext of the tile in the batch
    const F64Mod md = fp.m[m];
    double acc[CT][PJ][SV];
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int pj = 0; pj < PJ; pj++)
#pragma unroll
            for (int v = 0; v < SV; v++) acc[c][pj][v] = 0.0;
    const size_t nn = (size_t)n;
    f64_vec<SV> e[CT];
    auto fetch = [&](int g, f64_vec<SV> (&ev)[CT]) {
#pragma unroll
        for (int c = 0; c < CT; c++) {
            if (ct0 + c < per) ev[c] = f64_vec_load<SV>(E + (((i0 + c) * D + g) * CRC_NF64 + m) * nn + s);
            else
#pragma unroll
                for (int v = 0; v < SV; v++) ev[c].v[v] = 0.0;
        }
    };
    fetch(0, e);
    for (int g = 0; g < D; g++) {
        f64_vec<SV> en[CT];
        if (g + 1 < D) fetch(g + 1, en);
        const double *kr = Kf + (((size_t)g * 2 * K + pj0) * CRC_NF64 + m) * nn + s;
#pragma unroll
        for (int pj = 0; pj < PJ; pj++) {
            const f64_vec<SV> kv = f64_vec_load<SV>(kr + (size_t)pj * CRC_NF64 * nn);
#pragma unroll
            for (int c = 0; c < CT; c++)
#pragma unroll
                for (int v = 0; v < SV; v++) acc[c][pj][v] += f64_mulmod(kv.v[v], e[c].v[v], md);
        }
        if (g + 1 < D) {
#pragma unroll
            for (int c = 0; c < CT; c++) e[c] = en[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CT; c++)
        if (ct0 + c < per)
#pragma unroll
            for (int pj = 0; pj < PJ; pj++) {
                double *dst = A + (((i0 + c) * 2 * K + pj0 + pj) * CRC_NF64 + m) * nn + s;
                if constexpr (SV == 2) *reinterpret_cast<d2 *>(dst) = d2{acc[c][pj][0], acc[c][pj][1]};
                else *dst = acc[c][pj][0];
            }
}

// ---- K3: inverse transforms, CRT lift, mod q_j, + (c0, c1) --------------------------------------------------------------------------------------------------
// A [ct][poly k + j][m][n]; x3: size-`add_size` ciphertexts whose polys 0, 1 are added (coefficient form); y [ct][2][k][n].  The first prime's result waits in
// registers (NPT points per thread, reduced) while the image serves the second transform -- round 3 parked it in its own row of A (6 rows written and read back
// per ciphertext at (8192, 3), and 11 spilled registers: the twiddle companions took the room) Workgroups of n / 16 threads, 16 points each: at n = 8192 two
// 512-thread workgroups per CU, four waves per SIMD and 128 registers -- with 1024 threads and 8 points the 64-register line of the second workgroup left no
// room for the held row (18 spilled registers, 16.6 instead of 12.2 MB of traffic per ciphertext and 5.55 instead of 5.19 us at (8192, 3):
// profiles/r04_square_relin_ab_step1.txt)
// POLY (OUT_NTT only): the ring-linear terms of a degree-2 polynomial activation join the result while it leaves (crc_poly2_*_relin_forms):
//     y = mul (*) y + pt.p1 (*) Sum_w xh_w (+ pt.p0 on poly 0),   xh = the activation's NTT-form input (size-2 ciphertexts, laid out as x3's),
// NULL rows = 1 / 0 / 0.  A compile-time variant of relin_inv_crt_kernel: the kernel takes the PolyTail as a trailing parameter PACK (TAIL = PolyTail or
// nothing), so the instantiations without it keep their parameter list, their kernel-argument offsets and with them every instruction they had
template <typename T> __device__ __forceinline__ const T &first_of(const T &t) { return t; }
__device__ __forceinline__ void poly_tail_pair(ulonglong2 &v, int s, const u64 *mul, const PolyTail &pt, size_t actw, int poly, int j, int n, int k, const PoolGeom &pg,
                                               const ModParams &mq)
{
    const size_t row = (size_t)j * n + s;
    if (mul) { const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(mul + row); v.x = mulmod(v.x, w.x, mq); v.y = mulmod(v.y, w.y, mq); }
    if (pt.p1) {
        const size_t cw = 2 * (size_t)k * n;
        const u64 *xrow = pt.xh + actw * cw + (size_t)poly * k * n + row;
        const int xf = pg.xf > 0 ? pg.xf : 1, yf = pg.xf > 0 ? pg.yf : 1;
        ulonglong2 acc = make_ulonglong2(0, 0);
        for (int kx = 0; kx < xf; kx++, xrow += (size_t)pg.yd * cw)
            for (int ky = 0; ky < yf; ky++) {
                const ulonglong2 xv = *reinterpret_cast<const ulonglong2 *>(xrow + (size_t)ky * cw);
                acc.x = addmod(acc.x, xv.x, mq.q); acc.y = addmod(acc.y, xv.y, mq.q);
            }
        const ulonglong2 w1 = *reinterpret_cast<const ulonglong2 *>(pt.p1 + row);
        v.x = addmod(v.x, mulmod(acc.x, w1.x, mq), mq.q); v.y = addmod(v.y, mulmod(acc.y, w1.y, mq), mq.q);
    }
    if (pt.p0 && poly == 0) { const ulonglong2 w0 = *reinterpret_cast<const ulonglong2 *>(pt.p0 + row); v.x = addmod(v.x, w0.x, mq.q); v.y = addmod(v.y, w0.y, mq.q); }
}
template <int RB, int NPT, bool OUT_NTT, bool LAZY, typename... TAIL>
__global__ void __launch_bounds__(RB == 5 ? 512 : 1024, 4) relin_inv_crt_kernel(const double *A, const u64 *x3, int add_size, u64 *y, const ModParams *mods,
    const double *Wi,
                                                                                                                     const ulonglong2 *Wq, F64Params fp,
                                                                                                                         int n, int logn, int k,
                                                                                                                         const u64 *mul, PoolGeom pg,
                                                                                                                         TAIL... tail)
{
    constexpr bool POLY = sizeof...(TAIL) != 0;
    static_assert(!POLY || OUT_NTT, "the polynomial tail multiplies slot-wise");
    extern __shared__ double smd[];
    const size_t ct = blockIdx.x / (2 * k); const int pj = blockIdx.x % (2 * k), poly = pj / k, j = pj % k;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double *a0row = A + ((ct * 2 * k + pj) * CRC_NF64) * (size_t)n;
    double a0[NPT];
    for (int m = 0; m < CRC_NF64; m++) {
        const double *src = a0row + (size_t)m * n;
        f64_fill_inv<RB, NPT / 2>(smd, Wi + (size_t)m * n, n, logn, fp.m[m], [&](int s) { return *reinterpret_cast<const d2 *>(src + s); });
        __syncthreads();
        // (A holds lazy sums below 2^52.4: the fused first stage reduces them while it fills the image, otherwise the first pass does)
        ntt_row_passes_f64<true, RB>(smd, Wi + (size_t)m * n, n, logn, fp.m[m], !f64_fused_stage<RB>(logn));
        if (m == 0) {
#pragma unroll
            for (int u = 0; u < NPT / 2; u++) {
                const int s = 2 * (tid + u * nt);
                if (s < n) { const d2 v = sm_load_pair<RB>(smd, s); a0[2 * u] = f64_reduce(v.x, fp.m[0]); a0[2 * u + 1] = f64_reduce(v.y, fp.m[0]); }
            }
            __syncthreads();
        }
    }
    // x = a0 + p0 t,  t = (a1 - a0) p0^-1 mod p1 centred: |x| < p0 p1 / 2, and the true value is below a quarter of that, so t is nowhere near +- p1 / 2
    const ModParams mq = mods[j];
    const u64 q = mq.q, p0q = fp.p0_mod_q[j];
    // pooled key switch (pg.xf > 0): `ct` counts pooled ciphertexts and the (c0, c1) of the window's ciphertexts in x3 are added up here -- no pooling pass, no
    // pooled copy
    size_t actw = ct;
    if (pg.xf > 0) {
        const size_t per = (size_t)pg.xo * pg.yo, plane = ct / per; const int rem = (int)(ct % per), ox = rem / pg.yo, oy = rem % pg.yo;
        actw = (plane * pg.xd + (size_t)ox * pg.xs) * pg.yd + (size_t)oy * pg.ys;
    }
    const u64 *add = x3 + ((actw * add_size + poly) * k + j) * (size_t)n;
    u64 *dst = y + ((ct * 2 + poly) * k + j) * (size_t)n;
    u64 *sm = reinterpret_cast<u64 *>(smd);           // (a thread reads and rewrites only its own slot of the image here: no barrier in between)
    auto lift = [&](double a0v, double a1r, u64 addv) {
        const double a1 = f64_reduce(a1r, fp.m[1]);
        const double t = f64_reduce(f64_mulmod_const(a1 - a0v, fp.inv_p0_p1, fp.inv_p0_p1_q, fp.m[1].p), fp.m[1]);
        const long long ti = (long long)t, a0i = (long long)a0v;
        u64 lo, hi; mul64wide((u64)(ti < 0 ? -ti : ti), p0q, lo, hi);
        u64 r = barrett128(lo, hi, mq);
        if (ti < 0) r = negmod(r, q);
        u64 a0m = (u64)(a0i < 0 ? -a0i : a0i);                    // |a0| < 2^46: below q for the 54..60-bit coefficient moduli, not for SEAL's 40-bit ones
        if (a0m >= q) a0m = barrett128(a0m, 0, mq);
        r = addmod(r, a0i < 0 ? negmod(a0m, q) : a0m, q);
        return addmod(r, addv, q);
    };
#pragma unroll
    for (int u = 0; u < NPT / 2; u++) {
        const int s = 2 * (tid + u * nt);
        if (s < n) {
            const d2 a1 = sm_load_pair<RB>(smd, s);
            ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(add + s);
            if (pg.xf > 0) {
                for (int w = 1; w < pg.xf * pg.yf; w++) {
                    const int kx = w / pg.yf, ky = w - kx * pg.yf;
                    const ulonglong2 bv = *reinterpret_cast<const ulonglong2 *>(add + ((size_t)kx * pg.yd + ky) * add_size * k * n + s);
                    av.x = addmod(av.x, bv.x, q); av.y = addmod(av.y, bv.y, q);
                }
            }
            const u64 r0 = lift(a0[2 * u], a1.x, av.x), r1 = lift(a0[2 * u + 1], a1.y, av.y);
            if (OUT_NTT) {
                const int a = swz<RB>(s);
                *reinterpret_cast<ulonglong2 *>(sm + (a & ~1)) = (a & 1) ? ulonglong2{r1, r0} : ulonglong2{r0, r1};
            } else *reinterpret_cast<ulonglong2 *>(dst + s) = ulonglong2{r0, r1};
        }
    }
    if (!OUT_NTT) return;
    // NTT-resident result: forward transform over q_j of (c_poly + R) in the same LDS image, same layout (ntt_device.h's radix-8 passes on the fp64 image's
    // swizzle)
    __syncthreads();
    ntt_row_passes<false, LAZY, RB, true>(sm, Wq + (size_t)j * n, n, logn, q, mq.two_q);
    const float rq = 1.0f / (float)((u32)(q >> 32) + 1);
    // (the gap-1 stage of the forward transform is applied here, while the image is drained: ntt_device.h)
    const bool fuse1 = ntt_fused_stage(logn);
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const int a = swz<RB>(s);
        ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(sm + (a & ~1));
        if (a & 1) { const u64 t = v.x; v.x = v.y; v.y = t; }
        if (fuse1) fwd_pair_stage<LAZY>(v, Wq[(size_t)j * n + (n >> 1) + (s >> 1)], q, mq.two_q);
        if (LAZY) { v.x = reduce_small(v.x, q, mq.two_q, rq); v.y = reduce_small(v.y, q, mq.two_q, rq); }
        else { v.x = v.x >= mq.two_q ? v.x - mq.two_q : v.x; v.x = v.x >= q ? v.x - q : v.x; v.y = v.y >= mq.two_q ? v.y - mq.two_q : v.y;
            v.y = v.y >= q ? v.y - q : v.y; }
        if constexpr (POLY)
            poly_tail_pair(v, s, mul, first_of(tail...), actw, poly, j, n, k, pg, mq);
        else if (mul) {     // the divisor of an average pooling behind the Square layer (an NTT-form plaintext [k][n]): slot-wise, while the result leaves
            const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(mul + (size_t)j * n + s);
            v.x = mulmod(v.x, w.x, mq); v.y = mulmod(v.y, w.y, mq);
        }
        *reinterpret_cast<ulonglong2 *>(dst + s) = v;
    }
}

// K3 with ONE workgroup barrier per transform (round 5; ntt_f64.h, wave-local passes): n = 8192 (CS = 3) or 16384 (CS = 4), n / 16 threads.  Both inverse
// transforms end in the cross pass, i.e. in registers: the first prime's result simply stays there (no LDS read, no parking), the second meets it for the CRT
// lift, the (c0, c1) rows are read in the same cross layout, and the canonical sums go into the image for the forward transform over q_j (or straight to
// memory). U64W: the forward transform over q_j that follows the CRT runs wave-locally too -- its cross pass works on the CRT's results where they are made, in
// registers
template <int CS, bool OUT_NTT, bool LAZY, bool U64W>
__global__ void __launch_bounds__(CS == 2 ? 256 : CS == 3 ? 512 : 1024, 4) relin_inv_crt_wave_kernel(const double *A, const u64 *x3, int add_size, u64 *y,
    const ModParams *mods, const double *Wi,
                                                                                 const ulonglong2 *Wq, F64Params fp, int n, int logn, int k, const u64 *mul,
                                                                                     PoolGeom pg)
{
    extern __shared__ double smd[];
    const size_t ct = blockIdx.x / (2 * k); const int pj = blockIdx.x % (2 * k), poly = pj / k, j = pj % k;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double *a0row = A + ((ct * 2 * k + pj) * CRC_NF64) * (size_t)n;
    // (two explicit blocks, not a loop over the primes: a loop keeps BOTH result arrays alive through both transforms)
    double a0[16];
    {
        // (A holds lazy sums below 2^52.4: the fill reduces them)
        f64_local_fill<3>(smd, Wi, n, fp.m[0], [&](int, int s) { return *reinterpret_cast<const d2 *>(a0row + s); });
        f64_wave_inverse<CS, 3>(smd, Wi, n, fp.m[0], [&](int q, double x) { a0[q] = f64_reduce(x, fp.m[0]); });
        __syncthreads();                                      // the image is filled again
    }
    double a1[16];
    {
        const double *src = a0row + n, *W = Wi + n;
        f64_local_fill<3>(smd, W, n, fp.m[1], [&](int, int s) { return *reinterpret_cast<const d2 *>(src + s); });
        f64_wave_inverse<CS, 3>(smd, W, n, fp.m[1], [&](int q, double x) { a1[q] = x; });
    }
    const ModParams mq = mods[j];
    const u64 q = mq.q, p0q = fp.p0_mod_q[j];
    size_t actw = ct;
    if (pg.xf > 0) {
        const size_t per = (size_t)pg.xo * pg.yo, plane = ct / per; const int rem = (int)(ct % per), ox = rem / pg.yo, oy = rem % pg.yo;
        actw = (plane * pg.xd + (size_t)ox * pg.xs) * pg.yd + (size_t)oy * pg.ys;
    }
    const u64 *add = x3 + ((actw * add_size + poly) * k + j) * (size_t)n;
    u64 *dst = y + ((ct * 2 + poly) * k + j) * (size_t)n;
    // x = a0 + p0 t,  t = (a1 - a0) p0^-1 mod p1 centred (relin_inv_crt_kernel)
    auto lift = [&](double a0v, double a1r, u64 addv) {
        const double a1v = f64_reduce(a1r, fp.m[1]);
        const double t = f64_reduce(f64_mulmod_const(a1v - a0v, fp.inv_p0_p1, fp.inv_p0_p1_q, fp.m[1].p), fp.m[1]);
        const long long ti = (long long)t, a0i = (long long)a0v;
        u64 lo, hi; mul64wide((u64)(ti < 0 ? -ti : ti), p0q, lo, hi);
        u64 r = barrett128(lo, hi, mq);
        if (ti < 0) r = negmod(r, q);
        u64 a0m = (u64)(a0i < 0 ? -a0i : a0i);
        if (a0m >= q) a0m = barrett128(a0m, 0, mq);
        r = addmod(r, a0i < 0 ? negmod(a0m, q) : a0m, q);
        return addmod(r, addv, q);
    };
    const int nw = pg.xf > 0 ? pg.xf * pg.yf : 1;
    u64 *sm = reinterpret_cast<u64 *>(smd);
    if (OUT_NTT) __syncthreads();                             // every wave has read its part of the image in the cross pass: the canonical sums go into it now
    if constexpr (CS == 2 || CS == 3) {                        // pairs (CS = 2: two per block offset; the cross layout's registers 2 c, 2 c + 1 are neighbours either way)
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int s = f64_cross_point<CS == 2 ? 2 : 3>(2 * c);
            ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(add + s);
            for (int w = 1; w < nw; w++) {
                const int kx = w / pg.yf, ky = w - kx * pg.yf;
                const ulonglong2 bv = *reinterpret_cast<const ulonglong2 *>(add + ((size_t)kx * pg.yd + ky) * add_size * k * n + s);
                av.x = addmod(av.x, bv.x, q); av.y = addmod(av.y, bv.y, q);
            }
            const u64 r0 = lift(a0[2 * c], a1[2 * c], av.x), r1 = lift(a0[2 * c + 1], a1[2 * c + 1], av.y);
            if (OUT_NTT) {
                const int a = swz<3>(s);
                *reinterpret_cast<ulonglong2 *>(sm + (a & ~1)) = (a & 1) ? ulonglong2{r1, r0} : ulonglong2{r0, r1};
            } else *reinterpret_cast<ulonglong2 *>(dst + s) = ulonglong2{r0, r1};
        }
    } else {
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int s = f64_cross_point<4>(c);
            u64 av = add[s];
            for (int w = 1; w < nw; w++) { const int kx = w / pg.yf, ky = w - kx * pg.yf; av = addmod(av, add[((size_t)kx * pg.yd + ky) * add_size * k * n +
                s], q); }
            const u64 r0 = lift(a0[c], a1[c], av);
            if (OUT_NTT) sm[swz<3>(s)] = r0; else dst[s] = r0;
        }
    }
    if (!OUT_NTT) return;
    const float rq = 1.0f / (float)((u32)(q >> 32) + 1);
    if constexpr (U64W) {
        // the forward transform wave-locally too.  The points a thread has just written are the cross groups it owns (two of eight at n = 8192, one of sixteen
        // at 16384): the cross stages read them back in program order -- no barrier --, one barrier later every wave finishes its own block.  (Round 5, first
        // form: the cross stages on the lifts' results in registers -- with both held transforms still alive that spilled 190-400 bytes per lane and lost 4 %.)
        const ulonglong2 *W = Wq + (size_t)j * n;
        constexpr int E = 16 >> CS, C = 1 << CS;
        // (nothing of the transform is scheduled into the lifts above: they fill the register file as it is)
        __builtin_amdgcn_sched_barrier(0);
        int t2 = tid;
        // (... nor are the sixteen image addresses of the lifts kept alive for it: they are computed again)
        asm volatile("" : "+v"(t2));
        auto own = [&](int c, int e) { return swz<3>(CS == 2 ? 4 * t2 + e + CRC_F64_BLOCK * c : CS == 3 ? 2 * t2 + e + CRC_F64_BLOCK * c : t2 + CRC_F64_BLOCK * c); };
#pragma unroll
        for (int e = 0; e < E; e++) {
            u64 x[C];
#pragma unroll
            for (int c = 0; c < C; c++) x[c] = sm[own(c, e)];
            fwd_stages<CS, LAZY>(x, W, 1, 0, q, mq.two_q);
#pragma unroll
            for (int c = 0; c < C; c++) sm[own(c, e)] = x[c];
        }
        __syncthreads();
        u64_local_passes_fwd<LAZY>(sm, W, n, q, mq.two_q);
#pragma unroll 2
        for (int u = 0; u < 8; u++) {                         // block-local drain through the gap-1 stage
            const int s = f64_local_pair(u), a = swz<3>(s);
            ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(sm + (a & ~1));
            if (a & 1) { const u64 t = v.x; v.x = v.y; v.y = t; }
            fwd_pair_stage<LAZY>(v, W[(n >> 1) + (s >> 1)], q, mq.two_q);
            if (LAZY) { v.x = reduce_small(v.x, q, mq.two_q, rq); v.y = reduce_small(v.y, q, mq.two_q, rq); }
            else {
                v.x = v.x >= mq.two_q ? v.x - mq.two_q : v.x; v.x = v.x >= q ? v.x - q : v.x;
                v.y = v.y >= mq.two_q ? v.y - mq.two_q : v.y; v.y = v.y >= q ? v.y - q : v.y;
            }
            if (mul) {
                const ulonglong2 wv = *reinterpret_cast<const ulonglong2 *>(mul + (size_t)j * n + s);
                v.x = mulmod(v.x, wv.x, mq); v.y = mulmod(v.y, wv.y, mq);
            }
            *reinterpret_cast<ulonglong2 *>(dst + s) = v;
        }
        return;
    }
    // NTT-resident result: forward transform over q_j of (c_poly + R) in the same LDS image (as relin_inv_crt_kernel)
    __syncthreads();
    ntt_row_passes<false, LAZY, 3, true>(sm, Wq + (size_t)j * n, n, logn, q, mq.two_q);
    const bool fuse1 = ntt_fused_stage(logn);
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const int a = swz<3>(s);
        ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(sm + (a & ~1));
        if (a & 1) { const u64 t = v.x; v.x = v.y; v.y = t; }
        if (fuse1) fwd_pair_stage<LAZY>(v, Wq[(size_t)j * n + (n >> 1) + (s >> 1)], q, mq.two_q);
        if (LAZY) { v.x = reduce_small(v.x, q, mq.two_q, rq); v.y = reduce_small(v.y, q, mq.two_q, rq); }
        else {
            v.x = v.x >= mq.two_q ? v.x - mq.two_q : v.x; v.x = v.x >= q ? v.x - q : v.x;
            v.y = v.y >= mq.two_q ? v.y - mq.two_q : v.y; v.y = v.y >= q ? v.y - q : v.y;
        }
        if (mul) {
            const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(mul + (size_t)j * n + s);
            v.x = mulmod(v.x, w.x, mq); v.y = mulmod(v.y, w.y, mq);
        }
        *reinterpret_cast<ulonglong2 *>(dst + s) = v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------------
// can this context / key set take the fp64 path?  2 |R_j| <= n D 2^dbc q_max must stay below p_0 p_1 / 2 (a factor 2 of slack for the floating CRT), the row
// must fit the LDS image the transforms work on, and at most 48 products may be summed lazily
static int relin64_qbits(const crc_ctx *c) { int b = 0; for (int i = 0; i < c->k; i++) if ((int)c->tabs[i].m.bits > b) b = c->tabs[i].m.bits; return b; }
bool k_relin64_supported(const crc_ctx *c, int dbc)
{
    if (c->n < 64 || c->n > 16384 || dbc < 1 || dbc > 32) return false;
    const int D = relin_digit_count(c, dbc), qbits = relin64_qbits(c);
    if (D > 48) return false;
    int dbits = 0; while ((1 << dbits) < D) dbits++;
    // log2(n D 2^dbc q_max) <= logn + dbits + dbc + qbits  must be <= 2 * 47 - 2 (p_m > 2^46.99)
    return c->logn + dbits + dbc + qbits <= 2 * CRC_F64_PRIME_BITS - 3;
}
// the pooled form: the integer inner products are `window` times larger, a residue has at most four digits (two 32-bit fields per word hold their sums)
bool k_relin64_pool_supported(const crc_ctx *c, int dbc, int window)
{
    if (!k_relin64_supported(c, dbc) || window < 1 || window > 64 || dbc > 20) return false;
    for (int i = 0; i < c->k; i++) if (evk_digits(c->q[i], dbc) > 4) return false;
    const int D = relin_digit_count(c, dbc), qbits = relin64_qbits(c);
    int dbits = 0; while ((1 << dbits) < D) dbits++;
    int wbits = 0; while ((1 << wbits) < window) wbits++;
    // 2 |R| <= n D W 2^dbc q_max <= 2^92 leaves |R| <= 2^91 < p_0 p_1 / 2 / 3.9: the CRT's t = (a1 - a0) p_0^-1 mod p_1 stays below p_1 / 3.9 in magnitude,
    // well inside the centred range it is reduced to (the unpooled test keeps one bit more; this one admits n = 16384 with all eight primes, D = 32, W = 4)
    return c->logn + dbits + wbits + dbc + qbits <= 2 * CRC_F64_PRIME_BITS - 2;
}
size_t k_relin64_keys_words(const crc_ctx *c, int dbc) { return (size_t)CRC_NF64 * crc_evk_words(c, dbc); }
// The work space of K1 to K3 for cnt ciphertexts, in words from its start: the D digit polynomials E [cnt][D][2][n], behind them the inner products
// A [cnt][2k][2][n] of one key, and one more A, a_stride further, per further key applied to the same E.  Filled on the caller's work space it gives the
// pointers, on a null base it only counts
struct Relin64Work { int D; double *E, *A; size_t a_stride, words; };
static Relin64Work relin64_work(const crc_ctx *c, size_t cnt, int dbc, u64 *work = nullptr)
{
    Relin64Work w{};
    w.D = relin_digit_count(c, dbc);
    const size_t e = cnt * w.D * CRC_NF64 * c->n;
    w.a_stride = cnt * 2 * c->k * CRC_NF64 * c->n;
    w.E = reinterpret_cast<double *>(work); w.A = work ? w.E + e : nullptr;
    w.words = e + w.a_stride;
    return w;
}
// scratch words: PM [cnt][k][n] in front of relin64_work where the caller's c2 is not premultiplied (k_relinearize); the key preparation borrows the same space
size_t k_relin64_work_words(const crc_ctx *c, size_t cnt, int dbc)
{
    const size_t run = cnt * c->n * c->k + relin64_work(c, cnt, dbc).words, prep = crc_evk_words(c, dbc);
    return run > prep ? run : prep;
}

// kp: k_relin64_keys_words; scratch: crc_evk_words (k_relin64_work_words covers it)
int k_relin64_prepare_keys(crc_ctx *c, const u64 *evk, int dbc, u64 *kp, u64 *scratch, hipStream_t st)
{
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    double *Kf = reinterpret_cast<double *>(kp);
    const size_t rows = crc_evk_words(c, dbc) / c->n;                 // (2 g + poly) k + j
    hipLaunchKernelGGL(evk_canon_kernel, dim3((unsigned)rows), dim3(256), 0, st, evk, scratch, c->d_mods, c->n, c->k);
    HIPCHK(hipGetLastError());
    int rc;
    if ((rc = k_ntt_ct(c, true, scratch, scratch, rows / c->k, 1, false, st, nullptr, 0, 0, 0))) return rc;
    const int RB = f64_radix(c);
    return f64_launch(c, RB == 3 ? relin_keys_f64_kernel<3> : RB == 4 ? relin_keys_f64_kernel<4> : relin_keys_f64_kernel<5>, rows * CRC_NF64, f64_threads(c, RB), st,
                      scratch, Kf, c->d_mods, c->d_f64_rp, c->f64, c->n, c->logn, c->k);
}

template <int K, int BIGCT = 4>
static int relin64_mac(crc_ctx *c, const double *E, const double *Kf, double *A, int D, size_t cnt, hipStream_t st)
{
    // accumulators: CT x PJ doubles per thread (32..48)
    constexpr int PJ = 2 * K <= 8 ? 2 * K : (2 * K) % 8 == 0 ? 8 : (2 * K) % 6 == 0 ? 6 : (2 * K) % 5 == 0 ? 5 : 7, CT = PJ <= 4 ? 8 : PJ <= 6 ? 6 : BIGCT,
        PJS = 2 * K / PJ;
    static_assert(PJ * PJS == 2 * K, "key columns must split evenly");
    const int threads = c->n < 256 ? c->n : 256, sblocks = c->n / threads;
    const size_t groups = (cnt + CT - 1) / CT;
    hipLaunchKernelGGL((relin_mac_f64_kernel<K, CT, PJ>), dim3((unsigned)(groups * CRC_NF64 * PJS * sblocks)), dim3(threads), 0, st, E, Kf, A, c->f64, c->n,
        D, cnt);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}

template <int K>
static int relin64_mac2(crc_ctx *c, const double *E, const double *Kf0, const double *Kf1, double *A, size_t a_stride, int D, size_t cnt, hipStream_t st)
{
    constexpr int PJ = 2 * K <= 8 ? 2 * K : (2 * K) % 8 == 0 ? 8 : (2 * K) % 6 == 0 ? 6 : (2 * K) % 5 == 0 ? 5 : 7, CT = 18 / PJ > 6 ? 6 : 18 / PJ, PJS = 2 * K / PJ;       // (k = 1: 8 x 2 x 2 sums and the 16 look-ahead values spill)
    static_assert(PJ * PJS == 2 * K && CT >= 1, "key columns must split evenly");
    const int threads = c->n < 256 ? c->n : 256, sblocks = c->n / threads;
    const size_t groups = (cnt + CT - 1) / CT;
    hipLaunchKernelGGL((relin_mac_multi_f64_kernel<K, CT, PJ, 2>), dim3((unsigned)(groups * CRC_NF64 * PJS * sblocks)), dim3(threads), 0, st, E,
        RelinMultiKeys{{Kf0, Kf1}}, A, a_stride, c->f64, c->n, D, cnt);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}

// whether K3 can carry a polynomial activation's tail (tune.poly_tail = 0): at the default radix.  The radix-16 / -32 variants of the tuning switch "f64_radix"
// would spill with it, so those take poly2_tail_kernel
bool k_relin64_poly_fused(const crc_ctx *c) { return c->tune.poly_tail == 0 && f64_radix(c) == 3; }

static const PoolGeom NO_POOL{0, 0, 0, 0, 0, 0, 0, 0};        // what a kernel that can pool takes when the call does not (xf = 0)

// K3 at one transform radix (RB stages per LDS pass, NPT points per thread of the kernel that holds a row)
template <int RB, int NPT>
static int relin64_tail_rb(crc_ctx *c, const double *A, const u64 *x3, int add_size, u64 *y, size_t cnt, bool out_ntt, hipStream_t st, const u64 *mul,
    const PoolGeom *pool, const PolyTail *poly)
{
    bool lazy = true;
    for (int i = 0; i < c->k; i++) if (c->tabs[i].m.bits > 57 || c->tabs[i].m.bits < 45) lazy = false;
    const size_t blocks = cnt * 2 * c->k;
    const ulonglong2 *Wq = reinterpret_cast<const ulonglong2 *>(c->d_rp);
    const PoolGeom pg = pool ? *pool : NO_POOL;
    // (a polynomial tail goes through relin_inv_crt_kernel at every ring: with it the wave-local kernels spill 4 / 14 / 24 registers per lane at n = 4096 / 8192 /
    // 16384, and what they gain over this kernel is 0.3 to 1.5 % of the sequence)
    if (!poly && f64_wave_path(c, RB, 2)) {
        const int cs = c->logn - 10;
        const bool u64w = f64_wave_path(c, RB, 4);           // (bit 4: the 64-bit forward transform behind the CRT wave-local as well)
#define K3W(A, B, C) (cs == 2 ? relin_inv_crt_wave_kernel<2, A, B, C> : cs == 3 ? relin_inv_crt_wave_kernel<3, A, B, C> : relin_inv_crt_wave_kernel<4, A, B, C>)
        auto kern = !out_ntt ? K3W(false, false, false) : lazy ? (u64w ? K3W(true, true, true) : K3W(true, true, false)) : K3W(true, false, false);
#undef K3W
        return f64_launch(c, kern, blocks, c->n / 16, st, A, x3, add_size, y, c->d_mods, c->d_f64_irp, Wq, c->f64, c->n, c->logn, c->k, mul, pg);
    }
    const int hold = f64_hold_threads(c, RB);
    auto kern = !out_ntt ? relin_inv_crt_kernel<RB, NPT, false, false> : lazy ? relin_inv_crt_kernel<RB, NPT, true, true> : relin_inv_crt_kernel<RB, NPT,
        true, false>;
    if constexpr (RB != 3) { if (poly) return CRC_ERR_UNSUPPORTED; }       // (k_relin64_poly_fused: the wider passes have no registers left for the tail)
    else if (poly)
        return f64_launch(c, lazy ? relin_inv_crt_kernel<RB, NPT, true, true, PolyTail> : relin_inv_crt_kernel<RB, NPT, true, false, PolyTail>, blocks, hold, st, A, x3,
                          add_size, y, c->d_mods, c->d_f64_irp, Wq, c->f64, c->n, c->logn, c->k, mul, pg, *poly);
    return f64_launch(c, kern, blocks, hold, st, A, x3, add_size, y, c->d_mods, c->d_f64_irp, Wq, c->f64, c->n, c->logn, c->k, mul, pg);
}
// K3 (CRT lift, sum with (c0, c1), result form) of the inner products A at the radix in use.  (Defined behind k_relin64_from_digits, its first caller: the
// compiler emits the kernels in the order in which the launchers first name them, and this keeps K2's in front of K3's as they have always been)
static int relin64_tail(crc_ctx *c, const double *A, const u64 *x3, int add_size, u64 *y, size_t cnt, bool out_ntt, hipStream_t st, const u64 *mul = nullptr,
    const PoolGeom *pool = nullptr, const PolyTail *poly = nullptr);
// K2's launcher for the context's k: rc = MAC(k), MAC a macro that names the launcher's instantiation for a literal k; leaves the function where k has none
#define RELIN64_MAC_BY_K(rc, MAC) \
    switch (c->k) { \
    case 1: rc = MAC(1); break; case 2: rc = MAC(2); break; case 3: rc = MAC(3); break; case 4: rc = MAC(4); break; \
    case 5: rc = MAC(5); break; case 6: rc = MAC(6); break; case 7: rc = MAC(7); break; case 8: rc = MAC(8); break; \
    default: return CRC_ERR_UNSUPPORTED; \
    }

// The key switch in two halves.  K1 (k_relin64_digits): the digit polynomials of c2 (q/q_i)^-1, transformed over the fp64 primes, into E at the front of `work`.
// K2 + K3 (k_relin64_from_digits): the inner products of an E that is already there with one prepared key, the CRT lift, and the sum with (c0, c1).  E depends
// on the ciphertext alone, so several keys can be applied to one K1 (the hoisted rotations); k_relinearize64 is the two in a row.
// src / src_size / src_poly: where c2 (q/q_i)^-1 lives; x3 / add_size: the ciphertexts whose (c0, c1) are added; kp: the keys as k_relin64_prepare_keys left
// them; work: relin64_work
int k_relin64_digits(crc_ctx *c, const u64 *src, int src_size, int src_poly, size_t cnt, int dbc, u64 *work, hipStream_t st, const PoolGeom *pool)
{
    if (cnt == 0) return CRC_OK;
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    // (cnt counts POOLED ciphertexts then; src holds the unpooled ones)
    if (pool && !k_relin64_pool_supported(c, dbc, pool->xf * pool->yf)) return CRC_ERR_UNSUPPORTED;
    const int D = relin_digit_count(c, dbc);
    Relin64Tab tab{};                                              // digits of residue i and the index of its first one
    for (int i = 0, g = 0; i < c->k; i++) { tab.L[i] = (unsigned char)evk_digits(c->q[i], dbc); tab.g0[i] = (unsigned char)g; g += tab.L[i]; }
    double *E = relin64_work(c, cnt, dbc, work).E;
    const size_t blocks = cnt * c->k;
    const int RB = f64_radix(c), hold = f64_hold_threads(c, RB), cs = c->logn - 10;
    if (pool) {
        // all digit sums of a value in one word when they fit: fields of F = dbc + log2 W bits, the top digit of residue i has bits_i - (L_i - 1) dbc (+ log2
        // W) bits
        int wbits = 0; while ((1 << wbits) < pool->xf * pool->yf) wbits++;
        const int F = dbc + wbits;
        bool one = true;
        for (int i = 0; i < c->k; i++) { const int L = tab.L[i]; if ((L - 1) * F + ((int)c->tabs[i].m.bits - (L - 1) * dbc + wbits) > 64 || F > 32) one =
            false; }
        if (one && f64_wave_path(c, RB, 1))
            return f64_launch(c, cs == 2 ? relin_digits_wave_kernel<2, true> : cs == 3 ? relin_digits_wave_kernel<3, true> : relin_digits_wave_kernel<4, true>, blocks,
                              c->n / 16, st, src, src_size, src_poly, E, c->d_f64_rp, c->f64, c->n, c->k, D, dbc, tab, *pool, F);
        auto kern = RB == 3 ? (one ? relin_digits_pool_f64_kernel<3, 16, true> : relin_digits_pool_f64_kernel<3, 16, false>)
                  : RB == 4 ? (one ? relin_digits_pool_f64_kernel<4, 16, true> : relin_digits_pool_f64_kernel<4, 16, false>)
                            : (one ? relin_digits_pool_f64_kernel<5, 32, true> : relin_digits_pool_f64_kernel<5, 32, false>);
        return f64_launch(c, kern, blocks, hold, st, src, src_size, src_poly, E, c->d_f64_rp, c->f64, c->n, c->logn, c->k, D, dbc, tab, *pool, F);
    }
    if (f64_wave_path(c, RB, 1))
        return f64_launch(c, cs == 2 ? relin_digits_wave_kernel<2, false> : cs == 3 ? relin_digits_wave_kernel<3, false> : relin_digits_wave_kernel<4, false>, blocks,
                          c->n / 16, st, src, src_size, src_poly, E, c->d_f64_rp, c->f64, c->n, c->k, D, dbc, tab, NO_POOL, dbc);
    return f64_launch(c, RB == 3 ? relin_digits_f64_kernel<3, 16> : RB == 4 ? relin_digits_f64_kernel<4, 16> : relin_digits_f64_kernel<5, 32>, blocks, hold, st, src,
                      src_size, src_poly, E, c->d_f64_rp, c->f64, c->n, c->logn, c->k, D, dbc, tab);
}
int k_relin64_from_digits(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y, u64 *work, const u64 *kp, hipStream_t st, bool out_ntt,
                          const PoolGeom *pool, const u64 *mul, const PolyTail *poly)
{
    if (cnt == 0) return CRC_OK;
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    if (pool && !k_relin64_pool_supported(c, dbc, pool->xf * pool->yf)) return CRC_ERR_UNSUPPORTED;
    const Relin64Work w = relin64_work(c, cnt, dbc, work);
    const double *Kf = reinterpret_cast<const double *>(kp);
    int rc;
#define MAC(KV) (c->tune.relin_mac_ct == 8 ? relin64_mac<KV, 8>(c, w.E, Kf, w.A, w.D, cnt, st) : relin64_mac<KV, 4>(c, w.E, Kf, w.A, w.D, cnt, st))
    RELIN64_MAC_BY_K(rc, MAC)
#undef MAC
    if (rc) return rc;
    if ((mul || poly) && !out_ntt) return CRC_ERR_INVALID_ARGUMENT;
    // (pooled: x3 / add_size are the UNPOOLED ciphertexts whose (c0, c1) K3 adds up window by window)
    return relin64_tail(c, w.A, x3, add_size, y, cnt, out_ntt, st, mul, pool, poly);
}
static int relin64_tail(crc_ctx *c, const double *A, const u64 *x3, int add_size, u64 *y, size_t cnt, bool out_ntt, hipStream_t st, const u64 *mul, const PoolGeom *pool,
    const PolyTail *poly)
{
    const int RB = f64_radix(c);
    return RB == 3 ? relin64_tail_rb<3, 16>(c, A, x3, add_size, y, cnt, out_ntt, st, mul, pool, poly)
         : RB == 4 ? relin64_tail_rb<4, 16>(c, A, x3, add_size, y, cnt, out_ntt, st, mul, pool, poly)
                   : relin64_tail_rb<5, 32>(c, A, x3, add_size, y, cnt, out_ntt, st, mul, pool, poly);
}
int k_relinearize64(crc_ctx *c, const u64 *src, int src_size, int src_poly, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y, u64 *work, const u64 *kp,
                    hipStream_t st, bool out_ntt, const PoolGeom *pool, const u64 *mul, const PolyTail *poly)
{
    const int rc = k_relin64_digits(c, src, src_size, src_poly, cnt, dbc, work, st, pool);
    return rc ? rc : k_relin64_from_digits(c, x3, add_size, cnt, dbc, y, work, kp, st, out_ntt, pool, mul, poly);
}

// scratch of K2 + K3 for `keys` keys at once: one more A per further key behind k_relin64_work_words
size_t k_relin64_work_words_multi(const crc_ctx *c, size_t cnt, int dbc, int keys)
{
    return k_relin64_work_words(c, cnt, dbc) + (size_t)(keys > 1 ? keys - 1 : 0) * relin64_work(c, cnt, dbc).a_stride;
}
// K2 + K3 of TWO prepared keys on the E that is there (relin_mac_multi_f64_kernel): y0 / y1 what k_relin64_from_digits gives with kp0 / kp1, bit for bit.
// work: k_relin64_work_words_multi(.., 2)
int k_relin64_from_digits2(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y0, u64 *y1, u64 *work, const u64 *kp0, const u64 *kp1,
                           hipStream_t st, bool out_ntt)
{
    if (cnt == 0) return CRC_OK;
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    const Relin64Work w = relin64_work(c, cnt, dbc, work);
    const double *K0 = reinterpret_cast<const double *>(kp0), *K1 = reinterpret_cast<const double *>(kp1);
    int rc;
#define MAC(KV) relin64_mac2<KV>(c, w.E, K0, K1, w.A, w.a_stride, w.D, cnt, st)
    RELIN64_MAC_BY_K(rc, MAC)
#undef MAC
    if (rc) return rc;
    if ((rc = relin64_tail(c, w.A, x3, add_size, y0, cnt, out_ntt, st))) return rc;
    return relin64_tail(c, w.A + w.a_stride, x3, add_size, y1, cnt, out_ntt, st);
}

// K2 + K3 with one prepared key per STEP of the batch (relin_mac_keyed_f64_kernel): the cnt ciphertexts are [cnt / per_key][per_key], the ciphertexts of step j take
// the key kp_table[j] -- a DEVICE array of cnt / per_key pointers to prepared keys (k_relin64_prepare_keys).  E is there (k_relin64_digits over all cnt); y what
// k_relin64_from_digits gives for every step with its key, bit for bit.  work: relin64_work(cnt)
template <int K>
static int relin64_mac_keyed(crc_ctx *c, const double *E, const double *const *keys, double *A, int D, size_t steps, size_t per, hipStream_t st)
{
    constexpr int PJ = 2 * K <= 8 ? 2 * K : (2 * K) % 8 == 0 ? 8 : (2 * K) % 6 == 0 ? 6 : (2 * K) % 5 == 0 ? 5 : 7, PJS = 2 * K / PJ;
    static_assert(PJ * PJS == 2 * K, "key columns must split evenly");
    const int threads = c->n < 256 ? c->n : 256;
    const int ct = per == 1 ? 1 : per == 2 ? 2 : 4, sv = ct == 1 && c->n >= 512 ? 2 : 1;
    const size_t groups = (per + ct - 1) / ct, blocks = steps * groups * CRC_NF64 * PJS * (c->n / (threads * sv));
    if (blocks > 0x7fffffffull || steps > 0xffffffffull || per > 0xffffffffull) return CRC_ERR_INVALID_ARGUMENT;
#define KEYED(CT, SV) hipLaunchKernelGGL((relin_mac_keyed_f64_kernel<K, CT, PJ, SV>), dim3((unsigned)blocks), dim3(threads), 0, st, E, keys, A, c->f64, c->n, D, \
        (unsigned)steps, (unsigned)per)
    if (ct == 1 && sv == 2) KEYED(1, 2);
    else if (ct == 1) KEYED(1, 1);
    else if (ct == 2) KEYED(2, 1);
    else KEYED(4, 1);
#undef KEYED
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
int k_relin64_from_digits_keyed(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, size_t per_key, int dbc, u64 *y, u64 *work, const u64 *const *kp_table,
                                hipStream_t st, bool out_ntt)
{
    if (cnt == 0) return CRC_OK;
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    if (per_key < 1 || cnt % per_key || !kp_table) return CRC_ERR_INVALID_ARGUMENT;
    const Relin64Work w = relin64_work(c, cnt, dbc, work);
    const double *const *keys = reinterpret_cast<const double *const *>(kp_table);
    int rc;
#define MAC(KV) relin64_mac_keyed<KV>(c, w.E, keys, w.A, w.D, cnt / per_key, per_key, st)
    RELIN64_MAC_BY_K(rc, MAC)
#undef MAC
    return rc ? rc : relin64_tail(c, w.A, x3, add_size, y, cnt, out_ntt, st);
}

// kp_table for k_relin64_from_digits_keyed, built on the device: table[j] = base + slot[j] kpw words, null where slot[j] < 0 (a step without a key).  The slots
// travel as kernel arguments, KEY_TABLE_MAX per launch, as the pointer tables of the galois kernels do: no host memory is read after the call returns
enum { KEY_TABLE_MAX = 256 };
struct KeyTableSlots { int slot[KEY_TABLE_MAX]; };
__global__ void __launch_bounds__(KEY_TABLE_MAX) relin_key_table_kernel(const u64 *base, size_t kpw, KeyTableSlots s, int cnt, const u64 **table)
{
    const int i = threadIdx.x;
    if (i < cnt) table[i] = s.slot[i] < 0 ? nullptr : base + (size_t)s.slot[i] * kpw;
}
int k_relin64_key_table(const u64 *base, size_t kpw, const int *slots, size_t steps, const u64 **table, hipStream_t st)
{
    if (steps && (!base || !slots || !table)) return CRC_ERR_INVALID_ARGUMENT;
    for (size_t j0 = 0; j0 < steps; j0 += KEY_TABLE_MAX) {
        KeyTableSlots s{};
        const int cnt = steps - j0 < KEY_TABLE_MAX ? (int)(steps - j0) : (int)KEY_TABLE_MAX;
        for (int i = 0; i < cnt; i++) s.slot[i] = slots[j0 + i];
        hipLaunchKernelGGL(relin_key_table_kernel, dim3(1), dim3(KEY_TABLE_MAX), 0, st, base, kpw, s, cnt, table + j0);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}
