// modswitch_device.h -- device side of modulus switching (kernels_modswitch.hip): the constants, the arithmetic of one coefficient, and the bodies of the three
// kernels.  A header so that tests/cpp/mod_switch_kernel_check.cpp can run the same text on the CPU, one thread per workgroup, under sanitizers.
//
// From k moduli q_0 .. q_{k-1} to the first k' (D = k - k' drops, drop j takes p_j = q_{k-1-j}, h_j = p_j >> 1):  c <- floor((c + h_j) / p_j), j = 0 .. D-1.
// In residues: u_j = (c_{k-1-j} + h_j) mod p_j is the remainder shifted by h_j (r_j = u_j - h_j is the centred one); every row i below k-1-j becomes
// (c_i - r_j) p_j^-1 mod q_i.  The D dropped rows are updated among themselves in registers (ms_remainders); a kept row takes all D corrections at once:
//      c'_i = (c_i - R) (p_0 .. p_{D-1})^-1 mod q_i,      R = r_0 + p_0 r_1 + p_0 p_1 r_2 + ...      (the same residue as D updates one after another)
// R mod q_i does not depend on c_i, and the row transform is linear: NTT(c'_i) = (NTT(c_i) - NTT(R mod q_i)) P^-1, so a kept NTT-form row is never transformed
// back (modswitch_rows_body with a null `kept_coeff`).
#pragma once
#include "ntt_device.h"

#ifndef CRC_MAXK
#define CRC_MAXK 8
#endif

// by value in the kernels' argument block; [j][i]: drop j, modulus i < k - 1 - j (the other entries are 0 and never read)
struct ModSwitchConsts {
    int k, kept;                                        // moduli before / after; drops D = k - kept is the kernels' template parameter
    u64 q[CRC_MAXK], one_s[CRC_MAXK];                   // the moduli and floor(2^64 / q_i): mulmod_shoup(v, 1, one_s, q) is v mod q for any 64-bit v
    u64 h[CRC_MAXK];                                    // h_j = p_j >> 1
    u64 hmod[CRC_MAXK][CRC_MAXK];                       // h_j mod q_i
    u64 pinv[CRC_MAXK][CRC_MAXK], pinv_s[CRC_MAXK][CRC_MAXK];      // p_j^-1 mod q_i and its Shoup companion, for the dropped rows i >= kept
    u64 pmod[CRC_MAXK][CRC_MAXK], pmod_s[CRC_MAXK][CRC_MAXK];      // p_0 .. p_{j-1} mod q_i (j >= 1) and its Shoup companion, for the kept rows i < kept
    u64 Pinv[CRC_MAXK], Pinv_s[CRC_MAXK];               // (p_0 .. p_{D-1})^-1 mod q_i, i < kept
};

// last[m] = the residue mod q_{kept + m} of one coefficient, m < D (canonical)  ->  u[j] = the shifted remainder of drop j, in [0, p_j)
template <int D>
__device__ __forceinline__ void ms_remainders(const ModSwitchConsts &c, u64 (&last)[D], u64 (&u)[D])
{
#pragma unroll
    for (int j = 0; j < D; j++) {
        const int top = D - 1 - j;                      // index into last[] of the row that drop j removes; its modulus is q[kept + top] = p_j
        const u64 p = c.q[c.kept + top];
        u[j] = addmod(last[top], c.h[j], p);
#pragma unroll
        for (int m = 0; m < top; m++) {                 // the dropped rows still alive: (c - u + h) p_j^-1
            const int i = c.kept + m; const u64 q = c.q[i];
            const u64 um = mulmod_shoup(u[j], 1, c.one_s[i], q);
            last[m] = mulmod_shoup(last[m] + (q - um) + c.hmod[j][i], c.pinv[j][i], c.pinv_s[j][i], q);        // the sum is below 3 q < 2^64
        }
    }
}
// R mod q_i, canonical, for a kept modulus i
template <int D>
__device__ __forceinline__ u64 ms_correction(const ModSwitchConsts &c, const u64 (&u)[D], int i)
{
    const u64 q = c.q[i];
    u64 R = 0;
#pragma unroll
    for (int j = 0; j < D; j++) {
        const u64 r = mulmod_shoup(u[j], 1, c.one_s[i], q) + (q - c.hmod[j][i]);                               // r_j mod q_i, below 2 q
        R = addmod(R, j ? mulmod_shoup(r, c.pmod[j][i], c.pmod_s[j][i], q) : (r >= q ? r - q : r), q);
    }
    return R;
}
__device__ __forceinline__ u64 ms_kept(const ModSwitchConsts &c, u64 ci, u64 R, int i)
{
    return mulmod_shoup(ci + (c.q[i] - R), c.Pinv[i], c.Pinv_s[i], c.q[i]);
}

// Rows are addressed as base + poly * poly_stride + row * n, so that the dropped rows can come from the input tensor ([polys][k][n], rows kept ..) or from the
// work space the inverse pass has filled ([polys][rows][n]).
struct ModSwitchArgs {
    const u64 *kept_in; size_t kept_ps;                 // the kept rows i < kept of a polynomial
    const u64 *drop_in; size_t drop_ps;                 // its D dropped rows, coefficient form: row m at drop_in + poly * drop_ps + m * n
    u64 *out;                                           // [polys][kept][n]
    const ulonglong2 *W;                                // [k][n] {root power, Shoup companion}: the forward tables (rows kernel), the inverse-div-2 ones (inverse kernel)
    size_t polys;
    int n, logn;
    int row0, rows;                                     // inverse kernel: rows row0 .. row0 + rows - 1 of every polynomial
    int kept_ntt;                                       // rows kernel: the kept rows are in NTT form (only R is transformed), else in coefficient form
    ModSwitchConsts c;
};

// ---- coefficient form in, coefficient form out: elementwise, a lane owns the pair (s, s + 1) of one polynomial -----------------------------------------------
template <int D>
__device__ __forceinline__ void modswitch_coeff_body(const ModSwitchArgs &a)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int hl = a.logn - 1;
    const size_t poly = idx >> hl;
    if (poly >= a.polys) return;
    const int s = (int)(idx & (((size_t)1 << hl) - 1)) * 2;
    const u64 *dr = a.drop_in + poly * a.drop_ps + s;
    u64 lx[D], ly[D], ux[D], uy[D];
#pragma unroll
    for (int m = 0; m < D; m++) { const ulonglong2 v = ld2(dr + (size_t)m * a.n); lx[m] = v.x; ly[m] = v.y; }
    ms_remainders<D>(a.c, lx, ux);
    ms_remainders<D>(a.c, ly, uy);
    const u64 *src = a.kept_in + poly * a.kept_ps + s;
    u64 *dst = a.out + poly * ((size_t)a.c.kept * a.n) + s;
    for (int i = 0; i < a.c.kept; i++) {
        const ulonglong2 v = ld2(src + (size_t)i * a.n);
        st2(dst + (size_t)i * a.n, ms_kept(a.c, v.x, ms_correction<D>(a.c, ux, i), i), ms_kept(a.c, v.y, ms_correction<D>(a.c, uy, i), i));
    }
}

// ---- NTT-form rows row0 .. row0 + rows - 1 of every polynomial -> coefficient form, into work space [polys][rows][n]: one workgroup per row ---------------------
template <bool LAZY>
__device__ __forceinline__ void modswitch_inverse_body(const ModSwitchArgs &a, u64 *sm)
{
    const size_t item = blockIdx.x;
    if (item >= a.polys * (size_t)a.rows) return;
    const size_t poly = item / (size_t)a.rows; const int m = (int)(item - poly * (size_t)a.rows), i = a.row0 + m;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 q = a.c.q[i], one_s = a.c.one_s[i];
    const u64 *src = a.kept_in + poly * a.kept_ps + (size_t)i * n;
    for (int s = 2 * tid; s < n; s += 2 * nt) { const ulonglong2 p = ld2(src + s); sm_store_pair64(sm, s, p.x, p.y); }
    __syncthreads();
    ntt_row_passes<true, LAZY, 3, false>(sm, a.W + (size_t)i * n, n, a.logn, q, q + q);
    u64 *dst = a.out + item * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // below 16 q (lazy) / 2 q (strict): one Shoup reduction makes it canonical
        st2(dst + s, mulmod_shoup(r.x, 1, one_s, q), mulmod_shoup(r.y, 1, one_s, q));
    }
}

// ---- NTT form out: one workgroup per (polynomial, kept modulus i), the kept moduli of a polynomial in one XCD group (they read the same D dropped rows) --------
// kept_ntt: the image is R mod q_i, the drain reads the kept NTT row: (c_i - x) P^-1.  Otherwise (coefficient-form input) the image is the switched row itself.
template <int D, bool LAZY>
__device__ __forceinline__ void modswitch_rows_body(const ModSwitchArgs &a, u64 *sm)
{
    size_t poly; unsigned member;
    if (!xcd_group(blockIdx.x, (unsigned)a.c.kept, a.polys, poly, member)) return;
    const int i = (int)member;
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const u64 q = a.c.q[i], one_s = a.c.one_s[i];
    const u64 *dr = a.drop_in + poly * a.drop_ps;
    const u64 *src = a.kept_in + poly * a.kept_ps + (size_t)i * n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        u64 lx[D], ly[D], ux[D], uy[D];
#pragma unroll
        for (int m = 0; m < D; m++) { const ulonglong2 v = ld2(dr + (size_t)m * n + s); lx[m] = v.x; ly[m] = v.y; }
        ms_remainders<D>(a.c, lx, ux);
        ms_remainders<D>(a.c, ly, uy);
        u64 x = ms_correction<D>(a.c, ux, i), y = ms_correction<D>(a.c, uy, i);
        if (!a.kept_ntt) { const ulonglong2 v = ld2(src + s); x = ms_kept(a.c, v.x, x, i); y = ms_kept(a.c, v.y, y, i); }
        sm_store_pair64(sm, s, x, y);
    }
    __syncthreads();
    ntt_row_passes<false, LAZY, 3, false>(sm, a.W + (size_t)i * n, n, a.logn, q, q + q);
    u64 *dst = a.out + (poly * (size_t)a.c.kept + i) * (size_t)n;
    for (int s = 2 * tid; s < n; s += 2 * nt) {
        const ulonglong2 r = sm_load_pair64(sm, s);                    // below (1 + 4 log2 n) q (lazy) / 4 q (strict)
        const u64 x = mulmod_shoup(r.x, 1, one_s, q), y = mulmod_shoup(r.y, 1, one_s, q);
        if (a.kept_ntt) { const ulonglong2 v = ld2(src + s); st2(dst + s, ms_kept(a.c, v.x, x, i), ms_kept(a.c, v.y, y, i)); }
        else st2(dst + s, x, y);
    }
}
