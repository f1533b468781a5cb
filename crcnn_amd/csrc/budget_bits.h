// budget_bits.h -- one coefficient of Decryptor::invariant_noise_budget (SEAL decryptor.cpp:295-403): the k residues of v = c0 + c1 s (+ c2 s^2) in, the bit
// length of | t v mod q | (centred) out.  __host__ __device__: budget_norm_kernel (kernels_budget.hip) and crc_budget_bits_host run this same text.
//
//     x_i = v_i (t (q/q_i)^-1 mod q_i) mod q_i                        one Shoup multiplication (the constant is BehzParams.t_inv_qhat)
//     acc = sum_i x_i (q/q_i) mod q                                   K-word sum; every term is below q, so ONE conditional subtraction of q per term keeps acc < q
//     acc = acc > floor(q/2) ? q - acc : acc                          decryptor.cpp:376-384
//     bits = significant bits of acc                                  :386-403 takes them of the maximum over the coefficients: the maximum of the bit lengths
//
// Exact integers throughout; K is a compile-time constant so the accumulator is K registers wide and every index below is static.
#pragma once
#include "ctx.h"

struct BudgetParams {                            // by value to the kernel
    int k, total_bits;                           // significant bits of q (context.cpp: total_coeff_modulus_bit_count)
    u64 qi[CRC_MAXK];
    u64 xc[CRC_MAXK], xc_s[CRC_MAXK];            // t (q/q_i)^-1 mod q_i and its Shoup companion
    u64 qhat[CRC_MAXK][CRC_MAXK];                // q/q_i, little-endian words
    u64 q[CRC_MAXK], half[CRC_MAXK];             // q and floor(q/2)
};

template <int K> CRC_HD int budget_coeff_bits(const u64 *v, size_t stride, const BudgetParams &bp)
{
    u64 acc[K];
#pragma unroll
    for (int l = 0; l < K; l++) acc[l] = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const u64 x = mulmod_shoup(v[(size_t)i * stride], bp.xc[i], bp.xc_s[i], bp.qi[i]);
        // acc += x (q/q_i): the product is below q < 2^(64K - 1), so neither carry leaves word K - 1
        u64 mc = 0, ac = 0;
#pragma unroll
        for (int l = 0; l < K; l++) {
            u64 lo, hi; mul64wide(x, bp.qhat[i][l], lo, hi);
            const u64 term = lo + mc; mc = hi + (term < lo);
            const u64 s = acc[l] + term, s2 = s + ac;
            ac = (u64)(s < term) | (u64)(s2 < s);
            acc[l] = s2;
        }
        // acc >= q ? acc - q : acc
        u64 d[K], br = 0;
#pragma unroll
        for (int l = 0; l < K; l++) {
            const u64 a = acc[l], b = bp.q[l], w = a - b;
            d[l] = w - br; br = (u64)(a < b) | (u64)(w < br);
        }
#pragma unroll
        for (int l = 0; l < K; l++) acc[l] = br ? acc[l] : d[l];
    }
    // floor(q/2) - acc borrows exactly when acc > floor(q/2)
    u64 br = 0;
#pragma unroll
    for (int l = 0; l < K; l++) { const u64 a = bp.half[l], b = acc[l], w = a - b; br = (u64)(a < b) | (u64)(w < br); }
    if (br) {
        u64 b2 = 0;
#pragma unroll
        for (int l = 0; l < K; l++) { const u64 a = bp.q[l], b = acc[l], w = a - b; acc[l] = w - b2; b2 = (u64)(a < b) | (u64)(w < b2); }
    }
    int bits = 0;
#pragma unroll
    for (int l = 0; l < K; l++) if (acc[l]) bits = 64 * l + 64 - __builtin_clzll(acc[l]);
    return bits;
}
