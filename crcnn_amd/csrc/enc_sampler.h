// enc_sampler.h -- the pieces every device sampler decodes a keystream block with: the encryptor's noise magnitude and ternary sample (kernels_client.hip) and
// the reduction of a 128-bit keystream integer modulo a coefficient modulus.  Shared by the encryptors and the flood (flood_device.h); a header so that the
// flood's sampler also compiles for the CPU check of its kernel bodies.
#pragma once
#include "modarith.h"

// The noise law, exactly: SEAL draws g ~ N(0, 3.19^2), redraws while |g| > 6 sigma = 19.14 (util/clipnormal.h) and keeps static_cast<int64_t>(g)
// (encryptor.cpp:237-240) -- an integer in [-19, 19] with  P(0) = P(|g| < 1) / Z,  P(+-a) = P(a <= g < a + 1) / Z (a < 19),  P(+-19) = P(19 <= g <= 19.14) / Z,
// Z = P(|g| <= 19.14).  Sampling that integer directly needs no logarithm, cosine or rejection loop: the magnitude is the number of thresholds
// T_a = floor(2^64 P(|e| <= a)) (a = 0..18; enc_cdt in kernels_client.hip, computed once on the host in long double) that a uniform 64-bit word reaches -- the
// law above to 2^-63.
struct EncCdt { u64 t[19]; };
__device__ __forceinline__ int cdt_noise(u32 lo, u32 hi, u32 sign, const EncCdt &T)
{
    const u64 x = ((u64)hi << 32) | lo;
    int a = 0;
#pragma unroll
    for (int j = 0; j < 19; j++) a += x >= T.t[j] ? 1 : 0;
    return sign ? -a : a;
}
// 64 bits as 2-bit fields, rejecting 3: all 32 fields equal to 3 has probability 2^-64 and falls back to 0.  0, 1, 2 stand for 0, 1, -1
__device__ __forceinline__ u32 ternary_field(u32 lo, u32 hi)
{
    const u64 w = (u64)lo | ((u64)hi << 32);
    u32 v = 0;
    for (int j = 0; j < 32; j++) { const u32 f = (u32)(w >> (2 * j)) & 3u; if (f != 3u) { v = f; break; } }
    return v;
}

// z = hi 2^64 + lo -> z mod q for ANY 128-bit z.  The generic Barrett path's quotient estimate is off by at most one only for z < 2^64 q: the high word is
// reduced first there (the folding path takes any z)
__device__ __forceinline__ u64 mod128_any(u64 lo, u64 hi, const ModParams &m)
{
    if (m.fold) return fold128(lo, hi, m);
    return barrett128(lo, barrett128(hi, 0, m), m);
}
