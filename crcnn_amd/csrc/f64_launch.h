// f64_launch.h -- host side of the fp64 row kernels (kernels_square64.hip, kernels_relin64.hip; device side: ntt_f64.h): how the ring and the tuning switches
// shape a launch, and the launch itself.  Every such kernel works on one row of n doubles in dynamic LDS
#pragma once
#include "ctx.h"

// 3 stages (8 values per thread) per LDS pass by default: measured on (8192, 3) the digit kernel runs 0.90 / 1.08 / 1.34 us per ciphertext with 3 / 4 / 5 --
// the wider passes save LDS round trips and barriers but cost occupancy (76 / 134 registers), and the kernel is bound by instruction issue, not by LDS
// (profiles/r03_square_relin.txt)
static inline int f64_radix(const crc_ctx *c) { const int r = c->tune.f64_radix; return r >= 3 && r <= 5 ? r : 3; }
// threads per workgroup for passes of 2^RB values per thread
static inline int f64_threads(const crc_ctx *c, int RB) { int nt = c->n >> RB; if (nt < 64) nt = 64; if (nt > (RB == 5 ? 512 : 1024)) nt = RB == 5 ? 512 : 1024;
    return nt; }
// threads of the kernels that keep a row in registers
// (16 points per thread at radix 8 and 16, 32 at radix 32: n / 16 threads, at least a wave, at most 1024)
static inline int f64_hold_threads(const crc_ctx *c, int RB) { int nt = c->n >> (RB == 5 ? 5 : 4); if (nt < 64) nt = 64;
    if (nt > (RB == 5 ? 512 : 1024)) nt = RB == 5 ? 512 : 1024; return nt; }
// the wave-local transforms (one workgroup barrier per transform, n / 16 threads) serve n = 4096 (CS = 2, since round 6), 8192 and 16384 at the default radix;
// CRC_F64_WAVE=0 keeps the round-4 kernels.  Bit 0: sq64_inv_kernel / mul64_inv_kernel (-25 % at both bench rings), bit 1: the digit kernel, bit 2: K3, bit 3: the
// lifting forward kernel (+2 % / +31 %: it has no row to hold and the round-4 form runs it at eight waves per SIMD; off by default), bit 4: K3's 64-bit forward
// transform.  (Measured, same box: K1 -17 % at n = 8192, -16 % at 16384; K3 +3 % / +14 % in its first form, which parked the first prime's result in scratch,
// -0.3 % / -1.5 % of the whole sequence now: profiles/r05_square_pool_wave_local_*.txt)
static inline bool f64_wave_path(const crc_ctx *c, int RB, int bit)
{
    if (RB != 3 || (c->logn != 12 && c->logn != 13 && c->logn != 14)) return false;
    const int sel = c->tune.f64_wave < 0 ? 7 : c->tune.f64_wave;
    return (sel >> bit) & 1;
}

// one launch of a row kernel: the kernel's dynamic-LDS limit covers the row, `blocks` workgroups of `threads`, the error check
template <class... P, class... A>
static inline int f64_launch(crc_ctx *c, void (*kern)(P...), size_t blocks, int threads, hipStream_t st, const A &...args)
{
    const size_t lds = (size_t)c->n * 8;
    if (const int rc = crc_ctx_ensure_lds(c, (const void *)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), lds, st, args...);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
