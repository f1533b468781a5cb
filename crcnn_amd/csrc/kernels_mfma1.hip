// kernels_mfma1.hip -- one-channel convolutions (CrCNN's conv1, alone or fused with its pooling layer: 6 x 6 / 7 x 7 windows over the 28 x 28 encrypted image,
// 32 / 20 filters) on the matrix cores.
//
// With one input channel the reduction is xf*yf = 36..49 terms.  As a generic limb GEMM (kernels_mfma.hip) that is two reduction steps per output tile and the
// per-output work -- recombining 13 diagonals and reducing mod q -- dominates; on the vector ALU (mac3_kernel) the layer runs at 3.5 T modmul/s and, once conv2
// and fc3 moved to the matrix cores, is a third of PlainModelTiny.  This kernel is built around the two things such a layer offers:
//   reuse     per slot the window taps are K = 8 rows x 8 columns = 64 (zero weights beyond the window): ONE v_mfma_i32_16x16x64_i8 per limb pair covers the
//             whole reduction.  The 7 weight fragments of a wave's 16 filters live in registers for the whole workgroup, and a workgroup walks ALL images of
//             the chunk for its slot (image b+1 arrives by LDS-DMA while image b is multiplied);
//   a cheap   the accumulators start at per-diagonal biases B_d (so every diagonal stays in [0, 2^24) and their sum is a multiple of q: no signs, no
//   epilogue  correction term), pairs of diagonals pack into 32-bit words without carries, the 128-bit value is two word vectors added once.  Round 4: the
//   value is
//             reduced by FOLDING (q = 2^b - f: three folds, 3 + 1 multiplies: limbred.h diag_fold_short_centred) instead of a Montgomery step (7 quarter-rate
//             multiplies: 112 of ~370 issue cycles per output), and the MFMA operands are swapped -- weights as the A operand, image windows as B -- so that a
//             lane's four
//             accumulator registers are FOUR CONSECUTIVE FILTERS of one output row: their digit bytes transpose in registers (v_perm_b32) into one dword per
//             limb plane,
//             stored with 7 ds_write_b32 per four outputs instead of 28 byte stores (the byte-wise staging was most of the 23 % of CU cycles lost to LDS bank
//             conflicts, profiles/r03_pmc_conv1_issue.json; the two polys' image blocks now sit 8 banks apart for the window reads).
// 8 or 12 waves per workgroup (2-3 per SIMD: one wave's epilogue overlaps another's MFMAs); a wave owns 16 filters and every (waves/2)-th 16-row tile.
//   per image  the limb image [plane][poly][row + 1 pad][32 columns] (13 KiB for 28 x 28) in LDS, double-buffered; a lane's A fragment is two 8-byte LDS reads
//   per
//               plane (window rows kx, kx+1): the three words around byte offset oy * stride, byte-aligned in registers;
//   output      either the limb tensor of a following convolution, staged in LDS and written out as one contiguous [plane][pixel][poly][32 channels] block
//               (no limb_pack_tensor pass in front of conv2), or slot-major u64 for the generic conversions. Exact integer arithmetic throughout: the same
//               element of Z_q, hence the same bits, as mac3_kernel and the reference (convolutionalLayer.cpp:56-93).
// Two forms of the kernel share the epilogue's end (conv1_store4, conv1_copy_out): the plane-major one described above (mfma_conv1_kernel: any window up to
// 8 x 8, the packed second filter group of 17-20 filters) and, for windows of at most 40 taps, the pixel-major one further down (mfma_conv1_kernel_px: 35 MFMAs
// and 7 diagonals per tile, no window cutting, one fold).  k_limb_conv1_form picks per layer; the tuning key conv1_form forces one.
#include "kernels.h"
#include "limbred.h"
#include "boxstage.h"
#include "conv1_rowtab.h"
#include <cstdlib>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef signed char i8;
#define NPL 7
#define MAXK 8                                   // coefficient moduli (kernel argument tables)

struct Conv1Args {
    const i8 *xr; const i8 *wl; u64 *ys; i8 *xl_out; const ModParams *mods; const u64 *bias;
    int n, k, B, Bout, b0, xd, yo, xs, ystr, P, F, mtiles;   // B images in this launch; the limb result is image b0 + b of Bout
    // per (slot, image): 7 planes x 2 polys x xd rows x 32 bytes (+ 8: the last window may read past its row), rounded up to 1 KiB
    unsigned img_stride, plane_bytes, poly_bytes;
    // limb output, bytes per image: 7 * P * 2 * 32, or the flat form's 7 * 2 * P * zdc rounded up to 16 (kernels_mfma.hip)
    unsigned out_img_bytes;
    // flat form (fewer than 32 filters = channels of the next convolution): channel bytes per position, else 0
    int out_zdc;
    // 16 < F <= 20: the second filter group has at most four filters -- its waves pack (filter, weight limb) into the 16 rows of
    int narrow;
                                                       // the MFMA's A operand: 14 MFMAs and ONE output per lane and tile instead of 49 and four
                                                       // (mfma_conv1_kernel)
    int acc0[MAXK][13];                                // initial value of the 13 diagonal accumulators, per modulus (conv1_tables)
    u32 qbits[MAXK], qfold[MAXK];                      // q = 2^qbits - qfold (limbred.h conv1_fold_ok)
    // pixel-major form (mfma_conv1_kernel_px): image [poly][row][column] of 8-byte pixels, rows px_rs bytes apart (poly_bytes between the polys); taps = xf * yf,
    // tap = kx * yf + ky; px_pair: taps 2G and 2G + 1 are always neighbouring pixels at an even column (one 16-byte read per K group)
    unsigned px_rs;
    int px_taps, px_yf, px_pair;
    int acc7[MAXK][7];                                 // biases of the seven weight-digit diagonals (limbred.h conv1_bias7_table)
};

// canonical residue -> 7 balanced base-256 digits of its centred representative
__device__ __forceinline__ void limb_digits1(u64 r, u64 q, int (&d)[NPL])
{
    long long v = r > (q >> 1) ? (long long)r - (long long)q : (long long)r;
#pragma unroll
    for (int l = 0; l < NPL; l++) { d[l] = (int)(signed char)(v & 0xff); v = (v - d[l]) >> 8; }
}

// the end of a tile's epilogue, shared by both forms of the kernel: four consecutive filters f0 .. f0 + 3 of output row mm (pixel mm >> 1, poly mm & 1) of image b,
// given as centred representatives; sp = the staging byte of (row mm, channel f0, plane 0), the planes pstride bytes apart (conv1_rowtab.h)
__device__ __forceinline__ void conv1_store4(const Conv1Args &a, i8 *sp, unsigned pstride, const long long (&cv)[4], int mm, int f0, int chan_bytes, u64 q, int slot,
                                             int b)
{
    if (mm >= 2 * a.P) return;
    // limb tensor of the next convolution, staged in LDS as it leaves, in the tensor's own layout: [plane][row][32 channels], or the flat form
    // [plane][poly][pixel][zdc]
    if (a.xl_out) {
        if (f0 >= chan_bytes) return;                                      // (flat form: channel padding is a multiple of 4, this group is past it)
        u32 lo[4], hi[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) { const u64 dg = f0 + reg < a.F ? centred_digit_bytes(cv[reg]) : 0; lo[reg] = (u32)dg;
            hi[reg] = (u32)(dg >> 32); }
        // 4 x 7 byte transpose: dword l = digit l of the four filters (v_perm_b32: result byte = selector byte picks from {second operand: 0-3, first:
        // 4-7})
        const u32 t0 = __builtin_amdgcn_perm(lo[1], lo[0], 0x05010400u), t1 = __builtin_amdgcn_perm(lo[1], lo[0], 0x07030602u);
        const u32 u0 = __builtin_amdgcn_perm(lo[3], lo[2], 0x05010400u), u1 = __builtin_amdgcn_perm(lo[3], lo[2], 0x07030602u);
        const u32 t2 = __builtin_amdgcn_perm(hi[1], hi[0], 0x05010400u), t3 = __builtin_amdgcn_perm(hi[1], hi[0], 0x07030602u);
        const u32 u2 = __builtin_amdgcn_perm(hi[3], hi[2], 0x05010400u), u3 = __builtin_amdgcn_perm(hi[3], hi[2], 0x07030602u);
        u32 pl[NPL];
        pl[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u); pl[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
        pl[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u); pl[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
        pl[4] = __builtin_amdgcn_perm(u2, t2, 0x05040100u); pl[5] = __builtin_amdgcn_perm(u2, t2, 0x07060302u);
        pl[6] = __builtin_amdgcn_perm(u3, t3, 0x05040100u);
#pragma unroll
        for (int l = 0; l < NPL; l++) *reinterpret_cast<u32 *>(sp + l * pstride) = pl[l];
    } else {
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
            // canonical
            if (f0 + reg < a.F) a.ys[(((size_t)slot * a.B + b) * a.F + f0 + reg) * (2 * a.P) + mm] = (u64)(cv[reg] + ((cv[reg] >> 63) & (long long)q));
    }
}
// the staged limb result of image b leaves as one contiguous block (after a workgroup barrier): the staging area IS the image's byte layout, for either consumer
__device__ __forceinline__ void conv1_copy_out(const Conv1Args &a, const i8 *stage, int slot, int b)
{
    i8 *dst = a.xl_out + ((size_t)slot * a.Bout + a.b0 + b) * a.out_img_bytes;
    for (unsigned o = threadIdx.x * 16; o < a.out_img_bytes; o += blockDim.x * 16)
        *reinterpret_cast<uint4 *>(dst + o) = *reinterpret_cast<const uint4 *>(stage + o);
}

__global__ void __launch_bounds__(768) mfma_conv1_kernel(Conv1Args a)
{
    extern __shared__ __attribute__((aligned(16))) i8 lds[];                  // [2 image buffers][output staging]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.x, i = slot / a.n, s = slot % a.n;
    const u64 q = a.mods[i].q;
    const u32 qbits = a.qbits[i], qfold = a.qfold[i];
    // wave roles.  Usually wave w takes filter group w & 1 and row tiles w >> 1, w >> 1 + waves / 2, ...  With a NARROW second group (a.narrow) its waves cost
    // less than half of the others', and waves w, w + 4, w + 8 share a SIMD: groups alternate in blocks of four waves so that every SIMD hosts both kinds
    const int g = lane >> 4, r16 = lane & 15;
    const bool narrow = a.narrow != 0;
    const int nt = narrow ? (wave >> 2) & 1 : wave & 1;
    const int tile0 = !narrow ? wave >> 1 : nt ? wave - 4 : (wave < 4 ? wave : wave - 4), tile_step = !narrow ? nwaves >> 1 : nt ? 4 : nwaves - 4;
    const bool nar = narrow && nt;                          // this wave runs the packed form
    // operand A of the MFMA = the weights: this lane's filter nt * 16 + r16, K group g (window rows 2g, 2g+1): resident for the whole workgroup
    v4i wv[NPL];
    {
        const i8 *ws = a.wl + (size_t)slot * (NPL * 32 * 64) + (nt * 16 + r16) * 64 + g * 16;
        if (!nar) {
#pragma unroll
            for (int l = 0; l < NPL; l++) wv[l] = *reinterpret_cast<const v4i *>(ws + l * (32 * 64));
        } else {
            // packed A operand: row r16 = 4 f + m <-> filter 16 + f, weight limb 4 grp + m (grp = 0, 1: wv[0], wv[1]; limb 7 does not exist: zero rows)
            const i8 *wp = a.wl + (size_t)slot * (NPL * 32 * 64) + (16 + (r16 >> 2)) * 64 + g * 16;
#pragma unroll
            for (int grp = 0; grp < 2; grp++) {
                const int pl = 4 * grp + (r16 & 3);
                wv[grp] = pl < NPL ? *reinterpret_cast<const v4i *>(wp + pl * (32 * 64)) : v4i{0, 0, 0, 0};
            }
#pragma unroll
            for (int l = 2; l < NPL; l++) wv[l] = v4i{0, 0, 0, 0};
        }
    }
    // the accumulators start at zero (an inline constant of the MFMAs); the per-diagonal biases join pair by pair in the reduction (limbred.h)
    u32 PB[7];
#pragma unroll
    for (int j = 0; j < 6; j++) PB[j] = (u32)a.acc0[i][2 * j] + ((u32)a.acc0[i][2 * j + 1] << 8);
    PB[6] = (u32)a.acc0[i][12];
    // output pixel -> (row, column) of the output map with one multiply: p < 1024, yo <= 32, so (p rcp) >> 16 is exact
    const u32 rcp_yo = (65536u + (u32)a.yo - 1) / (u32)a.yo;
    // C/D layout of a 16 x 16 tile: col = lane & 15, row = 4 (lane >> 4) + reg.  With the weights as A the ROW is the filter and the COLUMN the output row:
    // this lane owns output row (pixel, poly) r16 of every tile and filters f0 .. f0 + 3, four consecutive channels of the next layer.  Rows alternate poly 0 /
    // poly 1 and tiles start at multiples of 16, so a lane's poly is lane & 1 for good: the bias (poly 0 only), centred, is a per-lane constant
    const int f0 = nt * 16 + 4 * g;
    long long bvc[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int f = f0 + reg;
        const u64 bv = (a.bias && f < a.F && !(lane & 1)) ? a.bias[((size_t)f * a.k + i) * a.n + s] : 0;
        bvc[reg] = bv > (q >> 1) ? (long long)(bv - q) : (long long)bv;
    }
    // (packed form: the lane's ONE filter is 16 + g)
    long long bvn = 0;
    if (nar) {
        const int f = 16 + g;
        const u64 bv = (a.bias && f < a.F && !(lane & 1)) ? a.bias[((size_t)f * a.k + i) * a.n + s] : 0;
        bvn = bv > (q >> 1) ? (long long)(bv - q) : (long long)bv;
    }
    i8 *stage = lds + 2 * (size_t)a.img_stride;
    const i8 *ximg = a.xr + (size_t)slot * a.B * a.img_stride;
    const int pieces = a.img_stride / 1024;
    auto issue_img = [&](int b) {
        i8 *dst = lds + (b & 1) * (size_t)a.img_stride;
        const i8 *src = ximg + (size_t)b * a.img_stride + lane * 16;
        for (int pc = wave; pc < pieces; pc += nwaves)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + pc * 1024),
                (__attribute__((address_space(3))) void *)(dst + pc * 1024), 16, 0, 0);
    };
    // (flat limb result: the bytes between the last position and the image's 16-byte end leave with every image -- zero, like the tensor the pack kernel makes)
    if (a.xl_out && a.out_zdc && threadIdx.x < 16) { const unsigned e = a.out_img_bytes - 16 + threadIdx.x;
        if (e >= (unsigned)(NPL * 2 * a.P * a.out_zdc)) stage[e] = 0; }
    issue_img(0);
    const int chan_bytes = a.out_zdc ? a.out_zdc : 32;          // channel bytes per (pixel, poly) position of a limb result
    const unsigned pstride = conv1_stage_plane_stride(a.P, a.out_zdc);
    for (int b = 0; b < a.B; b++) {
        // this wave's pieces of image b have landed (and its stores of image b-1's staging copy have left) ...
        __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));
        __syncthreads();                                          // ... everybody's; the other image buffer and the staging area are free
        if (b + 1 < a.B) issue_img(b + 1);
        const i8 *img = lds + (b & 1) * (size_t)a.img_stride;
        for (int mt = tile0; mt < a.mtiles; mt += tile_step) {
            v4i acc[13];
#pragma unroll
            for (int d = 0; d < 13; d++) acc[d] = v4i{0, 0, 0, 0};
            // operand B = this lane's output row: pixel p, poly c (rows past 2P re-read the last one and are never stored)
            const int mm = mt * 16 + r16, mrow = min(mm, 2 * a.P - 1), p = mrow >> 1, c = mrow & 1, ox = (int)(((u32)p * rcp_yo) >> 16), oy = p - ox * a.yo;
            // k = 16 g + j  <->  window row kx = 2 g + (j >> 3), window column ky = j & 7: per row the three words around the window's first column, cut to its
            // 8 bytes with a byte alignment (rows clamped, and columns past the window may belong to the next row: their weights are zero)
            const int r0 = min(ox * a.xs + 2 * g, a.xd - 1), r1 = min(ox * a.xs + 2 * g + 1, a.xd - 1);
            const int off = oy * a.ystr, sh = off & 3;
            const i8 *p0 = img + c * a.poly_bytes + (off & ~3) + r0 * 32, *p1 = img + c * a.poly_bytes + (off & ~3) + r1 * 32;
            // image limb plane l of this lane's window rows, cut to the window's 8 bytes
            auto window = [&](int l) {
                const u32 *q0 = reinterpret_cast<const u32 *>(p0 + l * a.plane_bytes), *q1 = reinterpret_cast<const u32 *>(p1 + l * a.plane_bytes);
                const u32 a0 = q0[0], a1 = q0[1], a2 = q0[2], b0 = q1[0], b1 = q1[1], b2 = q1[2];
                return v4i{(int)__builtin_amdgcn_alignbyte(a1, a0, sh), (int)__builtin_amdgcn_alignbyte(a2, a1, sh), (int)__builtin_amdgcn_alignbyte(b1, b0,
                    sh),
                           (int)__builtin_amdgcn_alignbyte(b2, b1, sh)};
            };
            if (nar) {
                // packed second filter group: acc[l] = image limb l x weight limbs 0-3, acc[7 + l] (hi6 for l = 6) x limbs 4-6, of filter 16 + g; register m =
                // limb
                v4i hi6;
#pragma unroll
                for (int l = 0; l < NPL; l++) {
                    const v4i av = window(l);
                    acc[l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[0], av, v4i{0, 0, 0, 0}, 0, 0, 0);
                    if (l < 6) acc[7 + l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[1], av, v4i{0, 0, 0, 0}, 0, 0, 0);
                    else hi6 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[1], av, v4i{0, 0, 0, 0}, 0, 0, 0);
                }
                // the 13 diagonals of this lane's one output: D_d = sum over l + m = d of (image limb l) x (weight limb m); then the same reduction as below
                int D[13];
#pragma unroll
                for (int d = 0; d < 13; d++) {
                    int sum = 0;
#pragma unroll
                    for (int l = 0; l < NPL; l++) {
                        const int m = d - l;
                        if (m < 0 || m >= NPL) continue;
                        sum += m < 4 ? acc[l][m] : (l < 6 ? acc[7 + l][m - 4] : hi6[m - 4]);
                    }
                    D[d] = sum;
                }
                const long long cvn = diag_fold_short_centred(D, q, qbits, qfold, bvn, PB);
                const int f = 16 + g;
                if (mm >= 2 * a.P) continue;
                if (a.xl_out) {
                    if (f >= chan_bytes) continue;
                    const u64 dg = f < a.F ? centred_digit_bytes(cvn) : 0;
                    i8 *sp = stage + conv1_stage_row(mm, a.P, a.out_zdc) + f;
#pragma unroll
                    for (int l = 0; l < NPL; l++) sp[l * pstride] = (i8)(dg >> (8 * l));
                } else if (f < a.F) a.ys[(((size_t)slot * a.B + b) * a.F + f) * (2 * a.P) + mm] = (u64)(cvn + ((cvn >> 63) & (long long)q));
                continue;
            }
#pragma unroll
            for (int l = 0; l < NPL; l++) {
                const v4i av = window(l);
#pragma unroll
                for (int m2 = 0; m2 < NPL; m2++)
                    acc[l + m2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[m2], av, acc[l + m2], 0, 0, 0);
            }
            // epilogue: four consecutive filters of output row mm
            long long cv[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                int D[13];
#pragma unroll
                for (int d = 0; d < 13; d++) D[d] = acc[d][reg];
                // one pass from the diagonals to the centred representative, bias included
                cv[reg] = diag_fold_short_centred(D, q, qbits, qfold, bvc[reg], PB);
            }
            conv1_store4(a, stage + conv1_stage_row(mm, a.P, a.out_zdc) + f0, pstride, cv, mm, f0, chan_bytes, q, slot, b);
        }
        if (a.xl_out) {
            __syncthreads();
            conv1_copy_out(a, stage, slot, b);
        }
    }
}

// ---- pixel-major form: windows of at most 40 taps --------------------------------------------------------------------------------------------------------
// The same layer with the image limb index inside the reduction.  Write a centred image residue as x = sum_l a_l 256^l and let W'_l = centred(w 256^l mod q)
// with balanced digits W'_{l,m}: x w = sum_m 256^m E_m (mod q), E_m = sum over (tap, l) of a_l[tap] W'_{l,m}[tap].  K = (tap, l): a pixel is ONE 8-byte value
// (balanced_digit_bytes: seven digits and a zero byte), the image is [poly][row][column] of pixels, and K group G of an MFMA -- 16 bytes -- is taps 2G and
// 2G + 1 (tap = kx yf + ky): every tap is an aligned 8-byte LDS read, two neighbouring taps at an even column one 16-byte read (always so for an even window
// width at an even column stride: the 6 x 6 stride-2 window of PlainModelTiny), no byte alignment and no per-plane loop.  40 taps = 20 groups = NJ = 5 MFMAs
// per weight-digit plane: 35 per tile instead of 49, 7 accumulators instead of 13, and the value they make is below 2^72: one fold (limbred.h
// diag7_fold_centred) instead of three.  The A operand is 35 resident fragments (140 registers) per wave: 8 waves per workgroup, two per SIMD.
// Weights Wp [slot][7 planes m][NJ][32 filters][4 K groups][2 taps][8: l] (limb_pack_w1_kernel_px).  Wave roles, C layout, staging and copy-out as above.
#define NJ 5
__global__ void __launch_bounds__(512) mfma_conv1_kernel_px(Conv1Args a)
{
    extern __shared__ __attribute__((aligned(16))) i8 lds[];                  // [2 image buffers][output staging]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.x, i = slot / a.n, s = slot % a.n;
    const u64 q = a.mods[i].q;
    const u32 qbits = a.qbits[i], qfold = a.qfold[i];
    const int g = lane >> 4, r16 = lane & 15, nt = wave & 1, tile0 = wave >> 1, tile_step = nwaves >> 1;
    // operand A = the weights: this lane's filter nt * 16 + r16, K group g of each of the NJ steps, every digit plane m: resident for the whole workgroup
    v4i wv[NPL][NJ];
    {
        const i8 *ws = a.wl + (size_t)slot * (NPL * NJ * 32 * 64) + (nt * 16 + r16) * 64 + g * 16;
#pragma unroll
        for (int m = 0; m < NPL; m++)
#pragma unroll
            for (int j = 0; j < NJ; j++) wv[m][j] = *reinterpret_cast<const v4i *>(ws + (m * NJ + j) * (32 * 64));
    }
    u32 PB[4];
#pragma unroll
    for (int j = 0; j < 3; j++) PB[j] = (u32)a.acc7[i][2 * j] + ((u32)a.acc7[i][2 * j + 1] << 8);
    PB[3] = (u32)a.acc7[i][6];
    // this lane's taps of step j, as byte offsets from the window's first pixel: low half tap 2G, high half tap 2G + 1, G = 4j + g (taps past the window meet
    // zero weights: they re-read its last tap, or its last pair)
    u32 toff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int last = a.px_pair ? a.px_taps - 2 : a.px_taps - 1;
        const int t0 = min(2 * (4 * j + g), last), t1 = min(2 * (4 * j + g) + 1, a.px_taps - 1);
        const u32 o0 = (u32)(t0 / a.px_yf) * a.px_rs + (u32)(t0 % a.px_yf) * 8, o1 = (u32)(t1 / a.px_yf) * a.px_rs + (u32)(t1 % a.px_yf) * 8;
        toff[j] = o0 | (o1 << 16);
    }
    const int f0 = nt * 16 + 4 * g;
    long long bvc[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int f = f0 + reg;
        const u64 bv = (a.bias && f < a.F && !(lane & 1)) ? a.bias[((size_t)f * a.k + i) * a.n + s] : 0;
        bvc[reg] = bv > (q >> 1) ? (long long)(bv - q) : (long long)bv;
    }
    i8 *stage = lds + 2 * (size_t)a.img_stride;
    // the row table behind the staging area (conv1_rowtab.h): where a row's window starts and where its digits are staged depends on the row alone, and this
    // workgroup walks the same rows for every image -- one entry per row, filled here.  A tile's entry is read one tile ahead, under the MFMAs of the tile before
    // (behind a wave's last tile comes its first one again, for the next image): read at the head of its own tile, the LDS round trip would stand in front of
    // the window reads with nothing to cover it (two waves per SIMD, in step behind the image barrier).  The entries are an ext_vector_type, not HIP's uint2
    // struct: through a uint2 pointer the compiler cannot tell the table from the LDS-DMA target of the next image and puts an s_waitcnt vmcnt(0) in front of
    // the read, which holds the tile until that image has landed (both together: 26.4 ms per launch against 25.2 without a table)
    const v2u *rowtab = reinterpret_cast<const v2u *>(stage + (a.xl_out ? a.out_img_bytes : 0));
    {
        const Conv1RowGeom geom{a.P, a.yo, a.xs, a.ystr, a.px_rs, a.poly_bytes, a.out_zdc};
        for (int mm = threadIdx.x; mm < a.mtiles * 16; mm += blockDim.x) {
            const Conv1RowEntry e = conv1_row_entry(mm, geom);
            const_cast<v2u *>(rowtab)[mm] = v2u{e.win, e.stg};
        }
    }
    const v2u *rowtab_lane = rowtab + r16;
    __syncthreads();
    v2u row = tile0 < a.mtiles ? rowtab_lane[tile0 * 16] : v2u{0u, 0u};
    i8 *stage_lane = stage + f0;
    const unsigned pstride = conv1_stage_plane_stride(a.P, a.out_zdc);
    const i8 *ximg = a.xr + (size_t)slot * a.B * a.img_stride;
    const int pieces = a.img_stride / 1024;
    auto issue_img = [&](int b) {
        i8 *dst = lds + (b & 1) * (size_t)a.img_stride;
        const i8 *src = ximg + (size_t)b * a.img_stride + lane * 16;
        for (int pc = wave; pc < pieces; pc += nwaves)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + pc * 1024),
                (__attribute__((address_space(3))) void *)(dst + pc * 1024), 16, 0, 0);
    };
    if (a.xl_out && a.out_zdc && threadIdx.x < 16) { const unsigned e = a.out_img_bytes - 16 + threadIdx.x;
        if (e >= (unsigned)(NPL * 2 * a.P * a.out_zdc)) stage[e] = 0; }
    issue_img(0);
    const int chan_bytes = a.out_zdc ? a.out_zdc : 32;
    for (int b = 0; b < a.B; b++) {
        __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));
        __syncthreads();
        if (b + 1 < a.B) issue_img(b + 1);
        const i8 *img = lds + (b & 1) * (size_t)a.img_stride;
        for (int mt = tile0; mt < a.mtiles; mt += tile_step) {
            // operand B = this lane's output row mm (rows past 2P re-read the last one and are never stored): its table entry
            const int mm = mt * 16 + r16;
            const v2u cur = row;
            const i8 *win = img + cur.x;
            v4i bv[NJ];
            if (a.px_pair) {
#pragma unroll
                for (int j = 0; j < NJ; j++) bv[j] = *reinterpret_cast<const v4i *>(win + (toff[j] & 0xffffu));
            } else {
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const uint2 t0 = *reinterpret_cast<const uint2 *>(win + (toff[j] & 0xffffu)), t1 = *reinterpret_cast<const uint2 *>(win + (toff[j] >> 16));
                    bv[j] = v4i{(int)t0.x, (int)t0.y, (int)t1.x, (int)t1.y};
                }
            }
            row = rowtab_lane[(mt + tile_step < a.mtiles ? mt + tile_step : tile0) * 16];
            v4i acc[NPL];
#pragma unroll
            for (int m = 0; m < NPL; m++) acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[m][0], bv[0], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int j = 1; j < NJ; j++)
#pragma unroll
                for (int m = 0; m < NPL; m++) acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[m][j], bv[j], acc[m], 0, 0, 0);
            // epilogue: four consecutive filters of output row mm
            long long cv[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                int E[NPL];
#pragma unroll
                for (int m = 0; m < NPL; m++) E[m] = acc[m][reg];
                cv[reg] = diag7_fold_centred(E, q, qbits, qfold, bvc[reg], PB);
            }
            conv1_store4(a, stage_lane + cur.y, pstride, cv, mm, f0, chan_bytes, q, slot, b);
        }
        if (a.xl_out) {
            __syncthreads();
            conv1_copy_out(a, stage, slot, b);
        }
    }
}

// ---- operand preparation -----------------------------------------------------------------------------------------------------------------
// NTT-form image x [B][xd*yd cts][2][k][n] (one channel; canonical or 28-bit packed) -> Xr [slot][B][plane][poly][row][32 columns] (yd <= 32, zero padded). A
// workgroup = 64 consecutive slots x (image, poly, group of RG rows): thread (slot lane, row q of the group) reads its row's columns -- lanes run over the
// slots, so every load is a coalesced 512-byte segment of one ciphertext row -- and stages the seven planes' 32 bytes in LDS; then the workgroup writes the
// staged block out so that the RG * 32 = 128 contiguous bytes a (slot, plane) owns in Xr leave as ONE full line from eight adjacent lanes.  (Round 2's form --
// every thread storing its own 16-byte pieces, neighbouring lanes 1.6 MB apart -- moved 26 GB at 1.7 TB/s; a forward transform that writes this layout itself
// would have to hold 32 columns of a row at once, 32 polynomials per workgroup: the image layout is slot-major because the convolution's workgroup walks one
// slot's image, the transform's row is slot-minor, and the transpose between them is this pass.)
#define RG 4
#define RSL 32
// (32 slots per workgroup, thread = (slot, row of the group, 16-column half): 28 KiB of staging and five workgroups per CU, so that the loads of one overlap
// the digit arithmetic and the stores of the others -- with 64 slots and two workgroups per CU the three ran one after the other: 2.5 TB/s, the same
// restructuring took the weight pack of kernels_mfma.hip from 1.0 to 3.7 TB/s)
__global__ void __launch_bounds__(256) limb_pack_rows1_kernel(const u64 *x, i8 *xr, const ModParams *mods, int n, int k, int B, int xd, int yd, int packed,
                                                              unsigned img_stride, unsigned plane_bytes, unsigned poly_bytes)
{
    __shared__ __attribute__((aligned(16))) i8 st[RSL * NPL * RG * 32];          // [slot][plane][row of the group][32 columns]
    const int sblocks = n / RSL;
    const int sb = blockIdx.x % (sblocks * k), i = sb / sblocks, s0 = (sb % sblocks) * RSL;
    const int rgs = (xd + RG - 1) / RG;
    size_t r = blockIdx.x / (sblocks * k);                       // (b*2 + c)*rgs + row group
    const int rg = (int)(r % rgs); r /= rgs; const int c = (int)(r % 2); const int b = (int)(r / 2);
    const u64 q = mods[i].q;
    const int lane = threadIdx.x & (RSL - 1), qrow = (threadIdx.x >> 5) & (RG - 1), h = threadIdx.x >> 7, row = rg * RG + qrow;
    {
        u32 pl[NPL][4];
#pragma unroll
        for (int l = 0; l < NPL; l++)
#pragma unroll
            for (int wv = 0; wv < 4; wv++) pl[l][wv] = 0;
        if (row < xd) {
            const u64 *src = x + ((((size_t)b * xd * yd + (size_t)row * yd + h * 16) * 2 + c) * k + i) * (size_t)n + s0 + lane;
#pragma unroll
            for (int colx = 0; colx < 16; colx++)
                if (h * 16 + colx < yd) {
                    u64 v = src[(size_t)colx * 2 * k * n];
                    if (packed) v = (v & 0xffffffffULL) | ((v >> 32) << 28);
                    const u64 dg = balanced_digit_bytes(v, q);         // the 7 balanced digits, one per byte
#pragma unroll
                    for (int l = 0; l < NPL; l++) pl[l][colx >> 2] |= (u32)((dg >> (8 * l)) & 0xff) << (8 * (colx & 3));
                }
        }
        i8 *sp = st + (size_t)lane * (NPL * RG * 32) + qrow * 32 + h * 16;
#pragma unroll
        for (int l = 0; l < NPL; l++) *reinterpret_cast<uint4 *>(sp + l * (RG * 32)) = make_uint4(pl[l][0], pl[l][1], pl[l][2], pl[l][3]);
    }
    __syncthreads();
    // RSL slots x 7 planes runs of RG * 32 bytes, 16 bytes per lane: eight adjacent lanes write one run (rows past xd of a ragged last group are not stored)
    const int pieces_per_run = RG * 2, rows_here = min(RG, xd - rg * RG);
    for (int o = threadIdx.x; o < RSL * NPL * pieces_per_run; o += 256) {
        const int run = o / pieces_per_run, part = o - run * pieces_per_run, sl = run / NPL, l = run - sl * NPL;
        if ((part >> 1) >= rows_here) continue;
        i8 *dst = xr + (((size_t)i * n + s0 + sl) * B + b) * img_stride + (size_t)l * plane_bytes + (size_t)c * poly_bytes + (size_t)(rg * RG) * 32 + part * 16;
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(st + (size_t)run * (RG * 32) + part * 16);
    }
}
// The pixel-major image: Xp [slot][B][poly][row][column], one balanced_digit_bytes value per pixel, rows rs bytes and polys poly_bytes apart.  The same workgroup
// and the same 32-slot transpose through LDS; a thread stages its 16 pixels as they are (no per-byte scatter into planes), and the RG rows a slot owns are one
// contiguous run of RG * rs bytes in Xp.  Staging: [slot][RG rows][rs bytes] + 16 bytes per slot (neighbouring slots on different banks).
// Box (bxf x byf, default 1 x 1): the packed image is the WINDOW SUM of the input at the layer's stride, pixel (r, c) = sum over a < bxf, b < byf of
// x(r + a xs, c + b ys) mod q, xdo x ydo = (xd - (bxf-1) xs) x (yd - (byf-1) ys) pixels -- a sum pool behind the convolution, moved in front of it (the layer is
// shift-equivariant: DESIGN.md section 4.5).  The sum is taken on canonical residues (after the 28-bit unpack) and reduced once (limbred.h sum_reduce16: bxf byf <=
// 9 terms below 2^55).  BOX = true is the DIRECT form: a thread reads every term of its 16 pixels itself -- bxf byf loads per pixel, the same coalesced 256-byte
// segment per (row, column) and 32 slots as without a box, nothing more staged in LDS.  The re-reads are not L1 hits (five workgroups per CU each walk 6 rows x 28
// columns x 256 bytes, more than the 32 KiB L1): 11.9 ms for PlainModelTiny's 2 x 2 box at n = 4096, 128 images, against 5.7-6.0 ms for the 28 x 28 image without
// one.  The launcher takes this form only for a box whose ring does not fit the LDS (boxstage.h box_staged: tall boxes at stride 2-3 on wide images); every
// other box runs limb_pack_box_kernel_px below, which loads every input once (8.7 ms: profiles/conv1_box_staged_ab.txt).
// (BOX = false: no box -- the body every unboxed layer ran before the pass could take one)
template <bool BOX>
__global__ void __launch_bounds__(256) limb_pack_rows1_kernel_px(const u64 *x, i8 *xr, const ModParams *mods, int n, int k, int B, int xd, int yd, int packed,
                                                                 unsigned img_stride, unsigned poly_bytes, unsigned rs, int xdo, int ydo, int bxf, int byf, int xs,
                                                                 int ys)
{
    extern __shared__ __attribute__((aligned(16))) i8 stp[];
    const unsigned sstride = RG * rs + 16;
    const int sblocks = n / RSL;
    const int sb = blockIdx.x % (sblocks * k), i = sb / sblocks, s0 = (sb % sblocks) * RSL;
    const int rgs = (xdo + RG - 1) / RG;
    size_t r = blockIdx.x / (sblocks * k);                       // (b*2 + c)*rgs + row group
    const int rg = (int)(r % rgs); r /= rgs; const int c = (int)(r % 2); const int b = (int)(r / 2);
    const u64 q = mods[i].q;
    const int lane = threadIdx.x & (RSL - 1), qrow = (threadIdx.x >> 5) & (RG - 1), h = threadIdx.x >> 7, row = rg * RG + qrow;
    if (row < xdo) {
        const size_t cs = (size_t)2 * k * n;                         // words between neighbouring columns
        const u64 *src = x + ((((size_t)b * xd * yd + (size_t)row * yd + h * 16) * 2 + c) * k + i) * (size_t)n + s0 + lane;
        u64 *sp = reinterpret_cast<u64 *>(stp + (size_t)lane * sstride + qrow * rs) + h * 16;
        if constexpr (!BOX) {
            // no box (xdo = xd, ydo = yd): a pixel is loaded, cut into digits and staged in one go, as the pass did before it could take a box
#pragma unroll
            for (int colx = 0; colx < 16; colx++) {
                const int col = h * 16 + colx;
                if ((unsigned)col * 8 >= rs) continue;
                u64 dg = 0;                                              // (a column past yd: the padding of an odd width)
                if (col < yd) {
                    u64 v = src[(size_t)colx * cs];
                    if (packed) v = (v & 0xffffffffULL) | ((v >> 32) << 28);
                    dg = balanced_digit_bytes(v, q);
                }
                sp[colx] = dg;
            }
        } else {
            u64 sum[16];
#pragma unroll
            for (int colx = 0; colx < 16; colx++) sum[colx] = 0;
            for (int a = 0; a < bxf; a++)
                for (int bb = 0; bb < byf; bb++) {
                    const u64 *tp = src + ((size_t)a * xs * yd + (size_t)bb * ys) * cs;  // (row + a xs <= xd - 1, column + bb ys <= yd - 1 for column < ydo)
#pragma unroll
                    for (int colx = 0; colx < 16; colx++)
                        if (h * 16 + colx < ydo) {
                            u64 v = tp[(size_t)colx * cs];
                            if (packed) v = (v & 0xffffffffULL) | ((v >> 32) << 28);
                            sum[colx] += v;
                        }
                }
#pragma unroll
            for (int colx = 0; colx < 16; colx++) {
                const int col = h * 16 + colx;
                if ((unsigned)col * 8 >= rs) continue;
                // (a column past ydo: the padding of an odd width)
                sp[colx] = col < ydo ? balanced_digit_bytes(sum_reduce16(sum[colx], q), q) : 0;
            }
        }
    }
    __syncthreads();
    // RSL runs of RG * rs bytes, 16 bytes per lane (rows past xdo of a ragged last group are not stored)
    const int per_run = RG * rs / 16, valid = min(RG, xdo - rg * RG) * (int)rs / 16;
    for (int o = threadIdx.x; o < RSL * per_run; o += 256) {
        const int sl = o / per_run, part = o - sl * per_run;
        if (part >= valid) continue;
        i8 *dst = xr + (((size_t)i * n + s0 + sl) * B + b) * img_stride + (size_t)c * poly_bytes + (size_t)(rg * RG) * rs + part * 16;
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(stp + (size_t)sl * sstride + part * 16);
    }
}
// The staged box (boxstage.h has the index arithmetic, tests/cpp/box_stage_check.cpp walks it on the CPU): the same image, byte for byte, with every input
// residue loaded from global memory ONCE per walk.  A workgroup = 32 slots x (modulus, image, poly) x a walk of row groups (gridDim.x decides: one group per
// workgroup, or the whole image).  Per group: (1) the 256 threads = 8 segment rows of 32 slots load the input pixels that are new -- BOX_LD independent loads
// per thread in flight, each the coalesced 256-byte segment of (row, column, 32 slots) -- unpack them and put the canonical residues into the ring
// [pixel mod ring_px][slot]; barrier; (2) thread (slot, row of the group, 16-column half) sums the bxf byf terms of its 16 pixels from the ring, reduces once,
// cuts digits and stages them as the unboxed pass does; barrier; (3) the 32-slot transpose and the 16-byte stores of the unboxed pass.  The next group's loads
// overwrite only rows this group's sums (before the second barrier) were the last to need, and its staging follows its own first barrier, after these stores.
#define BOX_LD 16
static_assert(CONV1_NPL == NPL, "conv1_rowtab.h describes these kernels' digit planes");
static_assert(BOX_RG == RG && BOX_RSL == RSL, "boxstage.h describes this pack's workgroup");
__global__ void __launch_bounds__(256) limb_pack_box_kernel_px(const u64 *x, i8 *xr, const ModParams *mods, int n, int k, int B, int xd, int yd, int packed,
                                                               unsigned img_stride, unsigned poly_bytes, unsigned rs, int xdo, int ydo, int bxf, int byf, int xs,
                                                               int ys)
{
    extern __shared__ __attribute__((aligned(16))) i8 stp[];
    u64 *ring = reinterpret_cast<u64 *>(stp);
    i8 *dig = stp + box_ring_bytes(yd, bxf, xs);
    const unsigned sstride = RG * rs + 16;
    const int sblocks = n / RSL;
    const int sb = blockIdx.x % (sblocks * k), i = sb / sblocks, s0 = (sb % sblocks) * RSL;
    const int wpi = (int)(gridDim.x / (unsigned)(sblocks * k * 2 * B));                // workgroups per (image, poly)
    size_t r = blockIdx.x / (sblocks * k);                       // (b*2 + c)*wpi + walk
    const int w = (int)(r % wpi); r /= wpi; const int c = (int)(r % 2); const int b = (int)(r / 2);
    const u64 q = mods[i].q;
    const int lane = threadIdx.x & (RSL - 1), seg = threadIdx.x >> 5, qrow = seg & (RG - 1), h = threadIdx.x >> 7;
    const u32 ring_px = box_ring_px(yd, bxf, xs);
    const size_t cs = (size_t)2 * k * n;                             // words between neighbouring pixels of a row, and between a row's last and the next row's first
    const u64 *src = x + (((size_t)b * xd * yd * 2 + c) * k + i) * (size_t)n + s0 + lane;
    const int g0 = box_walk_first(w, xdo, wpi), g1 = box_walk_end(w, xdo, wpi);
    for (int g = g0; g < g1; g++) {
        const int p1 = box_load_end(g, xd, yd, bxf, xs);
        for (int pb = box_load_first(g, g == g0, xd, yd, bxf, xs) + seg; pb < p1; pb += 8 * BOX_LD) {
            u64 v[BOX_LD];
#pragma unroll
            for (int u = 0; u < BOX_LD; u++) v[u] = pb + 8 * u < p1 ? src[(size_t)(pb + 8 * u) * cs] : 0;
#pragma unroll
            for (int u = 0; u < BOX_LD; u++)
                if (pb + 8 * u < p1) {
                    u64 t = v[u];
                    if (packed) t = (t & 0xffffffffULL) | ((t >> 32) << 28);
                    ring[box_cell((u32)(pb + 8 * u), ring_px, lane)] = t;
                }
        }
        __syncthreads();
        const int row = g * RG + qrow;
        if (row < xdo) {
            u64 sum[16];
#pragma unroll
            for (int colx = 0; colx < 16; colx++) sum[colx] = 0;
            for (int a = 0; a < bxf; a++)
                for (int bb = 0; bb < byf; bb++) {
                    u32 pos = box_ring_pos(box_term_px(row, box_col(h, 0), a, bb, xs, ys, yd), ring_px);
#pragma unroll
                    for (int colx = 0; colx < 16; colx++) {
                        if (box_col(h, colx) < ydo) sum[colx] += ring[box_pos_cell(pos, lane)];
                        pos = box_ring_step(pos, 1, ring_px);
                    }
                }
            u64 *sp = reinterpret_cast<u64 *>(dig + (size_t)lane * sstride + qrow * rs) + h * 16;
#pragma unroll
            for (int colx = 0; colx < 16; colx++) {
                const int col = box_col(h, colx);
                if ((unsigned)col * 8 >= rs) continue;
                // (a column past ydo: the padding of an odd width)
                sp[colx] = col < ydo ? balanced_digit_bytes(sum_reduce16(sum[colx], q), q) : 0;
            }
        }
        __syncthreads();
        // RSL runs of RG * rs bytes, 16 bytes per lane (rows past xdo of a ragged last group are not stored)
        const int per_run = RG * rs / 16, valid = box_rows_here(g, xdo) * (int)rs / 16;
        for (int o = threadIdx.x; o < RSL * per_run; o += 256) {
            const int sl = o / per_run, part = o - sl * per_run;
            if (part >= valid) continue;
            i8 *dst = xr + (((size_t)i * n + s0 + sl) * B + b) * img_stride + (size_t)c * poly_bytes + (size_t)(g * RG) * rs + part * 16;
            *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(dig + (size_t)sl * sstride + part * 16);
        }
    }
}
// NTT-form weights w [F][1][xf][yf][k][n] -> Wl1 [slot][7 planes][32 filters][64 taps], tap = kx*8 + ky (pre-zeroed).  (No 2^64 factor since round 4: the
// kernel's reduction folds, it no longer divides by 2^64.)
__global__ void __launch_bounds__(64) limb_pack_w1_kernel(const u64 *w, i8 *wl, const ModParams *mods, int n, int k, int F, int xf, int yf)
{
    const int sblocks = n / 64;
    const int sb = blockIdx.x % (sblocks * k), i = sb / sblocks, s = (sb % sblocks) * 64 + threadIdx.x;
    size_t r = blockIdx.x / (sblocks * k);                       // (f*xf + kx)*yf + ky
    const int ky = (int)(r % yf); r /= yf; const int kx = (int)(r % xf); const int f = (int)(r / xf);
    const ModParams m = mods[i];
    int d[NPL]; limb_digits1(w[((((size_t)f * xf + kx) * yf + ky) * k + i) * (size_t)n + s], m.q, d);
    i8 *dst = wl + ((size_t)i * n + s) * (NPL * 32 * 64) + f * 64 + kx * 8 + ky;
#pragma unroll
    for (int l = 0; l < NPL; l++) dst[(size_t)l * (32 * 64)] = (i8)d[l];
}

// The pixel-major form's weights: Wp [slot][7 digit planes m][NJ steps][32 filters][4 K groups][2 taps][8: image limb l] (pre-zeroed), tap = kx*yf + ky = 8 step +
// 2 group + half: byte l of a tap is digit m of W'_l = centred(w 256^l mod q) -- one mulmod by 256 per image limb, then the digits.
__global__ void __launch_bounds__(64) limb_pack_w1_kernel_px(const u64 *w, i8 *wl, const ModParams *mods, int n, int k, int F, int xf, int yf)
{
    const int sblocks = n / 64;
    const int sb = blockIdx.x % (sblocks * k), i = sb / sblocks, s = (sb % sblocks) * 64 + threadIdx.x;
    size_t r = blockIdx.x / (sblocks * k);                       // (f*xf + kx)*yf + ky
    const int ky = (int)(r % yf); r /= yf; const int kx = (int)(r % xf); const int f = (int)(r / xf);
    const ModParams m = mods[i];
    u64 v = w[((((size_t)f * xf + kx) * yf + ky) * k + i) * (size_t)n + s];
    const int tap = kx * yf + ky, G = tap >> 1;
    i8 *dst = wl + ((size_t)i * n + s) * (NPL * NJ * 32 * 64) + ((G >> 2) * 32 + f) * 64 + (G & 3) * 16 + (tap & 1) * 8;
    for (int l = 0; l < NPL; l++) {
        int d[NPL]; limb_digits1(v, m.q, d);
#pragma unroll
        for (int dm = 0; dm < NPL; dm++) dst[(size_t)dm * (NJ * 32 * 64) + l] = (i8)d[dm];
        v = mulmod(v, 256, m);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
// per (slot, image): 7 planes x 2 polys x (xd rows + 1) x 32 bytes: the extra row puts the two polys' blocks 8 LDS banks apart (xd = 28: 896-byte blocks would
// be 224 dwords = 0 banks apart, and the window reads of a pixel's two polys -- neighbouring lanes -- a two-way conflict each); it also takes the last window's
// read-ahead
static inline unsigned conv1_poly_bytes(int xd) { return ((unsigned)xd + 1) * 32; }
static inline unsigned conv1_img_stride(int xd) { const unsigned b = NPL * 2 * conv1_poly_bytes(xd); return (b + 1023) / 1024 * 1024; }
// pixel-major form: rows of yd 8-byte pixels rounded up to 16 bytes; the second poly's block starts 128 bytes (mod 256) past the first one's, so that the eight
// pixels x two polys that one LDS cycle of a 16-byte window read serves cover the 64 banks once (28 x 28: 224-byte rows, 6272-byte blocks, no padding at all)
static inline unsigned conv1_px_rs(int yd) { return ((unsigned)yd * 8 + 15) / 16 * 16; }
static inline unsigned conv1_px_poly_bytes(int xd, int yd) { const unsigned b = (unsigned)xd * conv1_px_rs(yd); return b + (128 + 256 - b % 256) % 256; }
static inline unsigned conv1_px_img_stride(int xd, int yd) { return (2 * conv1_px_poly_bytes(xd, yd) + 1023) / 1024 * 1024; }
static bool conv1_fits(unsigned img_stride, const Window &w, bool px)
{
    // two image buffers + the staging area of a limb result (at most 32 channel bytes per position) + the pixel-major form's row table (conv1_rowtab.h) must fit
    // the 160 KiB of LDS
    return 2 * (size_t)img_stride + (size_t)NPL * w.xo() * w.yo() * 2 * 32 + (px ? conv1_rowtab_bytes(w.xo() * w.yo()) : 0) <= 160 * 1024;
}
// Which form a layer runs: 1 plane-major (mfma_conv1_kernel), 2 pixel-major (mfma_conv1_kernel_px).  Decided by the tuning switch, the window and the filter
// count ALONE, so that the weights (packed without knowing the image) and every later launch agree; conv1_narrow does not enter (the tests flip it between
// launches on one set of weights).  Pixel-major takes windows of at most 8 NJ = 40 taps and moduli within conv1_fold7_ok; a forced form the layer cannot take
// falls back to the other one.  Auto: pixel-major wherever it applies except for 17-20 filters, whose second filter group has the packed plane-major form
// (DESIGN.md section 4.2 has the measurements).
int k_limb_conv1_form(const crc_ctx *c, int xf, int yf, int nf)
{
    bool px = xf * yf <= 8 * NJ;
    for (int i = 0; i < c->k && px; i++) px = conv1_fold7_ok(c->tabs[i].m.q, c->tabs[i].m.bits, fold_constant(c->tabs[i].m.q, c->tabs[i].m.bits));
    const int forced = c->tune.conv1_form;
    if (forced == 1 || !px) return 1;
    if (forced == 2) return 2;
    return nf > 16 && nf <= 20 ? 1 : 2;
}
bool k_limb_conv1_shape(const crc_ctx *c, const LayerShape &s)
{
    const int xd = s.w.xd, yd = s.w.yd, xf = s.w.xf, yf = s.w.yf, nf = s.nf;
    if (s.zd != 1 || xf > 8 || yf > 8 || nf > 32 || yd > 32 || c->n < 64 || c->k > MAXK) return false;
    // the epilogue's bounds: the folding reduction wants q = 2^b - f with 53 <= b <= 55 and a small f (limbred.h conv1_fold_ok); 7 balanced digits with |top
    // digit| <= 64 need q < 2^55
    for (int i = 0; i < c->k; i++) if (!conv1_fold_ok(c->tabs[i].m.q, c->tabs[i].m.bits, fold_constant(c->tabs[i].m.q, c->tabs[i].m.bits))) return false;
    if (s.w.P() > 1024) return false;                              // (the kernel's reciprocal division of a pixel index by yo <= 32 is exact below 2048)
    // (the pixel-major image is the smaller one up to 28 columns; wider than that it can be up to 14 % larger)
    const bool px = k_limb_conv1_form(c, xf, yf, nf) == 2;
    return conv1_fits(px ? conv1_px_img_stride(xd, yd) : conv1_img_stride(xd), s.w, px);
}
// A box (input-side window sum, limb_pack_rows1_kernel_px) in front of a layer with base window xf x yf: the pixel-major form only, at most 9 terms (sum_reduce16's
// bound with room to spare), and the SUMMED image must be a shape the kernel takes
bool k_limb_conv1_box_shape(const crc_ctx *c, const LayerShape &s, int bxf, int byf)
{
    if (bxf < 1 || byf < 1 || bxf * byf > 9) return false;
    const LayerShape sum{s.w.boxed(bxf, byf), s.zd, s.nf};
    if (sum.w.xd < sum.w.xf || sum.w.yd < sum.w.yf || !k_limb_conv1_shape(c, sum)) return false;
    return bxf * byf == 1 || k_limb_conv1_form(c, s.w.xf, s.w.yf, s.nf) == 2;
}
static size_t conv1_form_weights_bytes(const crc_ctx *c, int form) { return (size_t)c->n * c->k * NPL * 32 * 64 * (form == 2 ? NJ : 1); }
size_t k_limb_conv1_weights_bytes(const crc_ctx *c) { return conv1_form_weights_bytes(c, 2); }            // enough for either form
size_t k_limb_conv1_weights_bytes_for(const crc_ctx *c, int nf, int xf, int yf) { return conv1_form_weights_bytes(c, k_limb_conv1_form(c, xf, yf, nf)); }
size_t k_limb_conv1_image_bytes(const crc_ctx *c, int B, const Window &w, int nf)
{
    return (size_t)c->n * c->k * B * (k_limb_conv1_form(c, w.xf, w.yf, nf) == 2 ? conv1_px_img_stride(w.xd, w.yd) : conv1_img_stride(w.xd));
}

static void conv1_tables(const crc_ctx *c, Conv1Args &a)      // limbred.h: accumulator biases and q^-1 mod 2^64 per modulus
{
    for (int i = 0; i < c->k; i++) { conv1_bias_table(c->tabs[i].m.q, a.acc0[i]); conv1_bias7_table(c->tabs[i].m.q, a.acc7[i]); a.qbits[i] = c->tabs[i].m.bits;
        a.qfold[i] = fold_constant(c->tabs[i].m.q, c->tabs[i].m.bits); }
}

int k_limb_conv1_pack_weights(crc_ctx *c, const u64 *w, i8 *wl, int nf, int xf, int yf, hipStream_t st)
{
    const int form = k_limb_conv1_form(c, xf, yf, nf);
    HIPCHK(hipMemsetAsync(wl, 0, conv1_form_weights_bytes(c, form), st));
    const size_t blocks = (size_t)(c->n / 64) * c->k * nf * xf * yf;
    if (form == 2) hipLaunchKernelGGL(limb_pack_w1_kernel_px, dim3((unsigned)blocks), dim3(64), 0, st, w, wl, c->d_mods, c->n, c->k, nf, xf, yf);
    else hipLaunchKernelGGL(limb_pack_w1_kernel, dim3((unsigned)blocks), dim3(64), 0, st, w, wl, c->d_mods, c->n, c->k, nf, xf, yf);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
// x: B NTT-form one-channel images of in.xd x in.yd pixels; the convolution reads their bxf x byf window sums at its own stride (xd x yd pixels below; no box: the
// images themselves); xr: k_limb_conv1_image_bytes of scratch for that xd x yd image; result either images b0 .. b0 + B of a limb tensor of Bout images (xl_out,
// [slot][Bout][7][P][2][32]) or slot-major u64 (ys, [slot][B][F][P][2])
int k_limb_conv1(crc_ctx *c, const u64 *x, bool packed, i8 *xr, const i8 *wl, u64 *ys, i8 *xl_out, int Bout, int b0, const u64 *bias_ntt, int B, const Window &in,
                 int nf, hipStream_t st, int bxf, int byf)
{
    if (B == 0) return CRC_OK;
    if (!k_limb_conv1_box_shape(c, {in, 1, nf}, bxf, byf)) return CRC_ERR_UNSUPPORTED;
    const Window w = in.boxed(bxf, byf);
    const int xd = w.xd, yd = w.yd, xs = w.xs, xf = w.xf, yf = w.yf, xd_in = in.xd, yd_in = in.yd;
    const int form = k_limb_conv1_form(c, xf, yf, nf);
    Conv1Args a{};
    a.xr = xr; a.wl = wl; a.ys = ys; a.xl_out = xl_out; a.mods = c->d_mods; a.bias = bias_ntt;
    a.n = c->n; a.k = c->k; a.B = B; a.Bout = Bout; a.b0 = b0; a.xd = xd; a.yo = w.yo(); a.xs = xs; a.ystr = w.ys; a.P = w.P(); a.F = nf;
        a.mtiles = (2 * a.P + 15) / 16;
    // (the limb tensor of the convolution behind: its layout follows ITS channel count = this layer's filters)
    a.out_zdc = a.P > 1 ? k_limb_flat_zdc(nf) : 0;
    a.out_img_bytes = conv1_stage_bytes(a.P, a.out_zdc);
    conv1_tables(c, a);
    const size_t pack_blocks = (size_t)(c->n / RSL) * c->k * B * 2 * ((xd + RG - 1) / RG);
    if (pack_blocks > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    if (form == 2) {
        a.px_rs = conv1_px_rs(yd); a.poly_bytes = conv1_px_poly_bytes(xd, yd); a.img_stride = conv1_px_img_stride(xd, yd);
        a.px_taps = xf * yf; a.px_yf = yf;
        a.px_pair = yf % 2 == 0 && w.ys % 2 == 0 ? 1 : 0;
        if (bxf * byf > 1 && box_staged(yd_in, bxf, xs, a.px_rs)) {
            // the staged box, one workgroup per (32 slots, modulus, image, poly) walking the whole image: every input residue is loaded once
            const size_t lds = box_lds_bytes(yd_in, bxf, xs, a.px_rs);
            const int wpi = 1;                                          // (box_row_groups(xd): one row group per workgroup, the halo read 1.5 x: 10.2 ms against 8.7)
            { const int rc = crc_ctx_ensure_lds(c, (const void *)limb_pack_box_kernel_px, lds); if (rc) return rc; }
            hipLaunchKernelGGL(limb_pack_box_kernel_px, dim3((unsigned)((size_t)(c->n / RSL) * c->k * B * 2 * wpi)), dim3(256), lds, st, x, xr, c->d_mods, c->n,
                c->k, B, xd_in, yd_in, packed ? 1 : 0, a.img_stride, a.poly_bytes, a.px_rs, xd, yd, bxf, byf, xs, w.ys);
        } else if (bxf * byf > 1)                                   // a ring past the LDS of a CU (a 9 x 1 box at stride 3 on a wide image): every term read directly
            hipLaunchKernelGGL(limb_pack_rows1_kernel_px<true>, dim3((unsigned)pack_blocks), dim3(256), RSL * (RG * a.px_rs + 16), st, x, xr, c->d_mods, c->n, c->k,
                B, xd_in, yd_in, packed ? 1 : 0, a.img_stride, a.poly_bytes, a.px_rs, xd, yd, bxf, byf, xs, w.ys);
        else
            hipLaunchKernelGGL(limb_pack_rows1_kernel_px<false>, dim3((unsigned)pack_blocks), dim3(256), RSL * (RG * a.px_rs + 16), st, x, xr, c->d_mods, c->n, c->k,
                B, xd_in, yd_in, packed ? 1 : 0, a.img_stride, a.poly_bytes, a.px_rs, xd, yd, 1, 1, xs, w.ys);
        HIPCHK(hipGetLastError());
        // (140 registers of resident weights: two waves per SIMD, whatever conv1_waves asks for)
        const size_t lds = 2 * (size_t)a.img_stride + (xl_out ? a.out_img_bytes : 0) + conv1_rowtab_bytes(a.P);
        { const int rc = crc_ctx_ensure_lds(c, (const void *)mfma_conv1_kernel_px, lds); if (rc) return rc; }
        hipLaunchKernelGGL(mfma_conv1_kernel_px, dim3((unsigned)(c->n * c->k)), dim3(64 * 8), lds, st, a);
        HIPCHK(hipGetLastError());
        return CRC_OK;
    }
    a.poly_bytes = conv1_poly_bytes(xd); a.plane_bytes = 2 * a.poly_bytes; a.img_stride = conv1_img_stride(xd);
    a.narrow = c->tune.conv1_narrow != 0 && nf > 16 && nf <= 20 ? 1 : 0;
    {
        hipLaunchKernelGGL(limb_pack_rows1_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, st, x, xr, c->d_mods, c->n, c->k, B, xd, yd, packed ? 1 : 0,
            a.img_stride, a.plane_bytes, a.poly_bytes);
        HIPCHK(hipGetLastError());
    }
    // waves per workgroup (8 or 12; wave w runs on SIMD w % 4 and takes row tiles w/2, w/2 + waves/2, ...): the count that loads the busiest SIMD least, 12 on
    // a tie (a third wave per SIMD hides more of the epilogue behind the other waves' MFMAs)
    auto busiest = [&](int nw) {
        int load[4] = {0, 0, 0, 0}, worst = 0;
        for (int w = 0; w < nw; w++) load[w & 3] += (a.mtiles - (w >> 1) + nw / 2 - 1) / (nw / 2);
        for (int sd = 0; sd < 4; sd++) worst = load[sd] > worst ? load[sd] : worst;
        return worst;
    };
    const int forced = c->tune.conv1_waves;     // tuning (tools/)
    // (narrow second group: four of its waves + four or eight of the others, one or two heavy waves and one light wave per SIMD either way: 12, for the
    // overlap)
    const int nwaves = forced ? forced : a.narrow ? 12 : busiest(12) <= busiest(8) ? 12 : 8;
    const size_t lds = 2 * (size_t)a.img_stride + (xl_out ? a.out_img_bytes : 0);
    { const int rc = crc_ctx_ensure_lds(c, (const void *)mfma_conv1_kernel, lds); if (rc) return rc; }
    hipLaunchKernelGGL(mfma_conv1_kernel, dim3((unsigned)(c->n * c->k)), dim3(64 * nwaves), lds, st, a);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
