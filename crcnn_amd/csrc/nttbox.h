// nttbox.h -- the index arithmetic of the boxed forward transform (kernels.hip ntt_rows_wave_kernel<.., BOX = true>, k_ntt_ct_box); host + device, so that
// tests/cpp/ntt_box_index_check.cpp can walk the very same code over every shape on the CPU.
//
// The transform reads B images of xd x yd coefficient-form ciphertexts ([B][xd][yd][2][k][n]) and writes the NTT of their bxf x byf window sums at the layer's
// stride (xs, ys): B images of xdo x ydo = (xd - (bxf-1) xs) x (yd - (byf-1) ys) ciphertexts, pixel (r, c) = sum over a < bxf, bb < byf of x(r + a xs, c + bb ys)
// -- the box of limb_pack_rows1_kernel_px (kernels_mfma1.hip), taken in front of the transform instead of behind it (the transform is linear over Z_q).
// One workgroup per output row = (image, pixel, poly, modulus).  Two maps from the block index to that row:
//   order 0  the plain one, block = row;
//   order 1  XCD-grouped (xcd_group / xcd_grid of ntt_device.h / xcd_grid.h, the same arithmetic): a group is one (image, poly, modulus) PLANE, its xdo ydo members
//            are the plane's pixels in raster order, so one XCD walks a plane and the bxf byf users of an input row find it in that XCD's L2.  Blocks past
//            the last plane return at once.
#pragma once
#include <stddef.h>
#include "modarith.h"

struct NttBox { int xd, yd, xdo, ydo, bxf, byf, xs, ys; };
CRC_HD NttBox nttbox_make(int xd, int yd, int bxf, int byf, int xs, int ys) { return {xd, yd, xd - (bxf - 1) * xs, yd - (byf - 1) * ys, bxf, byf, xs, ys}; }
CRC_HD bool nttbox_ok(const NttBox &g) { return g.xd >= 1 && g.yd >= 1 && g.bxf >= 1 && g.byf >= 1 && g.xs >= 1 && g.ys >= 1 && g.xdo >= 1 && g.ydo >= 1; }
#define NTTBOX_MAX_TERMS 9              // sum_reduce16's operand bound with room to spare (limbred.h; tests/cpp/box_sum_check.cpp: 9 (q - 1) for the default moduli)

CRC_HD size_t nttbox_pixels(const NttBox &g) { return (size_t)g.xdo * g.ydo; }
CRC_HD size_t nttbox_planes(size_t B, int k) { return B * 2 * (size_t)k; }
CRC_HD size_t nttbox_rows(size_t B, const NttBox &g, int k) { return nttbox_planes(B, k) * nttbox_pixels(g); }

// output row ((b xdo ydo + r ydo + c) 2 + poly) k + mod.  Rows and blocks of a launch fit 31 bits (the launcher checks): the splits are 32-bit divisions
struct NttBoxRow { u32 b; int r, c, poly, mod; };
CRC_HD size_t nttbox_row_of(const NttBoxRow &o, const NttBox &g, int k)
{
    return ((((size_t)o.b * g.xdo + (size_t)o.r) * g.ydo + (size_t)o.c) * 2 + (size_t)o.poly) * (size_t)k + (size_t)o.mod;
}
// the source row of term (a, bb) of an output row
CRC_HD size_t nttbox_src_row(const NttBoxRow &o, const NttBox &g, int k, int a, int bb)
{
    return ((((size_t)o.b * g.xd + (size_t)(o.r + a * g.xs)) * g.yd + (size_t)(o.c + bb * g.ys)) * 2 + (size_t)o.poly) * (size_t)k + (size_t)o.mod;
}

// blocks of a launch, and block -> output row (false: a block past the last row -- the padding of the grouped order)
CRC_HD size_t nttbox_grid(int order, size_t B, const NttBox &g, int k)
{
    if (order == 0) return nttbox_rows(B, g, k);
    return (nttbox_planes(B, k) + 7) / 8 * 8 * nttbox_pixels(g);               // = xcd_grid(planes, pixels)
}
CRC_HD bool nttbox_block_row(int order, u32 blk, u32 B, const NttBox &g, int k, NttBoxRow &o)
{
    const u32 P = (u32)g.xdo * (u32)g.ydo, planes = B * 2 * (u32)k;
    u32 px, plane;
    if (order == 0) {                       // block = row = (b P + px) 2 k + (poly k + mod)
        const u32 pk = 2 * (u32)k, bp = blk / pk, pm = blk - bp * pk;
        o.b = bp / P; px = bp - o.b * P;
        plane = o.b * pk + pm;
    } else {                                // xcd_group(blk, P, planes): blocks b and b + 8 share an XCD, the members of a group take consecutive slots of it
        const u32 xcd = blk & 7, slot = blk >> 3, sp = slot / P;
        px = slot - sp * P; plane = sp * 8 + xcd;
        o.b = plane / (2 * (u32)k);
    }
    if (plane >= planes) return false;
    const u32 pm = plane - o.b * 2 * (u32)k;
    o.poly = pm >= (u32)k ? 1 : 0; o.mod = (int)(pm - (o.poly ? (u32)k : 0));
    o.r = (int)(px / (u32)g.ydo); o.c = (int)(px - (u32)o.r * (u32)g.ydo);
    return true;
}
