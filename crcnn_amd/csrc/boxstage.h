// boxstage.h -- the index arithmetic of the staged box of the pixel-major image pack (kernels_mfma1.hip limb_pack_box_kernel_px); host + device, so that
// tests/cpp/box_stage_check.cpp can walk the very same code over every shape on the CPU.
//
// The pack writes the bxf x byf window sums of an xd x yd input at the layer's stride (xs, ys): pixel (r, c) = sum over a < bxf, b < byf of x(r + a xs, c + b ys),
// xdo x ydo = (xd - (bxf-1) xs) x (yd - (byf-1) ys) pixels.  A workgroup = 32 slots x (modulus, image, poly) walks some of the row groups (BOX_RG output rows
// each) top to bottom.  Group g needs the input rows g RG .. g RG + RG + halo - 1, halo = (bxf-1) xs: ring_rows = RG + halo consecutive rows, whole rows, so
// ring_rows yd consecutive PIXELS p = row yd + column.  They live in a ring of ring_px = ring_rows yd cells, pixel p in cell p mod ring_px, 32 slots of 8 bytes
// per cell (a cell is the 256-byte segment one load instruction of 32 lanes fetches: LDS writes and reads both run over the slots, all 64 banks once).  The first
// group of a walk loads its whole window; every later group loads the RG rows that are new and overwrites exactly the RG rows nobody needs any more.  A term
// of an output pixel is then one 8-byte LDS read.
#pragma once
#include "modarith.h"

#define BOX_RG 4                        // output rows per group (= RG of the pack)
#define BOX_RSL 32                      // slots per workgroup (= RSL)
#define BOX_LDS_MAX (160 * 1024)        // the LDS of one CU: a box whose ring and digit staging do not fit is read directly (limb_pack_rows1_kernel_px<true>)

CRC_HD int box_halo(int bxf, int xs) { return (bxf - 1) * xs; }
CRC_HD int box_ring_rows(int bxf, int xs) { return BOX_RG + box_halo(bxf, xs); }
CRC_HD u32 box_ring_px(int yd, int bxf, int xs) { return (u32)box_ring_rows(bxf, xs) * (u32)yd; }
CRC_HD size_t box_ring_bytes(int yd, int bxf, int xs) { return (size_t)box_ring_px(yd, bxf, xs) * BOX_RSL * 8; }
// the digit staging behind the ring: [slot][RG rows][rs bytes] + 16 bytes per slot, as without a box
CRC_HD size_t box_digit_bytes(unsigned rs) { return (size_t)BOX_RSL * (BOX_RG * rs + 16); }
CRC_HD size_t box_lds_bytes(int yd, int bxf, int xs, unsigned rs) { return box_ring_bytes(yd, bxf, xs) + box_digit_bytes(rs); }
CRC_HD bool box_staged(int yd, int bxf, int xs, unsigned rs) { return box_lds_bytes(yd, bxf, xs, rs) <= BOX_LDS_MAX; }

CRC_HD int box_row_groups(int xdo) { return (xdo + BOX_RG - 1) / BOX_RG; }
CRC_HD int box_rows_here(int g, int xdo) { return xdo - g * BOX_RG < BOX_RG ? xdo - g * BOX_RG : BOX_RG; }       // (the ragged last group)
// the walk of workgroup w out of wpi per (image, poly): groups [first, end), wpi = row groups: one group each; wpi = 1: the whole image
CRC_HD int box_groups_per_wg(int xdo, int wpi) { return (box_row_groups(xdo) + wpi - 1) / wpi; }
CRC_HD int box_walk_first(int w, int xdo, int wpi) { return w * box_groups_per_wg(xdo, wpi); }
CRC_HD int box_walk_end(int w, int xdo, int wpi)
{
    const int e = (w + 1) * box_groups_per_wg(xdo, wpi), rgs = box_row_groups(xdo);
    return e < rgs ? e : rgs;
}
// the input pixels [first, end) group g loads: its whole window at the start of a walk, the RG new rows after that; never past the image
CRC_HD int box_load_end(int g, int xd, int yd, int bxf, int xs)
{
    const int r = g * BOX_RG + box_ring_rows(bxf, xs);
    return (r < xd ? r : xd) * yd;
}
CRC_HD int box_load_first(int g, bool walk_start, int xd, int yd, int bxf, int xs)
{
    const int f = (g * BOX_RG + (walk_start ? 0 : box_halo(bxf, xs))) * yd, e = box_load_end(g, xd, yd, bxf, xs);
    return f < e ? f : e;
}
// the LDS word (8 bytes) of (pixel, slot)
CRC_HD u32 box_cell(u32 px, u32 ring_px, int slot) { return (px % ring_px) * BOX_RSL + (u32)slot; }
// a run of neighbouring pixels: the ring position of the first one, then one step at a time (pos < ring_px, step <= ring_px)
CRC_HD u32 box_ring_pos(u32 px, u32 ring_px) { return px % ring_px; }
CRC_HD u32 box_ring_step(u32 pos, u32 step, u32 ring_px) { return pos + step >= ring_px ? pos + step - ring_px : pos + step; }
CRC_HD u32 box_pos_cell(u32 pos, int slot) { return pos * BOX_RSL + (u32)slot; }
// thread (row qrow of the group, 16-column half h) makes the output pixels (g RG + qrow, h 16 + colx), colx < 16; term (a, bb) of pixel (row, col)
CRC_HD int box_col(int h, int colx) { return h * 16 + colx; }
CRC_HD u32 box_term_px(int row, int col, int a, int bb, int xs, int ys, int yd) { return (u32)((row + a * xs) * yd + col + bb * ys); }
