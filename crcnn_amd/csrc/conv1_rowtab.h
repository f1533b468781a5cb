// conv1_rowtab.h -- the per-row addresses of the pixel-major one-channel convolution (kernels_mfma1.hip mfma_conv1_kernel_px) and the layout of the staged limb
// result both forms of the kernel share; host + device, so that tests/cpp/conv1_rowtab_check.cpp can walk the very same code over every shape on the CPU.
//
// An output row mm = 2 pixel + poly of a layer's map (P = xo yo pixels, yo columns) reads its window at a byte offset into the LDS image that depends on the
// row and the geometry alone, and stores its digits at a byte offset into the staging area that depends on the row and the consumer's layout alone: neither
// sees the image, and a workgroup walks the same rows for every image of its slot.  The kernel fills a table of conv1_rowtab_rows(P) entries once per workgroup
// and reads one 8-byte entry per tile and lane.
//
// The staged limb result IS the image's byte layout in the limb tensor, for either consumer:
//   blocked (32 channel bytes per position, zdc = 0)  [plane][row mm][32]:       byte of (row, channel f, plane l) = l 2P 32  + mm 32 + f
//   flat    (zdc channel bytes per position)          [plane][poly][pixel][zdc]: byte of (row, channel f, plane l) = l 2P zdc + ((mm & 1) P + (mm >> 1)) zdc + f
// so the copy-out is one linear copy of conv1_stage_bytes.
#pragma once
#include "modarith.h"

#define CONV1_NPL 7                     // digit planes (= NPL of the kernels)

struct Conv1RowGeom {
    int P, yo, xs, ystr;                // output pixels and columns of the map, the window's row and column stride
    u32 px_rs, poly_bytes;              // pixel-major image: bytes between rows and between the two polys
    int zdc;                            // channel bytes per position of a flat limb result, 0: the blocked one
};
struct Conv1RowEntry { u32 win, stg; }; // byte offsets: the window's first pixel in the image buffer, channel 0 of plane 0 in the staging area

CRC_HD int conv1_rowtab_rows(int P) { return (2 * P + 15) / 16 * 16; }                   // whole 16-row tiles
CRC_HD size_t conv1_rowtab_bytes(int P) { return (size_t)conv1_rowtab_rows(P) * sizeof(Conv1RowEntry); }
// bytes between the digit planes of one (row, channel), and the whole staging area of an image (the flat form rounds up to 16: kernels_mfma.hip)
CRC_HD u32 conv1_stage_plane_stride(int P, int zdc) { return (u32)(2 * P) * (u32)(zdc ? zdc : 32); }
CRC_HD u32 conv1_stage_bytes(int P, int zdc) { return zdc ? (CONV1_NPL * conv1_stage_plane_stride(P, zdc) + 15) / 16 * 16 : CONV1_NPL * conv1_stage_plane_stride(P, 0); }
// staging offset of output row mm < 2P
CRC_HD u32 conv1_stage_row(int mm, int P, int zdc) { return zdc ? (u32)((mm & 1) * P + (mm >> 1)) * (u32)zdc : (u32)mm * 32; }
// window offset of output row mm: rows past 2P re-read the last one (they are never stored).  Pixel -> (row, column) of the map with one multiply: p < 1024,
// yo <= 32, so (p rcp) >> 16 is exact
CRC_HD u32 conv1_window_row(int mm, const Conv1RowGeom &g)
{
    const u32 rcp_yo = (65536u + (u32)g.yo - 1) / (u32)g.yo;
    const int mrow = mm < 2 * g.P - 1 ? mm : 2 * g.P - 1, p = mrow >> 1, c = mrow & 1, ox = (int)(((u32)p * rcp_yo) >> 16), oy = p - ox * g.yo;
    return (u32)c * g.poly_bytes + (u32)(ox * g.xs) * g.px_rs + (u32)(oy * g.ystr) * 8;
}
CRC_HD Conv1RowEntry conv1_row_entry(int mm, const Conv1RowGeom &g)
{
    return Conv1RowEntry{conv1_window_row(mm, g), mm < 2 * g.P ? conv1_stage_row(mm, g.P, g.zdc) : 0u};
}
