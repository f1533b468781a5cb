// conv1_rowtab_check.cpp -- the row table of the pixel-major one-channel convolution and the staged limb result's layout (crcnn_amd/csrc/conv1_rowtab.h, used by
// kernels_mfma1.hip mfma_conv1_kernel_px / mfma_conv1_kernel) walked on the CPU: the same helpers the kernels call.  For the shapes of
// tests/test_gpu_conv1_staging_layout.py and a sweep of small (xd, yd, xs, ys, xf, yf), with the blocked consumer (32 channel bytes per position) and flat
// consumers of 4, 12 and 28 channel bytes:
//   every table entry equals the expressions the kernel computed per tile before it had a table (written out here again, with a true division beside the
//   reciprocal multiply), rows past 2P re-reading the last row;
//   every window lies inside its poly's block of the image buffer, the last tap included;
//   every staged dword (row, filter group, plane) lies inside the staging area, no two share a byte, and each sits where the limb tensor of the consumer has it
//   ([plane][row][32] blocked, [plane][poly][pixel][zdc] flat) -- so the copy-out is a linear copy;
//   the table and the staging area fit the allocation the launcher asks for, 8-byte aligned.
// A stand-alone program: it builds with host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv1_rowtab.h"

// kernels_mfma1.hip: the pixel-major image's row and poly strides
static unsigned px_rs(int yd) { return ((unsigned)yd * 8 + 15) / 16 * 16; }
static unsigned px_poly_bytes(int xd, int yd) { const unsigned b = (unsigned)xd * px_rs(yd); return b + (128 + 256 - b % 256) % 256; }
static unsigned px_img_stride(int xd, int yd) { return (2 * px_poly_bytes(xd, yd) + 1023) / 1024 * 1024; }

#define FAIL(...) do { printf("FAIL xd=%d yd=%d xs=%d ys=%d xf=%d yf=%d zdc=%d: ", xd, yd, xs, ys, xf, yf, zdc); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static long entries = 0, dwords = 0;

static void check(int xd, int yd, int xs, int ys, int xf, int yf, int zdc)
{
    const int xo = (xd - xf) / xs + 1, yo = (yd - yf) / ys + 1, P = xo * yo;
    const Conv1RowGeom g{P, yo, xs, ys, px_rs(yd), px_poly_bytes(xd, yd), zdc};
    const int rows = conv1_rowtab_rows(P), mtiles = (2 * P + 15) / 16;
    if (rows != mtiles * 16 || rows < 2 * P || rows >= 2 * P + 16) FAIL("%d table rows for %d output rows", rows, 2 * P);
    if (conv1_rowtab_bytes(P) != (size_t)rows * 8 || sizeof(Conv1RowEntry) != 8) FAIL("table bytes");
    const u32 stage_bytes = conv1_stage_bytes(P, zdc), pstride = conv1_stage_plane_stride(P, zdc);
    const int chan_bytes = zdc ? zdc : 32;
    // what the launcher has always asked for
    const u32 want_bytes = zdc ? (u32)((7 * 2 * P * zdc + 15) / 16 * 16) : (u32)(7 * P * 2 * 32);
    if (stage_bytes != want_bytes || stage_bytes % 16) FAIL("staging area of %u bytes, not %u", stage_bytes, want_bytes);
    if (pstride != (u32)(2 * P * chan_bytes)) FAIL("plane stride %u", pstride);
    if ((2 * (size_t)px_img_stride(xd, yd) + stage_bytes) % 8) FAIL("the table behind the staging area is not 8-byte aligned");
    std::vector<unsigned char> used(stage_bytes, 0);
    const u32 rcp_yo = (65536u + (u32)yo - 1) / (u32)yo;
    for (int mm = 0; mm < rows; mm++) {
        const Conv1RowEntry e = conv1_row_entry(mm, g);
        entries++;
        // the window: the kernel's expressions before the table ...
        const int mrow = mm < 2 * P - 1 ? mm : 2 * P - 1, p = mrow >> 1, c = mrow & 1, ox = (int)(((u32)p * rcp_yo) >> 16), oy = p - ox * yo;
        if (ox != p / yo || oy != p % yo) FAIL("pixel %d: the reciprocal gives (%d, %d)", p, ox, oy);
        const u32 win = (u32)c * g.poly_bytes + (u32)(ox * xs) * g.px_rs + (u32)(oy * ys) * 8;
        if (e.win != win) FAIL("row %d: window offset %u, the kernel computed %u", mm, e.win, win);
        // ... and its last tap inside the poly's rows
        const u32 last = e.win + (u32)(xf - 1) * g.px_rs + (u32)(yf - 1) * 8 + 8;
        if (last > (u32)c * g.poly_bytes + (u32)xd * g.px_rs || last > px_img_stride(xd, yd)) FAIL("row %d: window ends at byte %u", mm, last);
        if (mm >= 2 * P) { if (e.stg != 0) FAIL("row %d past the map has staging offset %u", mm, e.stg); continue; }
        // the staging offset: the kernel's expressions for the flat form, the consumer's own layout for the blocked one
        const u32 stg = zdc ? (u32)(((mm & 1) * P + (mm >> 1)) * zdc) : (u32)mm * 32;
        if (e.stg != stg) FAIL("row %d: staging offset %u, expected %u", mm, e.stg, stg);
        for (int f0 = 0; f0 < 32; f0 += 4) {
            if (f0 >= chan_bytes) continue;                              // the kernel's guard
            for (int l = 0; l < CONV1_NPL; l++) {
                const u32 at = e.stg + (u32)f0 + (u32)l * pstride;
                if (at + 4 > stage_bytes) FAIL("row %d filters %d.. plane %d: staging byte %u of %u", mm, f0, l, at, stage_bytes);
                for (int byte = 0; byte < 4; byte++) { if (used[at + byte]) FAIL("staging byte %u written twice (row %d filters %d.. plane %d)", at + byte, mm, f0, l); used[at + byte] = 1; }
                // the image's bytes in the limb tensor: [plane][row][32] / [plane][poly][pixel][zdc] (kernels_mfma.hip)
                const u32 tensor = zdc ? ((u32)(l * 2 + (mm & 1)) * (u32)P + (u32)(mm >> 1)) * (u32)zdc + (u32)f0 : ((u32)l * 2 * P + (u32)mm) * 32 + (u32)f0;
                if (at != tensor) FAIL("row %d filters %d.. plane %d: staged at %u, the tensor has it at %u", mm, f0, l, at, tensor);
                dwords++;
            }
        }
    }
    // every byte of the tensor's positions is staged (the flat form's round-up to 16 is zeroed once per workgroup)
    for (u32 at = 0; at < CONV1_NPL * pstride; at++) if (!used[at]) FAIL("staging byte %u never written", at);
}

int main()
{
    // tests/test_gpu_conv1_staging_layout.py
    const int shapes[][7] = {{3, 3, 1, 1, 2, 2, 32}, {3, 5, 1, 1, 2, 2, 32}, {8, 7, 1, 1, 2, 2, 32}, {26, 26, 2, 2, 6, 6, 32}, {9, 9, 2, 2, 3, 3, 32}, {8, 7, 1, 1, 2, 2, 5},
                             {28, 28, 2, 2, 7, 7, 20}, {28, 28, 2, 2, 6, 6, 32}, {32, 32, 1, 1, 1, 1, 32}};
    for (const auto &s : shapes) {
        const int nf = s[6], zdc = nf < 32 ? (nf + 3) / 4 * 4 : 0;
        check(s[0], s[1], s[2], s[3], s[4], s[5], zdc);
    }
    long swept = 0;
    for (int xd = 1; xd <= 12; xd++)
        for (int yd = 1; yd <= 12; yd++)
            for (int xs = 1; xs <= 3; xs++)
                for (int ys = 1; ys <= 3; ys++)
                    for (int xf = 1; xf <= 8 && xf <= xd; xf++)
                        for (int yf = 1; yf <= 8 && yf <= yd; yf++) {
                            if (xf * yf > 40) continue;
                            for (int zdc : {0, 4, 12, 28}) check(xd, yd, xs, ys, xf, yf, zdc);
                            swept++;
                        }
    printf("ok %ld shapes %ld entries %ld dwords\n", swept, entries, dwords);
    return 0;
}
