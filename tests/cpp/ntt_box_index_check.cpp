// ntt_box_index_check.cpp -- the index arithmetic of the boxed forward transform (crcnn_amd/csrc/nttbox.h, used by kernels.hip ntt_rows_wave_kernel<.., BOX = true>
// and its launcher k_ntt_ct_box) walked on the CPU the way the launch walks it: nttbox_grid blocks, every block through nttbox_block_row, every term of a row
// through nttbox_src_row.  Shapes: the images, boxes and moduli counts of tests/test_gpu_ntt_box.py (3 images of 7 x 6 pixels, k = 1, 2, 3) and PlainModelTiny's
// 28 x 28 image with the 2 x 2 box at stride 2 for 1, 2, 3 and 128 images (k = 2); both block orders.  Per shape and order:
//   every output row is hit exactly once, and a block past the last row answers "return" -- the plain order has none, the grouped order exactly its padding;
//   the row a block gets is ((b xdo ydo + r ydo + c) 2 + poly) k + mod of the (b, r, c, poly, mod) it reports, all of them in range;
//   every term's source row lies inside the input and equals the naive formula ((b xd yd + (r + a xs) yd + (c + bb ys)) 2 + poly) k + mod;
//   in the grouped order the blocks of one XCD (block mod 8) walk whole (image, poly, modulus) planes, pixels in raster order.
// The sums themselves: limbred.h sum_reduce16 covers 9 (q - 1) for the eight default moduli -- tests/cpp/box_sum_check.cpp checks that, not this program.
// A stand-alone program: it builds with host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nttbox.h"

#define FAIL(...) do { printf("FAIL B=%zu %dx%d box=%dx%d stride=%d,%d k=%d order=%d: ", B, xd, yd, bxf, byf, xs, ys, k, order); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static long checked_rows = 0, checked_terms = 0, padding_blocks = 0;

static void walk(size_t B, int xd, int yd, int bxf, int byf, int xs, int ys, int k, int order)
{
    const NttBox g = nttbox_make(xd, yd, bxf, byf, xs, ys);
    if (!nttbox_ok(g)) FAIL("not a box");
    if (g.xdo != xd - (bxf - 1) * xs || g.ydo != yd - (byf - 1) * ys) FAIL("summed image %d x %d", g.xdo, g.ydo);
    const size_t rows = nttbox_rows(B, g, k), grid = nttbox_grid(order, B, g, k), in_rows = B * xd * yd * 2 * (size_t)k;
    if (rows != B * g.xdo * g.ydo * 2 * (size_t)k) FAIL("%zu rows", rows);
    if (grid < rows || grid > 0x7fffffffULL) FAIL("a grid of %zu blocks for %zu rows", grid, rows);
    if (order == 0 && grid != rows) FAIL("the plain order pads: %zu blocks", grid);
    std::vector<unsigned char> hit(rows, 0);
    // grouped order: the plane and pixel an XCD is at
    long long cur_plane[8]; size_t next_px[8];
    for (int x = 0; x < 8; x++) { cur_plane[x] = -1; next_px[x] = 0; }
    size_t returned = 0;
    for (size_t blk = 0; blk < grid; blk++) {
        NttBoxRow o{};
        if (!nttbox_block_row(order, (u32)blk, (u32)B, g, k, o)) { returned++; continue; }
        if (o.b >= B || o.r < 0 || o.r >= g.xdo || o.c < 0 || o.c >= g.ydo || o.poly < 0 || o.poly > 1 || o.mod < 0 || o.mod >= k) FAIL("block %zu: (%u, %d, %d, %d, %d)", blk, o.b, o.r, o.c, o.poly, o.mod);
        const size_t row = nttbox_row_of(o, g, k);
        if (row != ((((size_t)o.b * g.xdo + o.r) * g.ydo + o.c) * 2 + o.poly) * k + o.mod) FAIL("block %zu: row %zu", blk, row);
        if (row >= rows) FAIL("block %zu: row %zu of %zu", blk, row, rows);
        if (order == 0 && row != blk) FAIL("block %zu: row %zu in the plain order", blk, row);
        if (hit[row]++) FAIL("row %zu twice", row);
        if (order == 1) {
            const int x = (int)(blk & 7);
            const long long plane = ((long long)o.b * 2 + o.poly) * k + o.mod; const size_t px = (size_t)o.r * g.ydo + o.c;
            if (px == 0) { if (next_px[x] != 0 || plane <= cur_plane[x]) FAIL("block %zu starts plane %lld on XCD %d at pixel %zu", blk, plane, x, next_px[x]); cur_plane[x] = plane; }
            if (plane != cur_plane[x] || px != next_px[x]) FAIL("block %zu: plane %lld pixel %zu, XCD %d is at plane %lld pixel %zu", blk, plane, px, x, cur_plane[x], next_px[x]);
            next_px[x] = px + 1 == nttbox_pixels(g) ? 0 : px + 1;
        }
        for (int a = 0; a < bxf; a++)
            for (int bb = 0; bb < byf; bb++) {
                const size_t s = nttbox_src_row(o, g, k, a, bb);
                const int r = o.r + a * xs, c = o.c + bb * ys;
                if (r >= xd || c >= yd) FAIL("row %zu term (%d, %d): pixel (%d, %d)", row, a, bb, r, c);
                if (s >= in_rows || s != ((((size_t)o.b * xd + r) * yd + c) * 2 + o.poly) * k + o.mod) FAIL("row %zu term (%d, %d): source row %zu", row, a, bb, s);
                checked_terms++;
            }
        checked_rows++;
    }
    for (size_t r = 0; r < rows; r++) if (hit[r] != 1) FAIL("row %zu hit %d times", r, hit[r]);
    if (returned != grid - rows) FAIL("%zu blocks return, %zu are padding", returned, grid - rows);
    padding_blocks += (long)returned;
}

int main()
{
    static const int boxes[][4] = {{2, 2, 2, 2}, {1, 2, 1, 1}, {2, 1, 1, 1}, {1, 2, 2, 2}, {2, 1, 2, 2}, {3, 3, 1, 1}, {2, 2, 3, 3}};     // bxf, byf, xs, ys
    long shapes = 0;
    for (int order = 0; order < 2; order++) {
        for (const auto &bx : boxes)
            for (int k = 1; k <= 3; k++) { walk(3, 7, 6, bx[0], bx[1], bx[2], bx[3], k, order); shapes++; }
        for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)128}) { walk(B, 28, 28, 2, 2, 2, 2, 2, order); shapes++; }
    }
    printf("ok %ld shapes %ld rows %ld terms %ld padding\n", shapes, checked_rows, checked_terms, padding_blocks);
    return 0;
}
