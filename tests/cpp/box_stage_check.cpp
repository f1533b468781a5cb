// box_stage_check.cpp -- the index arithmetic of the staged box of the pixel-major image pack (crcnn_amd/csrc/boxstage.h, used by kernels_mfma1.hip
// limb_pack_box_kernel_px) walked on the CPU the way the kernel walks it: the same helpers, the same loops over (segment row, batch), (row of the group, 16-column
// half, column), the phases of a group one after the other as the barriers order them.  Every input image up to 32 x 32, strides 1-3, every box of at most 9
// terms that leaves a summed image of at least one pixel -- a superset of what k_limb_conv1_box_shape accepts for base windows up to 8 x 8 (the window only asks
// for a summed image at least as large as itself; the index arithmetic does not see it) -- and the walks: one row group per workgroup, one workgroup per image,
// and (equal strides) two workgroups per image.  Per shape and walk:
//   every global read is a pixel of the image, and with one workgroup per image no pixel is read twice;
//   every LDS word lies inside the allocation the launcher asks for (box_lds_bytes), for the first and the last slot of the workgroup;
//   no ring cell is written twice within one group's loads, and every term read finds the pixel it wants (nothing overwritten early, nothing stale);
//   every output pixel's terms are the box's terms (a weighted sum over random pixel weights against the definition);
//   every output pixel and every padding pixel of an odd width is staged and stored exactly once, the ragged last group included.
// "box_stage_check path yd bxf xs ydo" prints which body the launcher takes for a box: staged or direct.  A stand-alone program: it builds with host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "boxstage.h"

static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static unsigned px_rs(int ydo) { return ((unsigned)ydo * 8 + 15) / 16 * 16; }        // kernels_mfma1.hip conv1_px_rs: a row of the packed image, bytes
#define FAIL(...) do { printf("FAIL xd=%d yd=%d xs=%d ys=%d box=%dx%d wpi=%d: ", xd, yd, xs, ys, bxf, byf, wpi); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)
#define BOX_LD 16

static u64 weight[32 * 32];
static long checked_pixels = 0;
// what the walk keeps of the LDS: per ring cell the pixel it holds and when it was written (epochs instead of clearing), and the digit staging of one slot.  Slots
// only enter an LDS word's index as its last term, so the first and the last slot bound every word
struct Cell { int px; long walk, group; };
static Cell ring[64 * 64];
static int dig[BOX_RG * 256 + 16], loads[32 * 32], stored[32 * 32];
static long epoch = 0;

static void walk(int xd, int yd, int xs, int ys, int bxf, int byf, int wpi)
{
    const int xdo = xd - (bxf - 1) * xs, ydo = yd - (byf - 1) * ys;
    const unsigned rs = px_rs(ydo), sstride = BOX_RG * rs + 16;
    const u32 ring_px = box_ring_px(yd, bxf, xs);
    const size_t ring_words = box_ring_bytes(yd, bxf, xs) / 8, dig_bytes = box_lds_bytes(yd, bxf, xs, rs) - box_ring_bytes(yd, bxf, xs);
    if (box_ring_bytes(yd, bxf, xs) % 16) FAIL("the digit staging behind the ring is not 16-byte aligned");
    if (box_lds_bytes(yd, bxf, xs, rs) > BOX_LDS_MAX || ring_px > 64 * 64) FAIL("a staged box of %zu bytes", box_lds_bytes(yd, bxf, xs, rs));
    for (int p = 0; p < xd * yd; p++) loads[p] = 0;
    for (int p = 0; p < xdo * (int)(rs / 8); p++) stored[p] = 0;
    for (int w = 0; w < wpi; w++) {
        const int g0 = box_walk_first(w, xdo, wpi), g1 = box_walk_end(w, xdo, wpi);
        if (w == 0 && g0 != 0) FAIL("the first walk starts at group %d", g0);
        if (w == wpi - 1 && g1 != box_row_groups(xdo)) FAIL("the last walk ends at group %d", g1);
        if (w + 1 < wpi && box_walk_first(w + 1, xdo, wpi) < g1) FAIL("walks overlap");
        if (w + 1 < wpi && box_walk_first(w + 1, xdo, wpi) > g1 && g1 < box_row_groups(xdo)) FAIL("walks leave a gap");
        const long this_walk = ++epoch;
        for (int g = g0; g < g1; g++) {
            // (1) the loads
            const long this_group = ++epoch;
            const int p1 = box_load_end(g, xd, yd, bxf, xs);
            for (int seg = 0; seg < 8; seg++)
                for (int pb = box_load_first(g, g == g0, xd, yd, bxf, xs) + seg; pb < p1; pb += 8 * BOX_LD)
                    for (int u = 0; u < BOX_LD; u++) {
                        const int p = pb + 8 * u;
                        if (p >= p1) continue;
                        if (p < 0 || p >= xd * yd) FAIL("global read of pixel %d", p);
                        loads[p]++;
                        const u32 first = box_cell((u32)p, ring_px, 0), last = box_cell((u32)p, ring_px, BOX_RSL - 1);
                        if (first % BOX_RSL || last != first + BOX_RSL - 1 || last >= ring_words) FAIL("ring words %u .. %u of %zu", first, last, ring_words);
                        Cell &c = ring[first / BOX_RSL];
                        if (c.group == this_group) FAIL("ring cell %u written twice by group %d", first / BOX_RSL, g);
                        c.px = p; c.walk = this_walk; c.group = this_group;
                    }
            // (2) the sums and the digit staging
            for (unsigned o = 0; o < sstride; o++) dig[o] = 0;
            for (int h = 0; h < 2; h++)
                for (int qrow = 0; qrow < BOX_RG; qrow++) {
                    const int row = g * BOX_RG + qrow;
                    if (row >= xdo) continue;
                    u64 sum[16] = {0}, want[16] = {0};
                    for (int a = 0; a < bxf; a++)
                        for (int bb = 0; bb < byf; bb++) {
                            u32 pos = box_ring_pos(box_term_px(row, box_col(h, 0), a, bb, xs, ys, yd), ring_px);
                            for (int colx = 0; colx < 16; colx++) {
                                if (box_col(h, colx) < ydo) {
                                    const u32 first = box_pos_cell(pos, 0), last = box_pos_cell(pos, BOX_RSL - 1);
                                    if (first % BOX_RSL || last != first + BOX_RSL - 1 || last >= ring_words) FAIL("ring read of words %u .. %u of %zu", first, last, ring_words);
                                    const int r = row + a * xs, cc = box_col(h, colx) + bb * ys;          // the definition
                                    if (r >= xd || cc >= yd) FAIL("term (%d, %d) outside the image", r, cc);
                                    const Cell &c = ring[first / BOX_RSL];
                                    if (c.walk != this_walk || c.px != r * yd + cc) FAIL("pixel (%d, %d) term (%d, %d) finds pixel %d", row, box_col(h, colx), a, bb, c.walk == this_walk ? c.px : -1);
                                    sum[colx] += weight[c.px]; want[colx] += weight[r * yd + cc];
                                }
                                pos = box_ring_step(pos, 1, ring_px);
                            }
                        }
                    for (int colx = 0; colx < 16; colx++) {
                        const int col = box_col(h, colx);
                        if ((unsigned)col * 8 >= rs) continue;
                        if (sum[colx] != want[colx]) FAIL("pixel (%d, %d): not the box's terms", row, col);
                        const size_t at = qrow * rs + (size_t)(h * 16 + colx) * 8;                   // within the slot's sstride bytes
                        if (at + 8 > sstride || (size_t)(BOX_RSL - 1) * sstride + at + 8 > dig_bytes) FAIL("digit staging byte %zu of %zu", (size_t)(BOX_RSL - 1) * sstride + at, dig_bytes);
                        for (int byte = 0; byte < 8; byte++) dig[at + byte]++;
                        checked_pixels++;
                    }
                }
            // (3) the transposed stores: every staged byte of the rows that exist leaves once, no byte that was not staged
            const int per_run = BOX_RG * rs / 16, valid = box_rows_here(g, xdo) * (int)rs / 16;
            if (valid <= 0) FAIL("group %d has no rows", g);
            for (int o = 0; o < BOX_RSL * per_run; o++) {                  // (thread o % 256; the slots differ by sl * sstride only: the last one bounds the reads)
                const int sl = o / per_run, part = o - sl * per_run;
                if (part >= valid || sl != BOX_RSL - 1) continue;
                if ((size_t)sl * sstride + part * 16 + 16 > dig_bytes) FAIL("store reads staging byte %zu of %zu", (size_t)sl * sstride + part * 16, dig_bytes);
                for (int byte = 0; byte < 16; byte++)
                    if (dig[part * 16 + byte] != 1) FAIL("stored byte %d staged %d times", part * 16 + byte, dig[part * 16 + byte]);
                stored[(size_t)(g * BOX_RG) * (rs / 8) + part * 2]++; stored[(size_t)(g * BOX_RG) * (rs / 8) + part * 2 + 1]++;
            }
        }
    }
    for (int p = 0; p < xdo * (int)(rs / 8); p++) if (stored[p] != 1) FAIL("output pixel %d stored %d times", p, stored[p]);
    if (wpi == 1) for (int p = 0; p < xd * yd; p++) if (loads[p] > 1) FAIL("pixel %d read %d times by one walk", p, loads[p]);
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "path")) {
        const int yd = atoi(argv[2]), bxf = atoi(argv[3]), xs = atoi(argv[4]), ydo = atoi(argv[5]);
        printf("%s %zu\n", box_staged(yd, bxf, xs, px_rs(ydo)) ? "staged" : "direct", box_lds_bytes(yd, bxf, xs, px_rs(ydo)));
        return 0;
    }
    for (u64 &wv : weight) wv = rnd();
    long shapes = 0, direct = 0;
    for (int xd = 1; xd <= 32; xd++)
        for (int yd = 1; yd <= 32; yd++)
            for (int xs = 1; xs <= 3; xs++)
                for (int ys = 1; ys <= 3; ys++)
                    for (int bxf = 1; bxf <= 9; bxf++)
                        for (int byf = 1; bxf * byf <= 9; byf++) {
                            const int xdo = xd - (bxf - 1) * xs, ydo = yd - (byf - 1) * ys;
                            if (bxf * byf == 1 || xdo < 1 || ydo < 1) continue;
                            if (!box_staged(yd, bxf, xs, px_rs(ydo))) { direct++; continue; }
                            const int rgs = box_row_groups(xdo);
                            walk(xd, yd, xs, ys, bxf, byf, rgs);
                            if (rgs > 2 && xs == ys) walk(xd, yd, xs, ys, bxf, byf, 2);           // (a walk no launcher asks for: the helpers' general case, a third of the shapes)
                            if (rgs > 1) walk(xd, yd, xs, ys, bxf, byf, 1);
                            shapes++;
                        }
    // the widest ring of a 32 x 32 image that still fits, and the one that does not (tests/test_gpu_conv1_box_staged.py runs both)
    if (!box_staged(32, 2, 2, px_rs(30)) || box_staged(32, 9, 3, px_rs(32))) { printf("FAIL staged / direct boundary\n"); return 1; }
    printf("ok %ld shapes %ld direct %ld pixels\n", shapes, direct, checked_pixels);
    return 0;
}
