// window_check.cpp -- the window geometry of crcnn_amd/csrc/window.h against brute force: every one-axis shape with an image of 1..16, a stride of 1..4 and a
// window of 1..17 is walked the way the reference walks it (Layer::computeBoundaries: for (i = 0; i < xd - max(xf, xs) + 1; i += xs)), and the header's answers are
// compared with what the walk found -- index by index, not with the header's formulas written out again.  Each x axis is paired with a DIFFERENT y axis (and each
// pool or box with a different one on y), so that an answer taken from the wrong axis cannot pass.  Checked per window:
//   ok() is true exactly when the walk makes the (xd - xf) / xs + 1 iterations the reference sizes its result for, at least one, every window inside the image
//   (a window one larger than the image at stride 1 makes 0 iterations of 0: not a layer);
//   xo(), yo() are the walk's iteration counts, P() and P64() their product;
//   fold(): for every sum pool of stride 1..3 and window 1..4 that crc_plan_fold_pool's shape test admits, output j of the folded window covers the input indices
//   from the first one of pooled output j's first convolution window to the last one of its last, and there are as many outputs as pooled ones;
//   boxed(): for every box of at most 9 terms, the window on the box sums reads, with multiplicity, the input indices that the enlarged window fold(1, 1, bxf, byf)
//   reads with the weights ones(xf) * box, output for output;
//   pool_geom(): the members of a PoolGeom written out by hand.
// A stand-alone program: it builds with host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "window.h"

struct Axis { int d, s, f; };
struct Walk { std::vector<int> start; bool inside, ok; int it; };
static Axis cur_x, cur_y;
#define FAIL(...) do { printf("FAIL x=(%d,%d,%d) y=(%d,%d,%d): ", cur_x.d, cur_x.s, cur_x.f, cur_y.d, cur_y.s, cur_y.f); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static Walk walk(const Axis &a)
{
    Walk w{{}, true, false, 0};
    for (int i = 0; i < a.d - (a.f > a.s ? a.f : a.s) + 1; i += a.s) {
        w.start.push_back(i);
        if (i < 0 || i + a.f > a.d) w.inside = false;
    }
    w.it = (int)w.start.size();
    w.ok = w.it >= 1 && w.it == (a.d - a.f) / a.s + 1 && w.inside;
    return w;
}
static long n_fold = 0, n_box = 0, n_index = 0;

// one axis of a folded window (stride fs, window ff, fo outputs) against the pool (ps, pf) on the walk's outputs
static bool fold_axis(const Axis &a, const Walk &w, int ps, int pf, int fs, int ff, int fo)
{
    int pooled = 0;
    for (int i = 0; i + pf <= w.it; i += ps) pooled++;
    if (pooled < 1) return false;                                   // the pool's window must fit the convolution's output
    const int hull = w.start[pf - 1] + a.f - w.start[0];           // pooled output 0: first index of its first window .. last index of its last
    int folded = 0;
    for (int i = 0; i + hull <= a.d; i += a.s * ps) folded++;
    if (folded != pooled) return false;                             // the folded convolution must produce exactly the pooled tensor
    if (fo != pooled) FAIL("pool (%d, %d): the folded window has %d outputs, the pooled tensor %d", ps, pf, fo, pooled);
    for (int j = 0; j < pooled; j++) {
        const int first = w.start[j * ps], last = w.start[j * ps + pf - 1] + a.f - 1;
        if (j * fs != first || j * fs + ff - 1 != last) FAIL("pool (%d, %d) output %d covers %d..%d, the pooled pair %d..%d", ps, pf, j, j * fs, j * fs + ff - 1, first, last);
        n_index += ff;
    }
    return true;
}
// one axis of a boxed window (summed image bd, stride bs, window bf, bo outputs) against the enlarged window (stride es, window ef, eo outputs)
static bool box_axis(const Axis &a, int b, int bd, int bs, int bf, int bo, int es, int ef, int eo)
{
    int sums = 0;
    for (int p = 0; p + (b - 1) * a.s < a.d; p++) sums++;           // box sums whose every term is a pixel
    if (bd != sums && !(sums == 0 && bd <= 0)) FAIL("box %d: a summed image of %d, %d sums exist", b, bd, sums);
    if (sums < a.f) return false;
    std::vector<int> weight(a.f + (b - 1) * a.s, 0);                 // ones(xf) * box: the enlarged window's weights
    for (int u = 0; u < a.f; u++) for (int t = 0; t < b; t++) weight[u + t * a.s]++;
    if ((int)weight.size() != ef) FAIL("box %d: the enlarged window has %d taps, ones * box %zu", b, ef, weight.size());
    if (bo != eo) FAIL("box %d: %d outputs on the box sums, %d with the enlarged window", b, bo, eo);
    for (int j = 0; j < bo; j++) {
        std::vector<int> reads(a.d, 0), want(a.d, 0);
        for (int u = 0; u < bf; u++)
            for (int t = 0; t < b; t++) {
                const int sum = j * bs + u, px = sum + t * a.s;     // pixel t of box sum `sum`
                if (sum >= bd || px >= a.d) FAIL("box %d output %d reads sum %d of %d, pixel %d of %d", b, j, sum, bd, px, a.d);
                reads[px]++;
            }
        for (int t = 0; t < ef; t++) {
            if (j * es + t >= a.d) FAIL("box %d output %d: the enlarged window reads pixel %d of %d", b, j, j * es + t, a.d);
            want[j * es + t] += weight[t];
        }
        for (int p = 0; p < a.d; p++) if (reads[p] != want[p]) FAIL("box %d output %d pixel %d: read %d times, weight %d", b, j, p, reads[p], want[p]);
        n_index += a.d;
    }
    return true;
}

int main()
{
    static_assert(sizeof(PoolGeom) == 8 * sizeof(int), "PoolGeom is a kernel argument: eight ints");
    std::vector<Axis> all, good;
    for (int d = 1; d <= 16; d++) for (int s = 1; s <= 4; s++) for (int f = 1; f <= 17; f++) { all.push_back({d, s, f}); if (walk(all.back()).ok) good.push_back(all.back()); }
    // every shape on x beside another one on y (i -> 7 i + 13 is a bijection mod 1088 without a fixed point: every shape stands on either axis once), then the
    // valid ones among themselves, where folds and boxes have something to do
    std::vector<std::pair<Axis, Axis>> pairs;
    for (size_t i = 0; i < all.size(); i++) pairs.push_back({all[i], all[(i * 7 + 13) % all.size()]});
    for (size_t i = 0; i < good.size(); i++) for (size_t m : {(size_t)1, (size_t)37}) pairs.push_back({good[i], good[(i * 5 + m) % good.size()]});
    long windows = 0, valid = 0;
    for (const auto &pr : pairs) {
        const Axis x = pr.first, y = pr.second;
        cur_x = x; cur_y = y;
        if (x.d == y.d && x.s == y.s && x.f == y.f) continue;
        const Walk wx = walk(x), wy = walk(y);
        const Window w{x.d, y.d, x.s, y.s, x.f, y.f};
        windows++;
        if (w.ok() != (wx.ok && wy.ok)) FAIL("ok() = %d, the walks %d and %d", (int)w.ok(), (int)wx.ok, (int)wy.ok);
        if (wx.ok && w.xo() != wx.it) FAIL("xo() = %d, %d iterations", w.xo(), wx.it);
        if (wy.ok && w.yo() != wy.it) FAIL("yo() = %d, %d iterations", w.yo(), wy.it);
        if (!w.ok()) continue;
        valid++;
        if (w.P() != wx.it * wy.it || w.P64() != (long long)wx.it * wy.it) FAIL("P() = %d, P64() = %lld", w.P(), w.P64());
        const PoolGeom g = pool_geom(w), hand{x.d, y.d, x.s, y.s, x.f, y.f, wx.it, wy.it};
        if (g.xd != hand.xd || g.yd != hand.yd || g.xs != hand.xs || g.ys != hand.ys || g.xf != hand.xf || g.yf != hand.yf || g.xo != hand.xo || g.yo != hand.yo)
            FAIL("pool_geom differs from the hand-built PoolGeom");
        // pools: (stride, window) on x beside another pair on y
        for (int q = 0; q < 12; q++) {
            const int r = (q * 5 + 1) % 12, pxs = q / 4 + 1, pxf = q % 4 + 1, pys = r / 4 + 1, pyf = r % 4 + 1;
            const Window w2 = w.fold(pxs, pys, pxf, pyf);
            if (w2.xd != x.d || w2.yd != y.d) FAIL("fold changes the image");
            const bool fx = fold_axis(x, wx, pxs, pxf, w2.xs, w2.xf, w2.xo()), fy = fold_axis(y, wy, pys, pyf, w2.ys, w2.yf, w2.yo());
            if (fx && fy) n_fold++;
        }
        // boxes of at most 9 terms
        for (int bxf = 1; bxf <= 9; bxf++)
            for (int byf = 1; bxf * byf <= 9; byf++) {
                const Window wb = w.boxed(bxf, byf), we = w.fold(1, 1, bxf, byf);
                if (wb.xs != x.s || wb.ys != y.s || wb.xf != x.f || wb.yf != y.f) FAIL("box %d x %d: boxed() changes stride or window", bxf, byf);
                if (wb.xd < wb.xf || wb.yd < wb.yf) continue;                       // (no output: nothing to divide for)
                const bool bx = box_axis(x, bxf, wb.xd, wb.xs, wb.xf, wb.xo(), we.xs, we.xf, we.xo()),
                           by = box_axis(y, byf, wb.yd, wb.ys, wb.yf, wb.yo(), we.ys, we.yf, we.yo());
                if (bx && by) n_box++;
            }
    }
    if (all.size() != 16 * 4 * 17) { printf("FAIL shape list\n"); return 1; }
    printf("ok %ld windows %ld valid %ld folds %ld boxes %ld indices\n", windows, valid, n_fold, n_box, n_index);
    return 0;
}
