// window.h -- the geometry of a convolution / pooling window, defined once for the host side of the library (plain C++17: no HIP, no crc_ctx)
#pragma once

// an xf x yf window moved in steps of (xs, ys) over an xd x yd image (valid padding)
struct Window {
    int xd, yd, xs, ys, xf, yf;
    bool ok() const               // (conv_shape_ok: the shape test of every entry point that takes a window)
    {
        if (xd < 1 || yd < 1 || xs < 1 || ys < 1 || xf < 1 || yf < 1 || xf > xd || yf > yd) return false;
        // the reference iterates i in [0, xd - max(xf,xs) + 1) step xs (Layer::computeBoundaries, layer.cpp:12-26) but sizes
        // its result (xd-xf)/xs+1: when the stride exceeds the window the two disagree and trailing outputs stay empty
        // Ciphertexts -- reject those shapes instead of inventing values.
        const int xl = xd - (xf > xs ? xf : xs) + 1, yl = yd - (yf > ys ? yf : ys) + 1;
        if (xl < 1 || yl < 1) return false;
        return (xl + xs - 1) / xs == xo() && (yl + ys - 1) / ys == yo();
    }
    // output positions (the caller has checked xs, ys >= 1); P64 where the product is formed in 64 bits
    int xo() const { return (xd - xf) / xs + 1; }
    int yo() const { return (yd - yf) / ys + 1; }
    int P() const { return xo() * yo(); }
    long long P64() const { return (long long)xo() * yo(); }
    // with the pxf x pyf sum pool of stride (pxs, pys) behind it folded in: output j of the result covers what pooled output j of the pair covers
    Window fold(int pxs, int pys, int pxf, int pyf) const { return {xd, yd, xs * pxs, ys * pys, (pxf - 1) * xs + xf, (pyf - 1) * ys + yf}; }
    // on the bxf x byf box sums of its image, taken at the window's own stride: what fold(1, 1, bxf, byf) reads, term for term
    Window boxed(int bxf, int byf) const { return {xd - (bxf - 1) * xs, yd - (byf - 1) * ys, xs, ys, xf, yf}; }
};

// a conv / dense layer: nf filters of zd channels each (dense: a 1 x 1 window on a 1 x 1 image, zd = in_dim, nf = out_dim)
struct LayerShape {
    Window w; int zd, nf;
    int T() const { return zd * w.xf * w.yf; }             // terms per output
    int in_cts() const { return zd * w.xd * w.yd; }        // input ciphertexts per image
};

// a pooling window as the kernels take it (by value: members, order and size are part of their argument lists)
struct PoolGeom { int xd, yd, xs, ys, xf, yf, xo, yo; };
static inline PoolGeom pool_geom(const Window &w) { return {w.xd, w.yd, w.xs, w.ys, w.xf, w.yf, w.xo(), w.yo()}; }
