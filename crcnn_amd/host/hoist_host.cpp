// hoist_host -- rotateRowsMany / matvecSlots of the host classes on slot-encrypted vectors (tests/test_gpu_hoist_cpp.py).
//
//   hoist_host <dir>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/values.i64 = [n][P] int64: slot j of ciphertext c holds values[j][c] (the test tiles a vector of 8 entries
// with period 8), <dir>/w8.i64 = [8][8] and <dir>/w5.i64 = [5][8] int64 matrices.  Keys: 3^d for d = 1..7.
// Writes <dir>/<name>.i64 = [n][P] (decrypted and decomposed) for name in many_0, many_1, many_5, many_7 (one rotateRowsMany call), many_5_ntt (NTT form in and
// out), rows_1 and rows_5 (rotateRows, for the budget comparison), matvec_8x8, matvec_5x8, matvec_8x8_ntt, matvec_zero; prints "budget <name> <min bits>" per
// result, "throws <case> <exception kind>" for the exceptions and "hoist_host ok" at the end.
//
//   hoist_host <dir> bsgs          (tests/test_gpu_bsgs_cpp.py)
//
// matvecSlotsBsgs at M = 16: values.i64 tiles a vector of 16 entries with period 16, <dir>/w16.i64 = [16][16] and <dir>/w11.i64 = [11][16].  Keys: those of
// crc_bsgs_elements(16, 4, n) only.  Per case (bsgs_16x16 at B = 4, bsgs_11x16 at the default split, bsgs_16x16_ntt, bsgs_16x16_B16 = the flat product through
// the same entry point, on the diagonals 0..3 and 4, 8, 12 that the keys reach) writes <dir>/<name>.i64, prints "budget <name> <min bits>" and
// "product <name> equal|differs" (every slot against W x mod t computed here), then "keys bsgs <bytes> flat <bytes>" for a dense 16 x 16 product,
// "throws <case> <kind>" and "hoist_host bsgs ok".
//
//   hoist_host <dir> conv          (tests/test_gpu_conv_slots_cpp.py)
//
// convSlots on one image of channel planes: <dir>/image.i64 = [12][12] pixels, <dir>/w1.i64 = [2][1][3][3], <dir>/w2.i64 = [3][2][3][3] int64 weights; M = 256.
// Layer 1 is the 3 x 3 convolution with a 2 x 2 sum pool folded in (16 taps, 5 x 5 outputs at dilation 2), layer 2 a 3 x 3 convolution at that dilation (3 x 3
// outputs).  Keys: convSlotsElements of both layers, each element once.  Per case (conv_fresh = the encrypted image read back, conv_1, conv_2, conv_2_ntt = both
// layers NTT-resident) writes <dir>/<name>.i64 = [channels][H W] (decryptPlanes), prints "budget <name> <min bits>" and "conv <name> equal|differs" (every valid
// pixel against the integer convolution computed here), then "keys conv <bytes> elements <count>", "throws <case> <kind>" and "hoist_host conv ok".
//
//   hoist_host <dir> planes        (tests/test_gpu_dense_planes_cpp.py)
//
// One packed image through convSlots -> densePlanes -> densePlanes: <dir>/image.i64 = [12][12] pixels, <dir>/w1.i64 = [2][1][3][3] (the conv case's first layer:
// 5 x 5 outputs per plane at dilation 2), <dir>/w3.i64 = [6][2][25] (the dense layer over the two planes, outputs on the input lattice at slots 2 (12 a + b),
// a < 2, b < 3), <dir>/w4.i64 = [3][1][6] (the dense layer on that vector, Cin = 1, outputs at slots 0, 2, 4); M = 256.  Keys: convSlotsElements and
// densePlanesElements of the layers, each element once.  Per case (dense_1, dense_2, dense_2_ntt = all three layers NTT-resident) writes <dir>/<name>.i64 = [M]
// (the first period's slots), prints "budget <name> <min bits>" and "planes <name> equal|differs" (every output slot of every period against the integer network
// computed here, every other slot 0), then "steps conv <T> dense_1 <R> dense_2 <R>", "keys planes <bytes> prepared <bytes> elements <count>",
// "throws <case> <kind>" and "hoist_host planes ok".
//
//   hoist_host <dir> convpad       (tests/test_gpu_conv_slots_pad_cpp.py)
//
// A padded, strided chain through convSlots with a bias and a mask: <dir>/image.i64 = [12][12] pixels, <dir>/w1.i64 = [2][1][3][3], <dir>/b1.i64 = [2],
// <dir>/w2.i64 = [3][2][3][3]; M = 256, the image encrypted with a margin of 1 (pitch 13, origin 14).  Layer 1 is 3 x 3 with pad 1, stride 1, the bias and the mask
// (12 x 12 outputs, a clean tensor), layer 2 is 3 x 3 with pad 1 and stride 2 (6 x 6 outputs at dilation 2) and reads the margin the mask zeroed.  Keys:
// convSlotsElements of both layers, each element once.  Per case (convpad_fresh, convpad_1, convpad_2, convpad_2_ntt = both layers NTT-resident) writes
// <dir>/<name>.i64 = [channels][H W] (decryptPlanes), prints "budget <name> <min bits>" and "conv <name> equal|differs" (every valid pixel against the integer
// convolution computed here), "clean convpad_1 yes|no" (every slot of layer 1's result that holds no output is 0, in every period), "budget convpad_1_unmasked
// <min bits>", then "keys convpad <bytes> elements <count>", "throws <case> <kind>" and "hoist_host convpad ok".
#include "crcnn_host.h"
#include "diag_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
using namespace std;

static vector<uint64_t> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<uint64_t> v(sz / 8); f.read((char *)v.data(), sz); return v;
}
static string dir;
static int n = 0;
static void put(const char *name, const ciphertext3D &t)
{
    printf("budget %s %d\n", name, minNoiseBudget(t));
    const vector<vector<int64_t>> v = decryptSlots(t, n);
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    for (auto &row : v) f.write((const char *)row.data(), row.size() * 8);
}
static void thrown(const char *name, const function<void()> &call)
{
    const char *kind = "nothing";
    try { call(); } catch (const invalid_argument &) { kind = "invalid_argument"; } catch (const logic_error &) { kind = "logic_error"; }
    catch (const exception &) { kind = "exception"; }
    printf("throws %s %s\n", name, kind);
}
static vector<vector<int64_t>> matrix(const string &p, int rows, int cols)
{
    const auto raw = rd(p);
    vector<vector<int64_t>> W(rows, vector<int64_t>(cols));
    for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) W[i][j] = (int64_t)raw[(size_t)i * cols + j];
    return W;
}
// the decrypted slots of y against W x mod t (centred), x read back from the slots of the input: "product <name> equal|differs"
static void product(const char *name, const ciphertext3D &y, const ciphertext3D &x, const vector<vector<int64_t>> &W, int M, int64_t t)
{
    put(name, y);
    const vector<vector<int64_t>> got = decryptSlots(y, n), in = decryptSlots(x, n);
    bool equal = true;
    for (size_t c = 0; c < in[0].size(); c++)
        for (int i = 0; i < n; i++) {
            __int128 acc = 0;
            const int r = i % M;
            if (r < (int)W.size()) for (int j = 0; j < (int)W[r].size(); j++) acc += (__int128)(W[r][j] % t) * in[j][c];
            int64_t w = (int64_t)(acc % t);
            w = (w + t) % t;
            if (w > (t - 1) / 2) w -= t;
            equal = equal && got[i][c] == w;
        }
    printf("product %s %s\n", name, equal ? "equal" : "differs");
}
static int bsgs_case(const vector<uint64_t> &p, const vector<uint64_t> &q)
{
    const int M = 16, B = 4;
    const int64_t t = (int64_t)p[2];
    vector<vector<int64_t>> W16 = matrix(dir + "/w16.i64", 16, 16), W11 = matrix(dir + "/w11.i64", 11, 16);
    setParameters(n, q, (uint64_t)1 << 20, 0);
    { ciphertext3D none(1, 1, 1, 1); thrown("no_batching_bsgs", [&] { matvecSlotsBsgs(none, W16, M); }); }
    setParameters(n, q, p[2], 0);
    setSlotEncoding(0, 0);
    const auto raw = rd(dir + "/values.i64");
    const size_t P = raw.size() / n;
    vector<vector<int64_t>> images(n, vector<int64_t>(P));
    for (int j = 0; j < n; j++) for (size_t c = 0; c < P; c++) images[j][c] = (int64_t)raw[(size_t)j * P + c];
    const ciphertext3D x = encryptImageSlots(images, 1, 1, (int)P);
    thrown("no_keys_bsgs", [&] { matvecSlotsBsgs(x, W16, M); });
    const vector<uint64_t> elts = crc_bsgs_elements(M, B, n);
    generateGaloisKeys(16, elts);
    product("bsgs_16x16", matvecSlotsBsgs(x, W16, M, B), x, W16, M, t);
    product("bsgs_11x16", matvecSlotsBsgs(x, W11, M), x, W11, M, t);
    { ciphertext3D xn = rotateRowsMany(x, {0}, CRC_NTT)[0]; product("bsgs_16x16_ntt", matvecSlotsBsgs(xn, W16, M, B, CRC_NTT), x, W16, M, t); }
    vector<vector<int64_t>> Wd = W16;                                   // only the diagonals whose own keys are in the set
    for (int i = 0; i < M; i++) for (int j = 0; j < M; j++) { const int d = (j - i + M) % M; if (d >= B && d % B) Wd[i][j] = 0; }
    product("bsgs_16x16_B16", matvecSlotsBsgs(x, Wd, M, M), x, Wd, M, t);
    product("bsgs_zero", matvecSlotsBsgs(x, vector<vector<int64_t>>(16, vector<int64_t>(16, 0)), M), x, {}, M, t);
    const size_t kb = crc_evk_words(context, 16) * 8;
    printf("keys bsgs %zu flat %zu\n", elts.size() * kb, (size_t)(M - 1) * kb);
    thrown("bad_B", [&] { matvecSlotsBsgs(x, W16, M, 3); });
    thrown("B_too_large", [&] { matvecSlotsBsgs(x, W16, M, 32); });
    thrown("bad_M_bsgs", [&] { matvecSlotsBsgs(x, W16, 6); });
    thrown("missing_key_bsgs", [&] { matvecSlotsBsgs(x, W16, M, 8); });             // B = 8: the baby steps 5, 6, 7 have no key
    thrown("bad_form_bsgs", [&] { matvecSlotsBsgs(x, W16, M, B, CRC_NTTP); });
    delParameters();
    clearDeterministicSeed();
    printf("hoist_host bsgs ok\n");
    return 0;
}

// [Cin][H][W] -> [Cout][oh][ow]: the 'valid' stride-1 convolution with w [Cout][Cin][fh][fw], then a pool x pool sum pool of stride pool; exact integers
static vector<vector<int64_t>> conv_int(const vector<vector<int64_t>> &x, int H, int W, const vector<int64_t> &w, int Cout, int fh, int fw, int pool)
{
    const int Cin = (int)x.size(), oh = (H - fh + 1) / pool, ow = (W - fw + 1) / pool;
    vector<vector<int64_t>> y(Cout, vector<int64_t>((size_t)oh * ow, 0));
    for (int co = 0; co < Cout; co++) for (int r = 0; r < oh; r++) for (int c = 0; c < ow; c++)
        for (int u = 0; u < pool; u++) for (int v = 0; v < pool; v++)
            for (int ci = 0; ci < Cin; ci++) for (int a = 0; a < fh; a++) for (int b = 0; b < fw; b++)
                y[co][(size_t)r * ow + c] += w[(((size_t)co * Cin + ci) * fh + a) * fw + b] * x[ci][(size_t)(pool * r + u + a) * W + pool * c + v + b];
    return y;
}
static void planes(const char *name, const ciphertext3D &y, const SlotPlanes &g, const vector<vector<int64_t>> &want)
{
    printf("budget %s %d\n", name, minNoiseBudget(y));
    const vector<vector<int64_t>> got = decryptPlanes(y, g);
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    for (auto &row : got) f.write((const char *)row.data(), row.size() * 8);
    printf("conv %s %s\n", name, got == want ? "equal" : "differs");
}
static int conv_case(const vector<uint64_t> &p, const vector<uint64_t> &q)
{
    const int M = 256, H = 12, W = 12;
    auto ints = [&](const char *file) { const auto raw = rd(dir + "/" + file); return vector<int64_t>(raw.begin(), raw.end()); };
    const vector<int64_t> img = ints("image.i64"), w1 = ints("w1.i64"), w2 = ints("w2.i64");
    SlotPlanes g1 = planesOf(H, W, M);
    g1.fh = 3; g1.fw = 3; g1.pool = 2;
    setParameters(n, q, (uint64_t)1 << 20, 0);
    { ciphertext3D none(1, 1, 1, 1); thrown("no_batching_conv", [&] { convSlots(none, w1, 2, g1); }); }
    thrown("no_slot_encoding", [&] { encryptImagePlanes(img, 1, H, W, M); });
    setParameters(n, q, p[2], 0);
    setSlotEncoding(0, 0);
    const ciphertext3D x = encryptImagePlanes(img, 1, H, W, M);
    thrown("no_keys_conv", [&] { convSlots(x, w1, 2, g1); });
    SlotPlanes g2, g3;
    {                                                                   // the second layer's geometry is the first one's output: known from the plan alone
        ConvSlotsPlan P1;
        if (!crc_conv_slots_plan(n, M, W, H, W, 3, 3, 1, 2, P1)) return 5;
        g2 = planesOf(H, W, M); g2.H = P1.out_h; g2.W = P1.out_w; g2.dil = P1.out_dil; g2.fh = 3; g2.fw = 3;
    }
    vector<uint64_t> elts = convSlotsElements(g1);
    for (uint64_t e : convSlotsElements(g2)) if (find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e);
    generateGaloisKeys(16, elts);
    const vector<vector<int64_t>> x0{img}, y1 = conv_int(x0, H, W, w1, 2, 3, 3, 2), y2 = conv_int(y1, g2.H, g2.W, w2, 3, 3, 3, 1);
    planes("conv_fresh", x, planesOf(H, W, M), x0);
    SlotPlanes o1;
    const ciphertext3D c1 = convSlots(x, w1, 2, g1, &o1);
    if (o1.H != g2.H || o1.W != g2.W || o1.dil != g2.dil || o1.pitch != g2.pitch || o1.M != M) return 6;
    planes("conv_1", c1, o1, y1);
    const ciphertext3D c2 = convSlots(c1, w2, 3, g2, &g3);
    planes("conv_2", c2, g3, y2);
    { const ciphertext3D n1 = convSlots(x, w1, 2, g1, nullptr, CRC_NTT); planes("conv_2_ntt", convSlots(n1, w2, 3, g2, nullptr, CRC_NTT), g3, y2); }
    printf("keys conv %zu elements %zu\n", elts.size() * crc_evk_words(context, 16) * 8, elts.size());
    thrown("bad_weights", [&] { convSlots(x, w2, 2, g1); });
    thrown("bad_M_conv", [&] { SlotPlanes b = g1; b.M = 96; convSlots(x, w1, 2, b); });
    thrown("plane_does_not_fit", [&] { SlotPlanes b = g1; b.M = 128; convSlots(x, w1, 2, b); });
    thrown("missing_key_conv", [&] { SlotPlanes b = g1; b.pool = 3; convSlots(x, vector<int64_t>(2 * 9, 1), 2, b); });       // a 5 x 5 window: taps without keys
    thrown("bad_form_conv", [&] { convSlots(x, w1, 2, g1, nullptr, CRC_NTTP); });
    thrown("not_planes", [&] { convSlots(ciphertext3D(1, 1, 2, 1), vector<int64_t>(2 * 9, 1), 2, g1); });
    thrown("plane_too_large", [&] { encryptImagePlanes(vector<int64_t>(17 * 17, 1), 1, 17, 17, M); });
    delParameters();
    clearDeterministicSeed();
    printf("hoist_host conv ok\n");
    return 0;
}

// [Cin][H][W] -> [Cout][oh][ow]: `pad` zero pixels on every side, stride `stride`, w [Cout][Cin][fh][fw], + bias[co] where one is given; exact integers
static vector<vector<int64_t>> conv_pad_int(const vector<vector<int64_t>> &x, int H, int W, const vector<int64_t> &w, int Cout, int fh, int fw, int pad, int stride,
                                            const vector<int64_t> &bias)
{
    const int Cin = (int)x.size(), oh = (H + 2 * pad - fh) / stride + 1, ow = (W + 2 * pad - fw) / stride + 1;
    vector<vector<int64_t>> y(Cout, vector<int64_t>((size_t)oh * ow, 0));
    for (int co = 0; co < Cout; co++) for (int r = 0; r < oh; r++) for (int c = 0; c < ow; c++) {
        int64_t acc = bias.empty() ? 0 : bias[co];
        for (int ci = 0; ci < Cin; ci++) for (int a = 0; a < fh; a++) for (int b = 0; b < fw; b++) {
            const int iy = stride * r + a - pad, ix = stride * c + b - pad;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) acc += w[(((size_t)co * Cin + ci) * fh + a) * fw + b] * x[ci][(size_t)iy * W + ix];
        }
        y[co][(size_t)r * ow + c] = acc;
    }
    return y;
}
static int convpad_case(const vector<uint64_t> &p, const vector<uint64_t> &q)
{
    const int M = 256, H = 12, W = 12, margin = 1;
    auto ints = [&](const char *file) { const auto raw = rd(dir + "/" + file); return vector<int64_t>(raw.begin(), raw.end()); };
    const vector<int64_t> img = ints("image.i64"), w1 = ints("w1.i64"), b1 = ints("b1.i64"), w2 = ints("w2.i64");
    setParameters(n, q, p[2], 0);
    setSlotEncoding(0, 0);
    SlotPlanes g1 = planesOf(H, W, M, margin);
    if (g1.pitch != 13 || g1.origin != 14 || g1.stride != 1 || g1.pad != 0 || g1.pool_stride != 0) return 5;
    g1.fh = 3; g1.fw = 3; g1.pad = 1;
    const ciphertext3D x = encryptImagePlanes(img, 1, H, W, M, margin, CRC_COEFF);
    SlotPlanes g2 = planesOf(H, W, M, margin);                          // a 'same' layer: the second one sees the first one's geometry
    g2.fh = 3; g2.fw = 3; g2.pad = 1; g2.stride = 2;
    vector<uint64_t> elts = convSlotsElements(g1);
    for (uint64_t e : convSlotsElements(g2)) if (find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e);
    generateGaloisKeys(16, elts);
    const vector<vector<int64_t>> x0{img}, y1 = conv_pad_int(x0, H, W, w1, 2, 3, 3, 1, 1, b1), y2 = conv_pad_int(y1, H, W, w2, 3, 3, 3, 1, 2, {});
    planes("convpad_fresh", x, planesOf(H, W, M, margin), x0);
    {                                                                   // the fresh tensor is clean: zeros around the plane
        const vector<vector<int64_t>> v = decryptSlots(x, n);
        const vector<int> in = densePlanesInSlots(planesOf(H, W, M, margin));
        bool clean = true;
        for (int i = 0; i < n; i++) if (find(in.begin(), in.end(), i % M) == in.end()) clean = clean && v[i][0] == 0;
        printf("clean convpad_fresh %s\n", clean ? "yes" : "no");
    }
    SlotPlanes o1, g3;
    const ciphertext3D c1 = convSlots(x, w1, 2, g1, b1, true, &o1);
    if (o1.H != H || o1.W != W || o1.dil != 1 || o1.pitch != g1.pitch || o1.origin != g1.origin || o1.M != M || o1.pad != 0) return 6;
    planes("convpad_1", c1, o1, y1);
    {
        const vector<vector<int64_t>> v = decryptSlots(c1, n);          // [n][2]
        const vector<int> in = densePlanesInSlots(o1);
        bool clean = true;
        for (int i = 0; i < n; i++) if (find(in.begin(), in.end(), i % M) == in.end()) clean = clean && v[i][0] == 0 && v[i][1] == 0;
        printf("clean convpad_1 %s\n", clean ? "yes" : "no");
    }
    printf("budget convpad_1_unmasked %d\n", minNoiseBudget(convSlots(x, w1, 2, g1, b1, false)));
    const ciphertext3D c2 = convSlots(c1, w2, 3, g2, &g3);
    if (g3.H != 6 || g3.W != 6 || g3.dil != 2 || g3.origin != g1.origin) return 7;
    planes("convpad_2", c2, g3, y2);
    { const ciphertext3D n1 = convSlots(x, w1, 2, g1, b1, true, nullptr, CRC_NTT); planes("convpad_2_ntt", convSlots(n1, w2, 3, g2, nullptr, CRC_NTT), g3, y2); }
    printf("keys convpad %zu elements %zu\n", elts.size() * crc_evk_words(context, 16) * 8, elts.size());
    thrown("bad_bias", [&] { convSlots(x, w1, 2, g1, vector<int64_t>(3, 1), true); });
    thrown("too_little_margin", [&] { SlotPlanes b = g1; b.pad = 2; convSlots(x, w1, 2, b, b1, true); });
    thrown("pad_without_margin", [&] { SlotPlanes b = planesOf(16, 16, M); b.fh = 3; b.fw = 3; b.pad = 1; convSlotsElements(b); });
    thrown("negative_margin", [&] { encryptImagePlanes(img, 1, H, W, M, -1, CRC_COEFF); });
    thrown("margin_too_large", [&] { encryptImagePlanes(img, 1, H, W, M, 4, CRC_COEFF); });      // 16 . 16 + 4 slots
    thrown("bad_stride", [&] { SlotPlanes b = g1; b.stride = 0; convSlots(x, w1, 2, b, b1, true); });
    delParameters();
    clearDeterministicSeed();
    printf("hoist_host convpad ok\n");
    return 0;
}

// every slot of y against `want` at out_slots of every period M and 0 elsewhere: "planes <name> equal|differs"
static void vector_slots(const char *name, const ciphertext3D &y, int M, const vector<int> &out_slots, const vector<int64_t> &want, int64_t t)
{
    printf("budget %s %d\n", name, minNoiseBudget(y));
    const vector<vector<int64_t>> got = decryptSlots(y, n);
    vector<int64_t> expect((size_t)M, 0);
    for (size_t o = 0; o < out_slots.size(); o++) {
        int64_t w = (want[o] % t + t) % t;
        expect[out_slots[o]] = w > (t - 1) / 2 ? w - t : w;
    }
    bool equal = true;
    for (int i = 0; i < n; i++) equal = equal && got[i][0] == expect[i % M];
    const vector<vector<int64_t>> v = decryptVector(y, out_slots);
    for (size_t o = 0; o < out_slots.size(); o++) equal = equal && v[0][o] == expect[out_slots[o]];
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    for (int i = 0; i < M; i++) f.write((const char *)&got[i][0], 8);
    printf("planes %s %s\n", name, equal ? "equal" : "differs");
}
static int planes_case(const vector<uint64_t> &p, const vector<uint64_t> &q)
{
    const int M = 256, H = 12, W = 12;
    const int64_t t = (int64_t)p[2];
    auto ints = [&](const char *file) { const auto raw = rd(dir + "/" + file); return vector<int64_t>(raw.begin(), raw.end()); };
    const vector<int64_t> img = ints("image.i64"), w1 = ints("w1.i64"), w3 = ints("w3.i64"), w4 = ints("w4.i64");
    SlotPlanes g1 = planesOf(H, W, M);
    g1.fh = 3; g1.fw = 3; g1.pool = 2;
    setParameters(n, q, (uint64_t)1 << 20, 0);
    { ciphertext3D none(1, 1, 1, 1); thrown("no_batching_planes", [&] { densePlanes(none, w4, 3, M, {0, 1, 2, 3, 4, 5}); }); }
    setParameters(n, q, p[2], 0);
    setSlotEncoding(0, 0);
    const ciphertext3D x = encryptImagePlanes(img, 1, H, W, M);
    ConvSlotsPlan P1;
    if (!crc_conv_slots_plan(n, M, W, H, W, 3, 3, 1, 2, P1)) return 5;
    SlotPlanes o1 = planesOf(H, W, M);
    o1.H = P1.out_h; o1.W = P1.out_w; o1.dil = P1.out_dil;
    if (densePlanesInSlots(o1) != crc_dense_planes_in_slots(P1)) return 6;
    vector<int> out1, out2{0, 2, 4};
    for (int a = 0; a < 2; a++) for (int b = 0; b < 3; b++) out1.push_back(2 * (12 * a + b));
    vector<uint64_t> elts = convSlotsElements(g1);
    const vector<uint64_t> e1 = densePlanesElements(o1, 6, out1), e2 = densePlanesElements(M, out1, 3, out2);
    for (uint64_t e : e1) if (find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e);
    for (uint64_t e : e2) if (find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e);
    const ciphertext3D c0 = [&] { generateGaloisKeys(16, convSlotsElements(g1)); return convSlots(x, w1, 2, g1); }();
    thrown("missing_key_planes", [&] { densePlanes(c0, w3, 6, o1, out1); });             // the conv's keys alone
    generateGaloisKeys(16, elts);
    const vector<vector<int64_t>> y1 = conv_int({img}, H, W, w1, 2, 3, 3, 2);
    vector<int64_t> v1(6, 0), v2(3, 0);
    for (int o = 0; o < 6; o++) for (int c = 0; c < 2; c++) for (int i = 0; i < 25; i++) v1[o] += w3[((size_t)o * 2 + c) * 25 + i] * y1[c][i];
    for (int o = 0; o < 3; o++) for (int i = 0; i < 6; i++) v2[o] += w4[(size_t)o * 6 + i] * v1[i];
    const ciphertext3D c1 = convSlots(x, w1, 2, g1);
    const ciphertext3D d1 = densePlanes(c1, w3, 6, o1, out1);
    vector_slots("dense_1", d1, M, out1, v1, t);
    const size_t prepared = preparedGaloisKeyBytes();
    const ciphertext3D d2 = densePlanes(d1, w4, 3, M, out1, out2);
    vector_slots("dense_2", d2, M, out2, v2, t);
    if (preparedGaloisKeyBytes() != prepared) return 7;                                  // (made once, kept)
    {
        const ciphertext3D n1 = convSlots(x, w1, 2, g1, nullptr, CRC_NTT), n2 = densePlanes(n1, w3, 6, o1, out1, CRC_NTT);
        vector_slots("dense_2_ntt", densePlanes(n2, w4, 3, M, out1, out2, CRC_NTT), M, out2, v2, t);
    }
    printf("steps conv %zu dense_1 %zu dense_2 %zu\n", P1.steps.size(), e1.size() + 1, e2.size() + 1);
    printf("keys planes %zu prepared %zu elements %zu\n", elts.size() * crc_evk_words(context, 16) * 8, prepared, elts.size());
    thrown("bad_weights_planes", [&] { densePlanes(c1, w4, 6, o1, out1); });
    thrown("bad_M_planes", [&] { densePlanes(d1, w4, 3, 96, out1, out2); });
    thrown("duplicate_slot", [&] { densePlanes(d1, w4, 3, M, out1, {0, 2, 2}); });
    thrown("slot_outside_M", [&] { densePlanes(d1, w4, 3, M, out1, {0, 2, 256}); });
    thrown("wrong_output_count", [&] { densePlanes(d1, w4, 3, M, out1, {0, 2}); });
    thrown("bad_form_planes", [&] { densePlanes(d1, w4, 3, M, out1, out2, CRC_NTTP); });
    thrown("not_planes_dense", [&] { densePlanes(ciphertext3D(1, 1, 2, 1), w4, 3, M, out1, out2); });
    thrown("no_slots", [&] { decryptVector(d2, {}); });
    delParameters();
    clearDeterministicSeed();
    printf("hoist_host planes ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: hoist_host <dir> [bsgs | conv | planes | convpad]\n"); return 1; }
    try {
        dir = argv[1];
        setDeterministicSeed(20241019);
        const auto p = rd(dir + "/params.u64");
        n = (int)p[0]; const int k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        if (argc > 2 && string(argv[2]) == "bsgs") return bsgs_case(p, q);
        if (argc > 2 && string(argv[2]) == "conv") return conv_case(p, q);
        if (argc > 2 && string(argv[2]) == "planes") return planes_case(p, q);
        if (argc > 2 && string(argv[2]) == "convpad") return convpad_case(p, q);
        const vector<vector<int64_t>> W8 = matrix(dir + "/w8.i64", 8, 8), W5 = matrix(dir + "/w5.i64", 5, 8);
        // a plain modulus without slots: the reference's logic_error, before any key is looked at
        setParameters(n, q, (uint64_t)1 << 20, 0);
        {
            ciphertext3D none(1, 1, 1, 1);
            thrown("no_batching_many", [&] { rotateRowsMany(none, {1}); });
            thrown("no_batching_matvec", [&] { matvecSlots(none, W8, 8); });
        }
        setParameters(n, q, p[2], 0);
        setSlotEncoding(0, 0);
        const auto raw = rd(dir + "/values.i64");
        const size_t P = raw.size() / n;
        vector<vector<int64_t>> images(n, vector<int64_t>(P));
        for (int j = 0; j < n; j++) for (size_t c = 0; c < P; c++) images[j][c] = (int64_t)raw[(size_t)j * P + c];
        const ciphertext3D x = encryptImageSlots(images, 1, 1, (int)P);
        thrown("no_keys_many", [&] { rotateRowsMany(x, {1}); });
        thrown("no_keys_matvec", [&] { matvecSlots(x, W8, 8); });
        vector<uint64_t> elts;
        for (int d = 1; d < 8; d++) elts.push_back(crc_galois_elt_rows(context, d));
        generateGaloisKeys(16, elts);
        put("fresh", x);
        {
            const vector<ciphertext3D> r = rotateRowsMany(x, {0, 1, 5, 7});
            put("many_0", r[0]); put("many_1", r[1]); put("many_5", r[2]); put("many_7", r[3]);
        }
        { ciphertext3D xn = rotateRowsMany(x, {0}, CRC_NTT)[0]; put("many_5_ntt", rotateRowsMany(xn, {5}, CRC_NTT)[0]); }
        put("rows_1", rotateRows(x, 1));
        put("rows_5", rotateRows(x, 5));
        put("matvec_8x8", matvecSlots(x, W8, 8));
        put("matvec_5x8", matvecSlots(x, W5, 8));
        { ciphertext3D xn = rotateRowsMany(x, {0}, CRC_NTT)[0]; put("matvec_8x8_ntt", matvecSlots(xn, W8, 8, CRC_NTT)); }
        put("matvec_zero", matvecSlots(x, vector<vector<int64_t>>(8, vector<int64_t>(8, 0)), 8));
        printf("empty %zu\n", rotateRowsMany(x, {}).size());
        thrown("steps_too_large", [&] { rotateRowsMany(x, {1, n / 2}); });
        thrown("missing_key_many", [&] { rotateRowsMany(x, {1, 9}); });                 // 3^9 has no key of its own: no chain is planned
        thrown("bad_M", [&] { matvecSlots(x, W8, 6); });
        thrown("M_too_large", [&] { matvecSlots(x, W8, n); });
        thrown("W_too_large", [&] { matvecSlots(x, W8, 4); });
        {
            vector<vector<int64_t>> W16(16, vector<int64_t>(16, 0));
            W16[0][9] = 1;                                                              // diagonal 9: the key of 3^9 is absent
            thrown("missing_key_matvec", [&] { matvecSlots(x, W16, 16); });
        }
        thrown("bad_form", [&] { rotateRowsMany(x, {1}, CRC_NTTP); });
        delParameters();
        clearDeterministicSeed();
        printf("hoist_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "hoist_host: %s\n", e.what()); return 4; }
}
