// abi.hip -- extern "C" entry points of include/crcnn_hip.h that drive the kernels (layers and Evaluator ops).
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels.h"
#include "chacha.h"
#include "work_arena.h"

// every device entry point makes its context's GPU current for the calling thread (a no-op in the one-process-per-GPU flow; in a one-process, many-GPU
// application the launch must not land on whatever device the thread used last)
#define CHECK_CTX(c) do { if (!(c) || (c)->device < 0) return CRC_ERR_INVALID_ARGUMENT; \
        int dev_ = -1; if (hipGetDevice(&dev_) != hipSuccess || dev_ != (c)->device) HIPCHK(hipSetDevice((c)->device)); } while (0)
#define RUN(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
static inline hipStream_t S(void *s) { return (hipStream_t)s; }
static inline bool form_ok(int f) { return f == CRC_COEFF || f == CRC_NTT; }
static inline bool nform_ok(int f) { return f == CRC_COEFF || f == CRC_NTT || f == CRC_NTTP; }
static inline bool lform_ok(int f) { return nform_ok(f) || f == CRC_NTTL; }
static inline bool limb_in(int f) { return f == CRC_NTTL || f == CRC_NTTLS; }          // the input already is the kernel's operand
// entry points whose work space is one region: its start in d_work, and the size of `words` of it
static inline u64 *work_base(void *d_work) { return WorkArena(d_work).take<u64>(0); }
static inline size_t work_bytes(size_t words) { WorkArena a; a.take<u64>(words); return a.bytes(); }

extern "C" int crc_plain_to_ntt(crc_ctx *c, const uint64_t *d_plain, size_t count, uint64_t *d_out, void *stream)
{
    CHECK_CTX(c); if (!d_plain || !d_out) return CRC_ERR_INVALID_ARGUMENT;
    return k_plain_ntt(c, d_plain, count, 1, true, d_out, S(stream));
}
extern "C" int crc_plain_expand(crc_ctx *c, const uint64_t *d_compact, size_t count, uint64_t *d_plain, void *stream)
{
    CHECK_CTX(c); if (!d_compact || !d_plain) return CRC_ERR_INVALID_ARGUMENT;
    return k_plain_expand(c, d_compact, count, d_plain, S(stream));
}
extern "C" int crc_plain_to_delta(crc_ctx *c, const uint64_t *d_plain, size_t count, int form, uint64_t *d_out, void *stream)
{
    CHECK_CTX(c); if (!d_plain || !d_out || !form_ok(form)) return CRC_ERR_INVALID_ARGUMENT;
    return k_plain_ntt(c, d_plain, count, 2, form == CRC_NTT, d_out, S(stream));
}

extern "C" int crc_ntt_fwd(crc_ctx *c, uint64_t *d_ct, size_t count, int size, void *stream)
{
    CHECK_CTX(c); if (!d_ct || size < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_ntt_ct(c, false, d_ct, d_ct, count, size, false, S(stream), nullptr, 0, 0);
}
// forward NTT of the bxf x byf window sums (dilation (xs, ys)) of B images of xd x yd coefficient-form size-2 ciphertexts: [B][xdo][ydo] NTT-form ciphertexts,
// out of place (kernels.hip k_ntt_ct_box)
extern "C" int crc_ntt_fwd_box(crc_ctx *c, const uint64_t *d_src, uint64_t *d_dst, int B, int xd, int yd, int bxf, int byf, int xs, int ys, void *stream)
{
    CHECK_CTX(c); if (!d_src || !d_dst) return CRC_ERR_INVALID_ARGUMENT;
    return k_ntt_ct_box(c, d_src, d_dst, B, xd, yd, bxf, byf, xs, ys, S(stream));
}
extern "C" int crc_ntt_inv(crc_ctx *c, uint64_t *d_ct, size_t count, int size, void *stream)
{
    CHECK_CTX(c); if (!d_ct || size < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_ntt_ct(c, true, d_ct, d_ct, count, size, false, S(stream), nullptr, 0, 0);
}
extern "C" int crc_ntt_fwd_bsk(crc_ctx *c, uint64_t *d_rows, size_t count, void *stream)
{
    CHECK_CTX(c); if (!d_rows) return CRC_ERR_INVALID_ARGUMENT;
    return k_ntt_ct(c, false, d_rows, d_rows, count, 1, true, S(stream), nullptr, 0, 0);
}
extern "C" int crc_ntt_inv_bsk(crc_ctx *c, uint64_t *d_rows, size_t count, void *stream)
{
    CHECK_CTX(c); if (!d_rows) return CRC_ERR_INVALID_ARGUMENT;
    return k_ntt_ct(c, true, d_rows, d_rows, count, 1, true, S(stream), nullptr, 0, 0);
}

extern "C" int crc_add(crc_ctx *c, uint64_t *d_acc, const uint64_t *d_b, size_t count, int size, void *stream)
{
    CHECK_CTX(c); if (!d_acc || !d_b || size < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_rowwise(c, d_acc, d_b, count, size, 0, 1, 1, 0, S(stream));
}
extern "C" int crc_add_plain(crc_ctx *c, uint64_t *d_ct, const uint64_t *d_delta, size_t count, size_t group, int sign, void *stream)
{
    CHECK_CTX(c); if (!d_ct || !d_delta || (sign != 1 && sign != -1)) return CRC_ERR_INVALID_ARGUMENT;
    return k_rowwise(c, d_ct, d_delta, count, 2, 1, sign, group, 0, S(stream));
}
extern "C" int crc_multiply_plain_ntt(crc_ctx *c, uint64_t *d_ct, const uint64_t *d_w, size_t count, size_t group, int size, void *stream)
{
    CHECK_CTX(c); if (!d_ct || !d_w || size < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_rowwise(c, d_ct, d_w, count, size, 2, 1, group, 0, S(stream));
}
extern "C" int crc_multiply_plain(crc_ctx *c, uint64_t *d_ct, const uint64_t *d_w, size_t count, size_t group, void *stream)
{
    CHECK_CTX(c); if (!d_ct || !d_w) return CRC_ERR_INVALID_ARGUMENT;
    // (the dyadic product in the last loop of the forward transform where the ring has the wave-local kernel, else as a pass of its own)
    const int rc = k_ntt_ct_fwd_mul(c, d_ct, count, d_w, group, S(stream));
    if (rc == CRC_ERR_UNSUPPORTED) {
        RUN(k_ntt_ct(c, false, d_ct, d_ct, count, 2, false, S(stream), nullptr, 0, 0));
        RUN(k_rowwise(c, d_ct, d_w, count, 2, 2, 1, group, 0, S(stream)));
    } else if (rc) return rc;
    return k_ntt_ct(c, true, d_ct, d_ct, count, 2, false, S(stream), nullptr, 0, 0);
}

// ---- convolution / dense ------------------------------------------------------------------------------------------
// (window geometry: window.h.  Every entry point builds its Window / LayerShape once from its integer parameters and checks it before anything divides by a stride)
// Work of a layer on the vector-ALU kernels: [offsets of the P outputs][offsets of the T (+ 8) taps, in ciphertexts and in words][NTT copy of a coefficient-form input]
struct ConvWork { int *xoff, *toff; unsigned *toffw; u64 *buf; };
static ConvWork conv_layout(const crc_ctx *c, int B, const LayerShape &s, int in_form, WorkArena &a)
{
    const size_t T = (size_t)s.zd * s.w.xf * s.w.yf;
    ConvWork L{};
    L.xoff = a.take<int>(s.w.P()); L.toff = a.take<int>(T + 8); L.toffw = a.take<unsigned>(T + 8);
    if (in_form == CRC_COEFF) L.buf = a.take<u64>((size_t)B * s.zd * s.w.xd * s.w.yd * crc_ct_words(c, 2));
    return L;
}

// ---- limb form (CRC_NTTL): the layer on the matrix cores (kernels_mfma.hip) ------------------------------------------------------------
extern "C" int crc_limb_supported(const crc_ctx *c, int zd, int xf, int yf)
{
    if (!c || zd < 1 || xf < 1 || yf < 1) return 0;
    return k_limb_supported(c, k_limb_steps(zd, xf, yf) * 32) ? 1 : 0;
}
extern "C" size_t crc_limb_tensor_bytes(const crc_ctx *c, int B, int zd, int xd, int yd) { return c ? k_limb_tensor_bytes(c, B, zd, xd * yd) : 0; }
extern "C" size_t crc_limb_weights_bytes(const crc_ctx *c, int nf, int zd, int xf, int yf) { return c ? k_limb_weights_bytes(c, nf, zd, xf, yf) : 0; }
extern "C" int crc_limb_pack_weights(crc_ctx *c, const uint64_t *d_w_ntt, int nf, int zd, int xf, int yf, void *d_wl, void *stream)
{
    CHECK_CTX(c); if (!d_w_ntt || !d_wl || nf < 1 || zd < 1 || xf < 1 || yf < 1) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_limb_supported(c, zd, xf, yf)) return CRC_ERR_UNSUPPORTED;
    return k_limb_pack_weights(c, d_w_ntt, (signed char *)d_wl, nf, zd, xf, yf, S(stream));
}
extern "C" int crc_limb_pack_weights_tile(crc_ctx *c, const uint64_t *d_w_tile_ntt, int nf, int f0, int ft, int zd, int xf, int yf, void *d_wl, void *stream)
{
    CHECK_CTX(c); if (!d_w_tile_ntt || !d_wl || nf < 1 || zd < 1 || xf < 1 || yf < 1 || f0 < 0 || ft < 1 || f0 + ft > nf) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_limb_supported(c, zd, xf, yf)) return CRC_ERR_UNSUPPORTED;
    return k_limb_pack_weights(c, d_w_tile_ntt, (signed char *)d_wl, nf, zd, xf, yf, S(stream), f0, ft);
}
extern "C" int crc_limb_pack_tensor(crc_ctx *c, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, void *d_xl, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_xl || B < 0 || zd < 1 || xd < 1 || yd < 1 || (in_form != CRC_NTT && in_form != CRC_NTTP)) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_limb_supported(c, zd, 1, 1)) return CRC_ERR_UNSUPPORTED;
    return k_limb_pack_tensor(c, d_x, (signed char *)d_xl, B, zd, xd * yd, in_form == CRC_NTTP, S(stream));
}
extern "C" int crc_limb_pack_tensor_at(crc_ctx *c, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, void *d_xl, int Btot, int b0, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_xl || B < 0 || zd < 1 || xd < 1 || yd < 1 || Btot < B || b0 < 0 || b0 + B > Btot || (in_form != CRC_NTT &&
        in_form != CRC_NTTP)) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_limb_supported(c, zd, 1, 1)) return CRC_ERR_UNSUPPORTED;
    return k_limb_pack_tensor(c, d_x, (signed char *)d_xl, B, zd, xd * yd, in_form == CRC_NTTP, S(stream), Btot, b0);
}
// one-channel convolutions (CRC_NTTL1, kernels_mfma1.hip)
extern "C" int crc_limb_conv1_supported(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf)
{
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    if (!c || nf < 1 || !s.w.ok()) return 0;
    return k_limb_conv1_shape(c, s) ? 1 : 0;
}
extern "C" size_t crc_limb_conv1_weights_bytes(const crc_ctx *c) { return c ? k_limb_conv1_weights_bytes(c) : 0; }
extern "C" size_t crc_limb_conv1_weights_bytes_for(const crc_ctx *c, int nf, int xf, int yf)
{
    return c && nf >= 1 && xf >= 1 && yf >= 1 ? k_limb_conv1_weights_bytes_for(c, nf, xf, yf) : 0;
}
// which form of the kernel a shape runs under the present tuning: 0 not a one-channel matrix-core shape, 1 plane-major, 2 pixel-major
extern "C" int crc_limb_conv1_form(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf)
{
    return crc_limb_conv1_supported(c, zd, xd, yd, xs, ys, xf, yf, nf) ? k_limb_conv1_form(c, xf, yf, nf) : 0;
}
extern "C" int crc_limb_conv1_pack_weights(crc_ctx *c, const uint64_t *d_w_ntt, int nf, int xf, int yf, void *d_wl, void *stream)
{
    CHECK_CTX(c); if (!d_w_ntt || !d_wl || nf < 1 || nf > 32 || xf < 1 || yf < 1 || xf > 8 || yf > 8) return CRC_ERR_INVALID_ARGUMENT;
    if (!k_limb_supported(c, 64)) return CRC_ERR_UNSUPPORTED;
    return k_limb_conv1_pack_weights(c, d_w_ntt, (signed char *)d_wl, nf, xf, yf, S(stream));
}
// images per internal pass: the y-expanded limb images and the slot-major result of a pass stay below ~16 GiB of work space (a dense consumer's flattened
// limb tensor is converted from the whole batch's result at once: no sub-batching there)
static int conv1_sub_batch(const crc_ctx *c, int B, const Window &w, int nf, int out_form)
{
    if (out_form == CRC_NTTL || B <= 1) return B;
    const size_t per = k_limb_conv1_image_bytes(c, 1, w, nf) + (out_form == CRC_NTTLC ? 0 : 8 * k_limb_result_words(c, 1, nf, w.P()));
    const long long ev = c->tune.conv1_pass_bytes;                   // (the tests shrink it to cover the multi-pass path at small sizes: crc_ctx_set_tuning)
    const size_t cap = ev > 0 ? (size_t)ev : (size_t)16 << 30;
    const size_t fit = cap / (per ? per : 1);
    return (int)(fit < 1 ? 1 : fit > (size_t)B ? (size_t)B : fit);
}
// Work of a one-channel layer, for a pass of Bs images: [y-expanded limb images][slot-major result (not where the kernel writes the limb tensor itself)][NTT copy
// of a coefficient-form sub-batch].  out_form: the form the passes produce.  in: the window on the input image; the kernel reads in.boxed(bxf, byf) (the box sums of a
// boxed layer, crc_conv2d_box_forms; the input itself otherwise)
struct Limb1Work { signed char *Xr; u64 *Ys, *buf; int Bs, out_form; };
static Limb1Work limb1_layout(const crc_ctx *c, int B, const Window &in, int bxf, int byf, int nf, int in_form, int out_form, WorkArena &a)
{
    const Window w = in.boxed(bxf, byf);
    const int P = w.P();
    Limb1Work L{};
    // a 1 x 1 result is a dense layer's input: the K-blocked form (kernels_mfma.hip), made from the slot-major result
    L.out_form = out_form == CRC_NTTLC && P == 1 ? CRC_NTTL : out_form;
    L.Bs = conv1_sub_batch(c, B, w, nf, L.out_form);
    L.Xr = a.take<signed char>(k_limb_conv1_image_bytes(c, L.Bs, w, nf));
    if (L.out_form != CRC_NTTLC) L.Ys = a.take<u64>(k_limb_result_words(c, L.Bs, nf, P));
    // (the boxed transform of conv2d_limb1 fills only Bs xdo ydo ciphertexts of it: the size does not depend on which path the call takes)
    if (in_form == CRC_COEFF) L.buf = a.take<u64>((size_t)L.Bs * in.xd * in.yd * crc_ct_words(c, 2));
    return L;
}
static int conv2d_limb1(crc_ctx *c, const uint64_t *d_x, const void *d_wl, const uint64_t *d_bias, int B, const Window &in, int nf, int in_form, int out_form,
                        uint64_t *d_y, void *d_work, hipStream_t st, int bxf = 1, int byf = 1)
{
    const int P = in.boxed(bxf, byf).P(), in_cts = in.xd * in.yd;
    WorkArena a(d_work);
    const Limb1Work L = limb1_layout(c, B, in, bxf, byf, nf, in_form, out_form, a);
    out_form = L.out_form;
    const size_t ctw = crc_ct_words(c, 2);
    // a coefficient-form input under a box: the window sums are taken while the input transform loads (k_ntt_ct_box: NTT(sum) = sum NTT mod q, bit for bit), 14 %
    // fewer rows transformed for PlainModelTiny's 2 x 2 box, and the pack runs its unboxed body on the summed image.  box_ntt = 0 or a ring without that kernel:
    // transform every input, then the boxed pack, as NTT-form inputs do
    const bool sum_first = in_form == CRC_COEFF && bxf * byf > 1 && c->tune.box_ntt != 0 && k_ntt_ct_box_supported(c, bxf, byf);
    const Window wsum = in.boxed(bxf, byf);
    for (int b0 = 0; b0 < B; b0 += L.Bs) {
        const int Bn = B - b0 < L.Bs ? B - b0 : L.Bs;
        const u64 *xn = d_x + (size_t)b0 * in_cts * ctw; bool packed = in_form == CRC_NTTP;
        if (sum_first) RUN(k_ntt_ct_box(c, xn, L.buf, Bn, in.xd, in.yd, bxf, byf, in.xs, in.ys, st));
        else if (in_form == CRC_COEFF) RUN(k_ntt_ct(c, false, xn, L.buf, (size_t)Bn * in_cts, 2, false, st, nullptr, 0, 0, 0, 0));
        if (in_form == CRC_COEFF) { xn = L.buf; packed = false; }
        RUN(k_limb_conv1(c, xn, packed, L.Xr, (const signed char *)d_wl, L.Ys, out_form == CRC_NTTLC ? (signed char *)d_y : nullptr, B, b0,
            out_form != CRC_COEFF ? d_bias : nullptr, Bn, sum_first ? wsum : in, nf, st, sum_first ? 1 : bxf, sum_first ? 1 : byf));
        if (out_form == CRC_NTTLC) continue;
        if (out_form == CRC_NTTL) return k_limb_result_to_limb(c, L.Ys, (signed char *)d_y, B, nf * P, st);     // (Bs == B)
        RUN(k_limb_result_to_rows(c, L.Ys, d_y + (size_t)b0 * nf * P * ctw, (size_t)Bn * nf * P * 2, out_form == CRC_NTTP, st));
    }
    if (out_form == CRC_COEFF) RUN(k_ntt_ct(c, true, d_y, d_y, (size_t)B * nf * P, 2, false, st, d_bias, 1, (size_t)P, nf));
    return CRC_OK;
}
// Work of a layer on the limb GEMM: [slot-major result][limb form of a canonical or packed input][NTT copy of a coefficient-form input]
struct LimbWork { u64 *Ys; signed char *Xl; u64 *buf; };
static LimbWork limb_layout(const crc_ctx *c, int B, const LayerShape &s, int in_form, WorkArena &a)
{
    LimbWork L{};
    L.Ys = a.take<u64>(k_limb_result_words(c, B, s.nf, s.w.P()));
    if (!limb_in(in_form)) L.Xl = a.take<signed char>(k_limb_tensor_bytes(c, B, s.zd, s.w.xd * s.w.yd));
    if (in_form == CRC_COEFF) L.buf = a.take<u64>((size_t)B * s.zd * s.w.xd * s.w.yd * crc_ct_words(c, 2));
    return L;
}
extern "C" size_t crc_conv2d_forms_work_bytes(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int in_form,
    int w_form, int out_form)
{
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    if (!c || !s.w.ok()) return 0;
    WorkArena a;
    if (w_form == CRC_NTTL1) limb1_layout(c, B, s.w, 1, 1, nf, in_form, out_form, a);
    else if (w_form == CRC_NTTL || w_form == CRC_NTTLS) limb_layout(c, B, s, in_form, a);
    else conv_layout(c, B, s, in_form, a);
    return a.bytes();
}
extern "C" size_t crc_conv2d_work_bytes(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int in_form)
{
    return crc_conv2d_forms_work_bytes(c, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, CRC_NTT, CRC_COEFF);
}
static int conv2d_limb(crc_ctx *c, const uint64_t *d_x, const void *d_wl, const uint64_t *d_bias, int B, const LayerShape &s, int in_form, int out_form,
                       uint64_t *d_y, void *d_work, hipStream_t st, bool scalar = false)
{
    const int zd = s.zd, nf = s.nf, npos = s.w.xd * s.w.yd;
    // scalar (w_form = CRC_NTTLS): the same steps on the merged GEMM of a modulus.  A convolution's tensor is the same bytes in either form; a dense layer's
    // (in_form / out_form = CRC_NTTLS) has its rows in image order e = s B + b.  Ys is the same bytes too, so every other out_form goes the way it always went
    if (!(scalar ? k_scalar_supported(c, B, s) : crc_limb_supported(c, zd, s.w.xf, s.w.yf) != 0)) return CRC_ERR_UNSUPPORTED;
    const int P = s.w.P(), in_cts = s.in_cts();
    WorkArena a(d_work);
    const LimbWork L = limb_layout(c, B, s, in_form, a);
    const signed char *xl = (const signed char *)d_x;
    if (!limb_in(in_form)) {
        const u64 *xn = d_x; bool packed = in_form == CRC_NTTP;
        if (in_form == CRC_COEFF) { RUN(k_ntt_ct(c, false, d_x, L.buf, (size_t)B * in_cts, 2, false, st, nullptr, 0, 0, 0, 0)); xn = L.buf; packed = false; }
        RUN(k_limb_pack_tensor(c, xn, L.Xl, B, zd, npos, packed, st, 0, 0, scalar));
        xl = L.Xl;
    }
    // bias joins in the NTT domain unless the result goes back to coefficient form (then add_plain(bias) rides on the inverse transform's store)
    // hand-over to a dense layer (channels = (f, px, py) flattened), written by the kernel itself -- in its own row order: the scalar kernel writes CRC_NTTLS
    if (out_form == (scalar ? CRC_NTTLS : CRC_NTTL) && k_limb_direct_dense(P))
        return k_limb_mac(c, xl, (const signed char *)d_wl, L.Ys, (signed char *)d_y, d_bias, B, s, st, scalar);
    RUN(k_limb_mac(c, xl, (const signed char *)d_wl, L.Ys, nullptr, out_form != CRC_COEFF ? d_bias : nullptr, B, s, st, scalar));
    if (limb_in(out_form)) return k_limb_result_to_limb(c, L.Ys, (signed char *)d_y, B, nf * P, st, out_form == CRC_NTTLS);     // ... or re-limbed from the slot-major result
    RUN(k_limb_result_to_rows(c, L.Ys, d_y, (size_t)B * nf * P * 2, out_form == CRC_NTTP, st));
    if (out_form == CRC_COEFF) RUN(k_ntt_ct(c, true, d_y, d_y, (size_t)B * nf * P, 2, false, st, d_bias, 1, (size_t)P, nf));
    return CRC_OK;
}

extern "C" int crc_conv2d_forms(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_w, int w_form, const uint64_t *d_bias, int B, int zd, int xd, int yd,
                                int xs, int ys, int xf, int yf, int nf, int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream)
{
    CHECK_CTX(c);
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    if (w_form == CRC_NTTL1) {
        if (!d_x || !d_w || !d_y || !d_work || B < 0 || nf < 1 || !nform_ok(in_form) || !(lform_ok(out_form) || out_form == CRC_NTTLC) || !s.w.ok())
            return CRC_ERR_INVALID_ARGUMENT;
        if (!k_limb_conv1_shape(c, s)) return CRC_ERR_UNSUPPORTED;
        if (B == 0) return CRC_OK;
        return conv2d_limb1(c, d_x, d_w, d_bias, B, s.w, nf, in_form, out_form, d_y, d_work, S(stream));
    }
    if (w_form == CRC_NTTL) {
        if (!d_x || !d_w || !d_y || !d_work || B < 0 || zd < 1 || nf < 1 || !lform_ok(in_form) || !lform_ok(out_form) || !s.w.ok())
            return CRC_ERR_INVALID_ARGUMENT;
        if (B == 0) return CRC_OK;
        return conv2d_limb(c, d_x, d_w, d_bias, B, s, in_form, out_form, d_y, d_work, S(stream));
    }
    if (w_form == CRC_NTTLS) {
        // in_form: a convolution's tensor as CRC_NTTL, a dense layer's (one position) as CRC_NTTLS -- the two dense layouts differ -- or rows in any form
        const bool in_ok = nform_ok(in_form) || (xd * yd == 1 ? in_form == CRC_NTTLS : in_form == CRC_NTTL);
        if (!d_x || !d_w || !d_y || !d_work || B < 0 || zd < 1 || nf < 1 || !(lform_ok(out_form) || out_form == CRC_NTTLS) || !s.w.ok() ||
            !in_ok) return CRC_ERR_INVALID_ARGUMENT;
        if (B == 0) return CRC_OK;
        return conv2d_limb(c, d_x, d_w, d_bias, B, s, in_form, out_form, d_y, d_work, S(stream), true);
    }
    if (!d_x || !d_w || !d_y || !d_work || B < 0 || zd < 1 || nf < 1 || !nform_ok(in_form) || !nform_ok(out_form) || (w_form != CRC_NTT && w_form != CRC_NTTP) ||
        !s.w.ok()) return CRC_ERR_INVALID_ARGUMENT;
    if (B == 0) return CRC_OK;
    const int P = s.w.P(), in_cts = s.in_cts();
    hipStream_t st = S(stream);
    WorkArena a(d_work);
    const ConvWork L = conv_layout(c, B, s, in_form, a);
    RUN(k_conv_offsets(c, L.xoff, L.toff, L.toffw, s, st));
    const u64 *xn = d_x;
    int xp = in_form == CRC_NTTP;
    if (in_form == CRC_COEFF) {                   // transform_input_to_ntt, convolutionalLayer.cpp:95-148 (out of place: x is const)
        int maxbits = 0; for (int i = 0; i < c->k; i++) if ((int)c->tabs[i].m.bits > maxbits) maxbits = c->tabs[i].m.bits;
        xp = maxbits <= 55;                       // the private copy goes straight into the MAC kernels' operand form
        RUN(k_ntt_ct(c, false, d_x, L.buf, (size_t)B * in_cts, 2, false, st, nullptr, 0, 0, 0, xp));
        xn = L.buf;
    }
    // sum of products in the NTT domain; bias joins here when the output stays NTT-resident
    RUN(k_mac2(c, xn, d_w, d_y, L.xoff, L.toff, B, s, out_form != CRC_COEFF ? d_bias : nullptr, L.toffw, st, xp, w_form == CRC_NTTP, out_form == CRC_NTTP));
    if (out_form == CRC_COEFF)                    // one inverse NTT per output ciphertext, add_plain(bias) fused into its store
        RUN(k_ntt_ct(c, true, d_y, d_y, (size_t)B * nf * P, 2, false, st, d_bias, 1, (size_t)P, nf));
    return CRC_OK;
}
// The one-channel layer on the bxf x byf window sums of its input (the box: kernels_mfma1.hip limb_pack_rows1_kernel_px).  (xd, yd): the full image, (xf, yf):
// the BASE window; a 1 x 1 box is crc_conv2d_forms
extern "C" int crc_limb_conv1_box_supported(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf)
{
    if (!c || nf < 1 || bxf < 1 || byf < 1 || xs < 1 || ys < 1) return 0;
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    if (!s.w.ok() || !s.w.boxed(bxf, byf).ok()) return 0;
    return k_limb_conv1_box_shape(c, s, bxf, byf) ? 1 : 0;
}
extern "C" size_t crc_conv2d_box_forms_work_bytes(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf,
    int in_form, int w_form, int out_form)
{
    if (c && bxf == 1 && byf == 1) return crc_conv2d_forms_work_bytes(c, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, w_form, out_form);
    if (w_form != CRC_NTTL1 || !crc_limb_conv1_box_supported(c, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf)) return 0;
    WorkArena a;
    limb1_layout(c, B, {xd, yd, xs, ys, xf, yf}, bxf, byf, nf, in_form, out_form, a);
    return a.bytes();
}
extern "C" int crc_conv2d_box_forms(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_w, int w_form, const uint64_t *d_bias, int B, int zd, int xd, int yd,
                                    int xs, int ys, int xf, int yf, int nf, int bxf, int byf, int in_form, int out_form, uint64_t *d_y, void *d_work,
                                    void *stream)
{
    if (bxf == 1 && byf == 1) return crc_conv2d_forms(c, d_x, d_w, w_form, d_bias, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form, d_y, d_work, stream);
    CHECK_CTX(c);
    const Window in{xd, yd, xs, ys, xf, yf};
    if (!d_x || !d_w || !d_y || !d_work || B < 0 || nf < 1 || bxf < 1 || byf < 1 || !nform_ok(in_form) || !(lform_ok(out_form) || out_form == CRC_NTTLC) ||
        !in.ok()) return CRC_ERR_INVALID_ARGUMENT;
    if (w_form != CRC_NTTL1 || !crc_limb_conv1_box_supported(c, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf)) return CRC_ERR_UNSUPPORTED;
    if (B == 0) return CRC_OK;
    return conv2d_limb1(c, d_x, d_w, d_bias, B, in, nf, in_form, out_form, d_y, d_work, S(stream), bxf, byf);
}
extern "C" int crc_conv2d(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_w, const uint64_t *d_bias, int B, int zd, int xd, int yd,
                          int xs, int ys, int xf, int yf, int nf, int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream)
{
    if (!form_ok(in_form) || !form_ok(out_form)) return CRC_ERR_INVALID_ARGUMENT;
    return crc_conv2d_forms(c, d_x, d_w, CRC_NTT, d_bias, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form, d_y, d_work, stream);
}
extern "C" int crc_dense_forms(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_w, int w_form, const uint64_t *d_bias, int B, int in_dim, int out_dim,
                               int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream)
{
    return crc_conv2d_forms(c, d_x, d_w, w_form, d_bias, B, in_dim, 1, 1, 1, 1, 1, 1, out_dim, in_form, out_form, d_y, d_work, stream);
}
extern "C" int crc_pack28(crc_ctx *c, uint64_t *d_rows, size_t rows, int unpack, void *stream)
{
    CHECK_CTX(c); if (!d_rows) return CRC_ERR_INVALID_ARGUMENT;
    return k_pack28(c, d_rows, rows, unpack != 0, S(stream));
}

extern "C" size_t crc_dense_work_bytes(const crc_ctx *c, int B, int in_dim, int out_dim, int in_form)
{
    return crc_conv2d_work_bytes(c, B, in_dim, 1, 1, 1, 1, 1, 1, out_dim, in_form);
}
extern "C" int crc_dense(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_w, const uint64_t *d_bias, int B, int in_dim, int out_dim,
                         int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream)
{
    // a dense layer is the 1x1 convolution of an in_dim-channel 1x1 image (reshapeInput, fullyConnectedLayer.cpp:38-56,
    // flattens z,x,y row-major, which is the tensor's memory order)
    return crc_conv2d(c, d_x, d_w, d_bias, B, in_dim, 1, 1, 1, 1, 1, 1, out_dim, in_form, out_form, d_y, d_work, stream);
}

extern "C" int crc_conv2d_fold_pool(crc_ctx *c, const uint64_t *d_w, const uint64_t *d_bias_ntt, const uint64_t *d_div_ntt, int nf, int zd, int xf, int yf,
                                    int cxs, int cys, int pxf, int pyf, uint64_t *d_w_out, uint64_t *d_bias_out, void *stream)
{
    CHECK_CTX(c);
    if (!d_w || !d_bias_ntt || !d_w_out || !d_bias_out || nf < 1 || zd < 1 || xf < 1 || yf < 1 || cxs < 1 || cys < 1 || pxf < 1 ||
        pyf < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_fold_pool(c, d_w, d_bias_ntt, d_div_ntt, d_w_out, d_bias_out, nf, zd, xf, yf, cxs, cys, pxf, pyf, S(stream));
}
// the downstream half of the hoisted pair (crc_plan_hoist_pool): w' = div * w in the convolution's own window, b' = div * pxf*pyf * b
extern "C" int crc_conv2d_hoist_pool(crc_ctx *c, const uint64_t *d_w, const uint64_t *d_bias_ntt, const uint64_t *d_div_ntt, int nf, int zd, int xf, int yf,
                                     int pxf, int pyf, uint64_t *d_w_out, uint64_t *d_bias_out, void *stream)
{
    CHECK_CTX(c);
    if (!d_w || !d_bias_ntt || !d_w_out || !d_bias_out || nf < 1 || zd < 1 || xf < 1 || yf < 1 || pxf < 1 || pyf < 1) return CRC_ERR_INVALID_ARGUMENT;
    return k_fold_pool(c, d_w, d_bias_ntt, d_div_ntt, d_w_out, d_bias_out, nf, zd, xf, yf, 1, 1, pxf, pyf, S(stream), true);
}

// ---- pooling / batch-norm -----------------------------------------------------------------------------------------
extern "C" int crc_pool(crc_ctx *c, const uint64_t *d_x, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
                        const uint64_t *d_div, int form, uint64_t *d_y, void *stream)
{
    // form = CRC_NTTP: NTT-form input, result written in the MAC kernels' operand form (the layer behind is a conv / dense layer)
    CHECK_CTX(c);
    const Window w{xd, yd, xs, ys, xf, yf};
    if (!d_x || !d_y || B < 0 || zd < 1 || !nform_ok(form) || !w.ok()) return CRC_ERR_INVALID_ARGUMENT;
    if (B == 0) return CRC_OK;
    hipStream_t st = S(stream);
    if (form == CRC_NTTP) return k_pool(c, d_x, d_y, B, zd, w, d_div, st, 1);
    if (form == CRC_NTT || !d_div) return k_pool(c, d_x, d_y, B, zd, w, form == CRC_NTT ? d_div : nullptr, st);
    // coefficient form average pooling: add_many then multiply_plain(div_factor) (avgPoolingLayer.cpp:37-38)
    RUN(k_pool(c, d_x, d_y, B, zd, w, nullptr, st));
    const size_t cnt = (size_t)B * zd * w.xo() * w.yo();
    RUN(k_ntt_ct(c, false, d_y, d_y, cnt, 2, false, st, nullptr, 0, 0));
    RUN(k_rowwise(c, d_y, d_div, cnt, 2, 2, 1, cnt, 0, st));
    return k_ntt_ct(c, true, d_y, d_y, cnt, 2, false, st, nullptr, 0, 0);
}

// zero padding (PaddingLayer): all-zero ciphertexts around every channel plane, the form kept.  Only canonical rows: in the packed and limb operand forms a
// tensor is laid out for the layer that reads it, and no such hand-over spans a pad
extern "C" int crc_pad(crc_ctx *c, const uint64_t *d_x, int B, int zd, int xd, int yd, int px0, int px1, int py0, int py1, int form, uint64_t *d_y,
                       void *stream)
{
    CHECK_CTX(c);
    if (!d_x || !d_y || B < 0 || zd < 1 || xd < 1 || yd < 1 || px0 < 0 || px1 < 0 || py0 < 0 || py1 < 0 || !form_ok(form)) return CRC_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_x | (uintptr_t)d_y) & 15) return CRC_ERR_INVALID_ARGUMENT;           // 16-byte loads and stores
    const long long xo = (long long)xd + px0 + px1, yo = (long long)yd + py0 + py1;
    if (xo > 0x7fffffffLL || yo > 0x7fffffffLL) return CRC_ERR_INVALID_ARGUMENT;
    const size_t ctb = crc_ct_words(c, 2) * 8;
    const size_t in_bytes = (size_t)B * zd * xd * yd * ctb, out_bytes = (size_t)B * zd * (size_t)xo * (size_t)yo * ctb;
    // not in place: an output row would overwrite input rows that are still to be read
    const uintptr_t x0 = (uintptr_t)d_x, y0 = (uintptr_t)d_y;
    if (x0 < y0 + out_bytes && y0 < x0 + in_bytes) return CRC_ERR_INVALID_ARGUMENT;
    if (B == 0) return CRC_OK;
    return k_pad(c, d_x, d_y, B, zd, xd, yd, px0, px1, py0, py1, S(stream));
}

extern "C" int crc_batchnorm(crc_ctx *c, uint64_t *d_x, int B, int zd, int xd, int yd, const uint64_t *d_mean, const uint64_t *d_invstd,
                             int form, void *stream)
{
    CHECK_CTX(c);
    if (!d_x || !d_mean || !d_invstd || B < 0 || zd < 1 || xd < 1 || yd < 1 || !form_ok(form)) return CRC_ERR_INVALID_ARGUMENT;
    if (B == 0) return CRC_OK;
    hipStream_t st = S(stream);
    const size_t hw = (size_t)xd * yd, cnt = (size_t)B * zd * hw;
    if (form == CRC_NTT) return k_bn_ntt(c, d_x, B, zd, (int)hw, d_mean, d_invstd, st);
    // sub_plain(mean[z]) then multiply_plain(var[z])  (batchNormLayer.cpp:36-37)
    RUN(k_rowwise(c, d_x, d_mean, cnt, 2, 1, -1, hw, (size_t)zd, st));
    RUN(k_ntt_ct(c, false, d_x, d_x, cnt, 2, false, st, nullptr, 0, 0));
    RUN(k_rowwise(c, d_x, d_invstd, cnt, 2, 2, 1, hw, (size_t)zd, st));
    return k_ntt_ct(c, true, d_x, d_x, cnt, 2, false, st, nullptr, 0, 0);
}

// ---- kernel selection: ONE statement of the policy for every host (netrun.py, crcnn_amd/host) ------------------------------------------------------
// which multiply-accumulate kernel a conv / dense layer (dense: xd = yd = xf = yf = xs = ys = 1, zd = in_dim, nf = out_dim) runs on when launched on B images
static int plan_mac(const crc_ctx *c, const LayerShape &s, int B, int matrix_cores, int *w_form)
{
    const int zd = s.zd, nf = s.nf, xf = s.w.xf, yf = s.w.yf;
    if (!c || !w_form || zd < 1 || nf < 1 || !s.w.ok()) return CRC_ERR_INVALID_ARGUMENT;
    bool packable = true;
    for (int i = 0; i < c->k; i++) if (c->tabs[i].m.bits > 55) packable = false;
    *w_form = packable ? CRC_NTTP : CRC_NTT;                      // mac3_kernel / mac2_kernel on 28-bit limb pairs (canonical residues above 55 bits)
    if (!matrix_cores || !packable) return CRC_OK;
    // one-channel convolutions (conv1, alone or with its pooling layer folded in) have their own matrix-core kernel
    if (zd == 1) { if (k_limb_conv1_shape(c, s)) *w_form = CRC_NTTL1; return CRC_OK; }
    // the limb GEMM pays from 8 reduction steps of 32 channels on (below that its fixed costs per output tile and the channel padding eat the gain), and only
    // with at least half a 64-row tile of rows = (image, pixel, poly) per launch: with fewer, most of every MFMA is padding and every slot's weights are
    // streamed for a handful of rows (PlainModelWoPad at 6 images per launch: fc4 0.23 ms per image on mac3_kernel against 1.59)
    const int min_steps = c->tune.mfma_min_steps > 0 ? c->tune.mfma_min_steps : 8;
    const long long P = s.w.P64();
    // ... a full tile of rows for layers of fewer than 24 filters: the limb form pads the filters to 64, so a 10-filter layer -- CrCNN's fc4 -- spends 6x its
    // canonical bytes and 5/6 of its MFMAs on zeros (PlainModelWoPad's fc4 at 24 images: 14 GiB of weights, 0.16 against 0.11 ms per image on the vector-ALU
    // kernel; with 64 rows and more -- PlainModelTiny at 128 images, ApproxPlainModel at 32 -- it still wins, not least because the layer in front hands its
    // tensor over in limb form)
    // -- and only on the smaller rings (n k <= 32768), where those 6x are a few GB (28 GiB at n = 16384 with eight primes)
    const long long rows = (long long)B * 2 * P, min_rows = nf >= 24 ? 32 : 64;
    const bool few_filters_ok = nf >= 24 || (long long)c->n * c->k <= 32768;
    if (zd >= 16 && few_filters_ok && (long long)((zd + 31) / 32) * xf * yf >= min_steps && crc_limb_supported(c, zd, xf, yf) && (B <= 0 ||
        rows >= min_rows)) *w_form = CRC_NTTL;
    return CRC_OK;
}
extern "C" int crc_plan_mac(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int B, int matrix_cores, int *w_form)
{
    return plan_mac(c, {{xd, yd, xs, ys, xf, yf}, zd, nf}, B, matrix_cores, w_form);
}
// ---- scalar form (CRC_NTTLS): slot-batched networks, whose weights are constant polynomials -----------------------------------------------------
extern "C" size_t crc_scalar_weights_bytes(const crc_ctx *c, int nf, int zd, int xf, int yf)
{
    return c && nf >= 1 && zd >= 1 && xf >= 1 && yf >= 1 ? k_scalar_weights_bytes(c, nf, zd, xf, yf) : 0;
}
extern "C" int crc_scalar_supported(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf)
{
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    if (!c || B < 1 || zd < 1 || nf < 1 || !s.w.ok()) return 0;
    return k_scalar_supported(c, B, s) ? 1 : 0;
}
extern "C" int crc_scalar_pack_weights(crc_ctx *c, const uint64_t *d_w, int w_stride, int nf, int zd, int xf, int yf, void *d_ws, int *constant, void *stream)
{
    if (constant) *constant = 1;                                  // 0 only where a row was found not to be constant
    CHECK_CTX(c);
    if (!d_w || !d_ws || !constant || nf < 1 || zd < 1 || xf < 1 || yf < 1 || (w_stride != 1 && w_stride != c->n)) return CRC_ERR_INVALID_ARGUMENT;
    if (c->k > 8 || !k_limb_supported(c, k_limb_steps(zd, xf, yf) * 32)) return CRC_ERR_UNSUPPORTED;
    return k_scalar_pack_weights(c, d_w, (size_t)w_stride, (signed char *)d_ws, nf, zd, xf, yf, constant, S(stream));
}
// crc_plan_mac for a layer of a slot-batched network: the scalar form wherever it runs and the layer has a reduction worth a GEMM (zd >= 2); one-channel
// convolutions keep their own kernel, moduli above 55 bits theirs.  The rows guard of crc_plan_mac does not apply: the merged GEMM has n B 2P rows.
extern "C" int crc_plan_mac_scalar(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int B, int *w_form)
{
    const LayerShape s{{xd, yd, xs, ys, xf, yf}, zd, nf};
    RUN(plan_mac(c, s, B, 1, w_form));
    if (c->tune.scalar_mac && zd >= 2 && k_scalar_supported(c, B < 1 ? 1 : B, s)) *w_form = CRC_NTTLS;
    return CRC_OK;
}
// should a (sum / average) pooling layer be folded into the convolution in front of it (crc_conv2d_fold_pool: exact)?  Cost in units of one multiply-accumulate
// term per output ciphertext: the MAC kernels pay ~24 terms of prologue / epilogue per output and take filters in multiples of 8; a pooling pass moves (window
// + 1) ciphertexts per output at HBM rate, ~10 term-times each.  Folding wins whenever it removes MACs (decimating pools) and narrowly for CrCNN's stride-1
// pools.
extern "C" int crc_plan_fold_pool(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int pxs, int pys, int pxf, int pyf,
    int *fold)
{
    const Window w{xd, yd, xs, ys, xf, yf};
    if (!c || !fold || zd < 1 || nf < 1 || !w.ok() || pxs < 1 || pys < 1 || pxf < 1 || pyf < 1) return CRC_ERR_INVALID_ARGUMENT;
    *fold = 0;
    const int xo = w.xo(), yo = w.yo();
    const Window w2 = w.fold(pxs, pys, pxf, pyf), pool{xo, yo, pxs, pys, pxf, pyf};
    if (w2.xf > w.xd || w2.yf > w.yd || pxf > xo || pyf > yo) return CRC_OK;
    const int xo2 = w2.xo(), yo2 = w2.yo();
    if (xo2 != pool.xo() || yo2 != pool.yo()) return CRC_OK;           // the folded convolution must produce exactly the pooled tensor
    const long long fpad = (nf + 7) / 8 * 8, T1 = (long long)zd * w.xf * w.yf, T2 = (long long)zd * w2.xf * w2.yf;
    const long long cost_sep = fpad * xo * yo * (T1 + 24) + (long long)nf * xo2 * yo2 * 10 * (pxf * pyf + 1);
    const long long cost_fused = fpad * xo2 * yo2 * (T2 + 24);
    *fold = cost_fused < cost_sep ? 1 : 0;
    return CRC_OK;
}

// Cost of a conv / dense layer on the kernel crc_plan_mac gives it, in crc_plan_fold_pool's units (one multiply-accumulate term per output ciphertext, ~24 terms
// of prologue / epilogue per output).  The limb GEMM pads the channels of every tap to 32 and takes filters in tiles of 32.  The one-channel matrix-core kernel
// pays for its whole K whatever the window -- 64 taps in the plane-major form, 40 in the pixel-major one -- for 32 filters and whole 16-row tiles (8 positions x 2
// polys), and a term there costs 8/5 of the limb GEMM's (PlainModelTiny at n = 4096, 128 images per launch, kernel + image pack: pixel-major 6 x 6 35.9 ms for 18
// tiles, plane-major 8 x 8 44.5 ms for 16, against 92.6 ms for the limb GEMM's 64 x 16 outputs of 1152 + 24 terms -- 1.59 and 1.60; profiles/conv1_box_ab.txt.
// 25/16 before those measurements)
static long long plan_mac_cost(const crc_ctx *c, const LayerShape &s, int B, int matrix_cores)
{
    const int zd = s.zd, nf = s.nf, xf = s.w.xf, yf = s.w.yf;
    int wf = CRC_NTT;
    if (plan_mac(c, s, B, matrix_cores, &wf) != CRC_OK) return -1;
    const long long P = s.w.P64();
    if (wf == CRC_NTTL1) return 32 * ((2 * P + 15) / 16 * 8) * ((k_limb_conv1_form(c, xf, yf, nf) == 2 ? 40 : 64) + 24) * 8 / 5;
    if (wf == CRC_NTTL) return (long long)(nf + 31) / 32 * 32 * P * ((long long)k_limb_steps(zd, xf, yf) * 32 + 24);
    return (long long)(nf + 7) / 8 * 8 * P * ((long long)zd * xf * yf + 24);
}
// Should the pooling layer behind a stride-1 convolution be HOISTED instead of folded into that convolution's weights?  pool(conv_w(x) + b) = conv_{div w}(S) +
// div pxf pyf b with S the stride-1 pxf x pyf window sum of x: the convolution keeps its window (xf x yf taps per channel instead of the folded (xf + pxf - 1) x
// (yf + pyf - 1)) and takes the pool's stride, and S is made by the layer in FRONT -- u..., a convolution, as already folded -- with that sum pool folded into its
// weights (crc_conv2d_fold_pool, no divisor): no pass of its own.  Exact over Z_q.  The answer is no unless: the convolution has stride 1; the pool decimates (a
// stride-1 pool removes no multiply-accumulates) and crc_plan_fold_pool folds it; the layer in front is a convolution whose output is this one's input (the
// caller passes uzd = 0 where there is none, or where it is not resident: streamed or tile-wise weights); its enlarged window fits its image and, where the layer
// runs on the matrix cores, keeps a matrix-core kernel (one-channel kernel: windows up to 8 x 8); and the two layers cost less hoisted than folded (plan_mac_cost
// on B images per launch).  The tuning key hoist_pool = 0 (CRC_HOIST_POOL=0) answers no throughout.
extern "C" int crc_plan_hoist_pool(const crc_ctx *c, int uzd, int uxd, int uyd, int uxs, int uys, int uxf, int uyf, int unf, int zd, int xd, int yd, int xs,
                                   int ys, int xf, int yf, int nf, int pxs, int pys, int pxf, int pyf, int B, int matrix_cores, int *hoist)
{
    const LayerShape up{{uxd, uyd, uxs, uys, uxf, uyf}, uzd, unf}, conv{{xd, yd, xs, ys, xf, yf}, zd, nf};
    const Window &w = conv.w;
    if (!c || !hoist || zd < 1 || nf < 1 || !w.ok() || pxs < 1 || pys < 1 || pxf < 1 || pyf < 1) return CRC_ERR_INVALID_ARGUMENT;
    *hoist = 0;
    if (!c->tune.hoist_pool || xs != 1 || ys != 1 || pxs * pys == 1) return CRC_OK;
    int fold = 0;
    { const int rc = crc_plan_fold_pool(c, zd, xd, yd, xs, ys, xf, yf, nf, pxs, pys, pxf, pyf, &fold); if (rc != CRC_OK) return rc; }
    if (!fold) return CRC_OK;
    if (uzd < 1 || unf != zd || !up.w.ok() || up.w.xo() != xd || up.w.yo() != yd) return CRC_OK;
    // the layer in front with the sum pool folded in: S = [zd][xd - pxf + 1][yd - pyf + 1], the stride-1 box sums of the convolution's image, which the
    // convolution's own window then reads at the pool's stride
    const LayerShape up_folded{up.w.fold(1, 1, pxf, pyf), uzd, unf}, folded{w.fold(pxs, pys, pxf, pyf), zd, nf};
    LayerShape hoisted{w.boxed(pxf, pyf), zd, nf};
    hoisted.w.xs = pxs; hoisted.w.ys = pys;
    if (up_folded.w.xf > uxd || up_folded.w.yf > uyd || !up_folded.w.ok()) return CRC_OK;
    if (up_folded.w.xo() != hoisted.w.xd || up_folded.w.yo() != hoisted.w.yd) return CRC_OK;
    // the convolution over S must produce exactly the pooled tensor (pool: on the convolution's own output, xd - xf + 1 at its stride of 1)
    const Window pool{xd - xf + 1, yd - yf + 1, pxs, pys, pxf, pyf};
    if (!hoisted.w.ok() || hoisted.w.xo() != pool.xo() || hoisted.w.yo() != pool.yo()) return CRC_OK;
    int uf = CRC_NTT, uf2 = CRC_NTT;
    if (plan_mac(c, up, B, matrix_cores, &uf) != CRC_OK || plan_mac(c, up_folded, B, matrix_cores, &uf2) != CRC_OK) return CRC_OK;
    if ((uf == CRC_NTTL1 || uf == CRC_NTTL) && uf2 != uf) return CRC_OK;
    const long long cost_folded = plan_mac_cost(c, up, B, matrix_cores) + plan_mac_cost(c, folded, B, matrix_cores);
    const long long cost_hoisted = plan_mac_cost(c, up_folded, B, matrix_cores) + plan_mac_cost(c, hoisted, B, matrix_cores);
    *hoist = cost_hoisted < cost_folded ? 1 : 0;
    return CRC_OK;
}

// Should a one-channel convolution whose weights are its base window W (xf x yf) convolved with a bxf x byf sum at its own stride -- the upstream layer of a hoisted
// pair (crc_plan_hoist_pool) -- sum its INPUT instead (crc_conv2d_box_forms) and keep W?  conv_{W * box}(x) = conv_W(box x): exact over Z_q.  Yes when the base
// window runs on the pixel-major one-channel kernel, the summed image fits it, and the box execution costs less than the enlarged window in plan_mac_cost's units.
// The box's own cost is what the image pack takes on top of packing the summed image alone, written as PLAN_BOX_READ units per further term (bxf byf - 1 per
// pixel and poly of the summed image) -- measured, not derived: PlainModelTiny at n = 4096, 128 images per launch, the staged pack (kernels_mfma1.hip
// limb_pack_box_kernel_px: every input loaded once into a ring in LDS) 8.67 ms with the 2 x 2 box against 5.67 ms x 26^2 / 28^2 = 4.89 ms without one, 3.78 ms for
// 26 x 26 x 2 x 3 terms, at the limb GEMM's 75.2 ns per unit (90.56 ms / 1 204 224 units in the same job: profiles/conv1_box_staged_ab.txt) = 12.4.  (The direct
// form, which re-read every term from L2, was 21.)  What is left is no longer re-reading: the pass reads 28 x 28 inputs to write 26 x 26 pixels, holds 68.5 KiB of
// LDS (two workgroups per CU) and has two barriers per row group.  The tuning key conv1_box = 0 (CRC_CONV1_BOX=0) answers no throughout.
// A COEFFICIENT-form input no longer pays this: its window sums are taken in front of the input transform (conv2d_limb1: k_ntt_ct_box) and the pack runs unboxed on
// the summed image.  The constant stays the staged pack's: an NTT-form input still pays it, the plan has no input-form argument, and the cheaper path only makes a
// yes more right.
#define PLAN_BOX_READ 12
extern "C" int crc_plan_conv1_box(const crc_ctx *c, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf, int B, int matrix_cores,
                                  int *box)
{
    const Window w{xd, yd, xs, ys, xf, yf};
    if (!c || !box || zd < 1 || nf < 1 || bxf < 1 || byf < 1 || !w.ok()) return CRC_ERR_INVALID_ARGUMENT;
    *box = 0;
    if (!c->tune.conv1_box || !matrix_cores || bxf * byf == 1) return CRC_OK;
    if (!crc_limb_conv1_box_supported(c, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf)) return CRC_OK;
    const LayerShape enlarged{w.fold(1, 1, bxf, byf), zd, nf}, boxed{w.boxed(bxf, byf), zd, nf};
    if (!enlarged.w.ok()) return CRC_OK;
    int wf = CRC_NTT;
    if (plan_mac(c, boxed, B, matrix_cores, &wf) != CRC_OK || wf != CRC_NTTL1) return CRC_OK;
    const long long cost_enlarged = plan_mac_cost(c, enlarged, B, matrix_cores);
    const long long cost_boxed = plan_mac_cost(c, boxed, B, matrix_cores) + (long long)boxed.w.xd * boxed.w.yd * 2 * (bxf * byf - 1) * PLAN_BOX_READ;
    *box = cost_enlarged >= 0 && cost_boxed < cost_enlarged ? 1 : 0;
    return CRC_OK;
}

// ---- square + relinearize -----------------------------------------------------------------------------------------
// ciphertexts per internal pass of square + relinearise: bounds the scratch footprint at ~10 GB for every ring size -- 1024 up to n k = 32768, 512 up to 65536,
// 256 at n = 16384 with all eight primes.  (Round 5: 1024 instead of 512 on the small rings -- the eight kernels of a pass each end in a partly filled last
// wave of workgroups; at (8192, 3) twice the pass is 2 % faster, at (16384, 4) it changes nothing: profiles/r05_square_chunk_sweep.txt)
static size_t square_chunk(const crc_ctx *c)
{
    if (c->tune.sq_chunk > 0) return (size_t)c->tune.sq_chunk;
    const size_t nk = (size_t)c->n * c->k;
    return nk <= 32768 ? 1024 : nk <= 65536 ? 512 : nk <= 131072 ? 256 : 128;
}

// Work of the activation family (the square or the multiply, then the key switch; flat or pooled; with or without ring-linear terms), sized for one internal pass:
// [xh: NTT copy of a coefficient-form input][s: relin(x^2) of the degree-3 activation][packed keys (filled by pass 0)][size-3 products][scratch of the product, then
// of the key switch].  A pass takes `step` whole channel planes of pin ciphertexts in, pout out (a pooling window never leaves its plane); flat calls have 1 x 1 planes
struct ActWork { u64 *xh, *s, *kp, *y3, *rest; size_t step; };
enum { ACT_XH = 1, ACT_S = 2, ACT_MULTIPLY = 4 };      // which of xh and s a call has, and whether its product is the multiply's (k_multiply_work_words)
static ActWork act_layout(const crc_ctx *c, size_t planes, size_t pin, size_t pout, int dbc, int regions, WorkArena &a)
{
    ActWork L{};
    L.step = square_chunk(c) / pin ? square_chunk(c) / pin : 1;
    const size_t pp = planes < L.step ? planes : L.step, cin = pp * pin, cout = pp * pout;
    const size_t pr = regions & ACT_MULTIPLY ? k_multiply_work_words(c, cin) : k_square_work_words(c, cin), rl = k_relin_work_words(c, cout, dbc);
    if (regions & ACT_XH) L.xh = a.take<u64>(cin * crc_ct_words(c, 2));
    if (regions & ACT_S) L.s = a.take<u64>(cin * crc_ct_words(c, 2));
    L.kp = a.take<u64>(k_relin_keys_words(c, dbc));
    L.y3 = a.take<u64>(cin * crc_ct_words(c, 3));
    L.rest = a.take<u64>(pr > rl ? pr : rl);
    return L;
}
static size_t act_bytes(const crc_ctx *c, size_t planes, size_t pin, size_t pout, int dbc, int regions)
{
    WorkArena a;
    act_layout(c, planes, pin, pout, dbc, regions, a);
    return a.bytes();
}
static inline size_t pass_len(size_t count, size_t o, size_t step) { return count - o < step ? count - o : step; }      // of the internal pass that starts at o
// a coefficient-form pass of ch ciphertexts, copied into work space and transformed
static int ntt_copy(crc_ctx *c, const u64 *x, size_t ch, u64 *xh, void *stream)
{
    HIPCHK(hipMemcpyAsync(xh, x, 8 * ch * crc_ct_words(c, 2), hipMemcpyDeviceToDevice, S(stream)));
    return crc_ntt_fwd(c, xh, ch, 2, stream);
}
extern "C" size_t crc_square_relin_work_bytes(const crc_ctx *c, size_t count, int dbc) { return c && dbc_ok(dbc) ? act_bytes(c, count, 1, 1, dbc, 0) : 0; }
extern "C" size_t crc_encrypt_dev_work_bytes(const crc_ctx *c, size_t count) { return c ? work_bytes(k_encrypt_work_words(c, count)) : 0; }
extern "C" int crc_encrypt_dev_key(crc_ctx *c, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, const uint8_t *key, uint64_t stream_base,
                                   uint64_t *d_ct, void *d_work, void *stream)
{
    return crc_encrypt_dev_key_forms(c, d_pk, d_plain, count, key, stream_base, CRC_COEFF, d_ct, d_work, stream);
}
extern "C" int crc_encrypt_dev(crc_ctx *c, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, uint64_t seed, uint64_t *d_ct, void *d_work,
    void *stream)
{
    return crc_encrypt_dev_forms(c, d_pk, d_plain, count, seed, CRC_COEFF, d_ct, d_work, stream);
}
extern "C" int crc_encrypt_dev_key_forms(crc_ctx *c, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, const uint8_t *key, uint64_t stream_base,
                                         int out_form, uint64_t *d_ct, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_pk || !d_plain || !d_ct || !d_work || !key || (out_form != CRC_COEFF && out_form != CRC_NTT)) return CRC_ERR_INVALID_ARGUMENT;
    return k_encrypt(c, d_pk, d_plain, count, chacha_load_key(key), stream_base, d_ct, work_base(d_work), S(stream), out_form == CRC_NTT);
}
extern "C" int crc_encrypt_dev_forms(crc_ctx *c, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, uint64_t seed, int out_form, uint64_t *d_ct,
                                     void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_pk || !d_plain || !d_ct || !d_work || (out_form != CRC_COEFF && out_form != CRC_NTT)) return CRC_ERR_INVALID_ARGUMENT;
    return k_encrypt(c, d_pk, d_plain, count, chacha_seed_key(seed), 0, d_ct, work_base(d_work), S(stream), out_form == CRC_NTT);
}
extern "C" void crc_encrypt_dev_noise_thresholds(uint64_t *h_out19) { if (h_out19) k_encrypt_cdt(h_out19); }

// ---- Decryptor::decrypt, FractionalEncoder and the refresh of Network::forward on the device (kernels_decrypt.hip) ----
static bool ct_form_ok(int f) { return f == CRC_COEFF || f == CRC_NTT; }
extern "C" size_t crc_decrypt_dev_work_bytes(const crc_ctx *c, size_t count, int size, int in_form)
{
    return c && ct_form_ok(in_form) ? work_bytes(k_decrypt_work_words(c, count, size, in_form == CRC_NTT)) : 0;
}
extern "C" int crc_decrypt_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct, size_t count, int size, int in_form, uint64_t *d_plain, void *d_work,
                               void *stream)
{
    CHECK_CTX(c); if (!d_sk || !d_ct || !d_plain || !d_work || !ct_form_ok(in_form)) return CRC_ERR_INVALID_ARGUMENT;
    return k_decrypt(c, d_sk, d_ct, count, size, in_form == CRC_NTT, d_plain, work_base(d_work), S(stream));
}
// Decryptor::invariant_noise_budget of every ciphertext of a tensor (kernels_budget.hip)
extern "C" size_t crc_noise_budget_dev_work_bytes(const crc_ctx *c, size_t count, int size, int in_form)
{
    return c && ct_form_ok(in_form) && (size == 2 || size == 3) ? work_bytes(k_decrypt_work_words(c, count, size, in_form == CRC_NTT)) : 0;
}
extern "C" int crc_noise_budget_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct, size_t count, int size, int in_form, int32_t *d_bits, int32_t *d_min,
                                    void *d_work, void *stream)
{
    if (!d_sk || !d_ct || !d_bits || !d_work || !ct_form_ok(in_form) || size < 2 || size > 3) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return k_noise_budget(c, d_sk, d_ct, count, size, in_form == CRC_NTT, d_bits, d_min, work_base(d_work), S(stream));
}
extern "C" int crc_budget_bits_host(const crc_ctx *c, const uint64_t *h_v, size_t count, int32_t *h_bits)
{
    if (!c || !h_v || !h_bits) return CRC_ERR_INVALID_ARGUMENT;
    return k_budget_bits_host(c, h_v, count, h_bits);
}
// Slot batching (kernels_slots.hip).  The parameter check comes first: a context without slots answers CRC_ERR_PARAMETERS whatever else is wrong
static int slots_args_ok(const crc_ctx *c, const void *values, const void *plain, int slots, size_t item_stride, size_t slot_stride)
{
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;
    if (!values || !plain || slots < 1 || slots > c->n || !item_stride || !slot_stride) return CRC_ERR_INVALID_ARGUMENT;
    return CRC_OK;
}
extern "C" int crc_slots_compose(crc_ctx *c, const int64_t *h_values, size_t count, int slots, size_t item_stride, size_t slot_stride, uint64_t *h_plain)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    RUN(slots_args_ok(c, h_values, h_plain, slots, item_stride, slot_stride));
    return k_slots_compose_host(c, (const long long *)h_values, count, slots, item_stride, slot_stride, h_plain);
}
extern "C" int crc_slots_decompose(crc_ctx *c, const uint64_t *h_plain, size_t count, int slots, int64_t *h_values, size_t item_stride, size_t slot_stride)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    RUN(slots_args_ok(c, h_values, h_plain, slots, item_stride, slot_stride));
    return k_slots_decompose_host(c, h_plain, count, slots, (long long *)h_values, item_stride, slot_stride);
}
extern "C" int crc_slots_compose_dev(crc_ctx *c, const int64_t *d_values, size_t count, int slots, size_t item_stride, size_t slot_stride, uint64_t *d_plain,
                                     void *stream)
{
    CHECK_CTX(c);
    RUN(slots_args_ok(c, d_values, d_plain, slots, item_stride, slot_stride));
    if (((uintptr_t)d_plain & 15) || ((uintptr_t)d_values & 7)) return CRC_ERR_INVALID_ARGUMENT;
    return k_slots_compose(c, (const long long *)d_values, count, slots, item_stride, slot_stride, d_plain, S(stream));
}
extern "C" int crc_slots_decompose_dev(crc_ctx *c, const uint64_t *d_plain, size_t count, int slots, int64_t *d_values, size_t item_stride, size_t slot_stride,
                                       void *stream)
{
    CHECK_CTX(c);
    RUN(slots_args_ok(c, d_values, d_plain, slots, item_stride, slot_stride));
    if (((uintptr_t)d_plain & 15) || ((uintptr_t)d_values & 7)) return CRC_ERR_INVALID_ARGUMENT;
    return k_slots_decompose(c, d_plain, count, slots, (long long *)d_values, item_stride, slot_stride, S(stream));
}
static int slots_rescale_args_ok(const crc_ctx *c, const void *in, const void *out, uint64_t divisor)
{
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;
    if (!in || !out || divisor < 1 || divisor > ((uint64_t)1 << 62)) return CRC_ERR_INVALID_ARGUMENT;
    return CRC_OK;
}
extern "C" int crc_slots_rescale(crc_ctx *c, const uint64_t *h_plain_in, size_t count, uint64_t divisor, uint64_t *h_plain_out)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    RUN(slots_rescale_args_ok(c, h_plain_in, h_plain_out, divisor));
    return k_slots_rescale_host(c, h_plain_in, count, divisor, h_plain_out);
}
extern "C" int crc_slots_rescale_dev(crc_ctx *c, const uint64_t *d_plain_in, size_t count, uint64_t divisor, uint64_t *d_plain_out, void *stream)
{
    CHECK_CTX(c);
    RUN(slots_rescale_args_ok(c, d_plain_in, d_plain_out, divisor));
    if (((uintptr_t)d_plain_in & 15) || ((uintptr_t)d_plain_out & 15)) return CRC_ERR_INVALID_ARGUMENT;
    return k_slots_rescale(c, d_plain_in, count, divisor, d_plain_out, S(stream));
}
extern "C" int crc_decode_dev(crc_ctx *c, const uint64_t *d_plain, size_t count, double *d_out, void *stream)
{
    CHECK_CTX(c); if (!d_plain || !d_out) return CRC_ERR_INVALID_ARGUMENT;
    return k_fra_decode(c, d_plain, count, d_out, S(stream));
}
extern "C" int crc_encode_dev_f32(crc_ctx *c, const float *d_values, size_t count, uint64_t *d_plain, void *stream)
{
    CHECK_CTX(c); if (!d_values || !d_plain) return CRC_ERR_INVALID_ARGUMENT;
    return k_fra_encode(c, d_values, 0, count, d_plain, nullptr, S(stream));
}
extern "C" int crc_encode_dev_f64(crc_ctx *c, const double *d_values, size_t count, uint64_t *d_plain, void *stream)
{
    CHECK_CTX(c); if (!d_values || !d_plain) return CRC_ERR_INVALID_ARGUMENT;
    return k_fra_encode(c, d_values, 1, count, d_plain, nullptr, S(stream));
}
// ---- client-side refreshes: decrypt on the device, do something to the plaintexts, encrypt again under fresh randomness ----
// Four families (fractional, slots rescale, slots activation, slots CRT), one frame: the family's check, nothing to do for no items (the slot activations), the
// work carved by the family's layout, the decryptor, the family's middle kernel, Reenc::run.
// Reenc: who encrypts a refresh's results (sym: the secret key, d_pk unused), with which randomness, into which form.  A null key pointer comes down as has_key =
// false, for ok() to refuse where the family's check orders it
struct Reenc {
    const u64 *d_sk, *d_pk; bool sym; ChaChaKey key; u64 stream_base; int out_form; bool has_key;
    static Reenc seeded(const u64 *d_sk, const u64 *d_pk, bool sym, u64 seed, int out_form) { return {d_sk, d_pk, sym, chacha_seed_key(seed), 0, out_form, true}; }
    static Reenc keyed(const u64 *d_sk, const u64 *d_pk, bool sym, const uint8_t *key, u64 stream_base, int out_form)
    {
        return {d_sk, d_pk, sym, key ? chacha_load_key(key) : ChaChaKey{}, stream_base, out_form, key != nullptr};
    }
    bool ok() const { return d_sk && (sym || d_pk) && has_key && ct_form_ok(out_form); }
    static size_t words(const crc_ctx *c, bool sym, size_t count) { return sym ? k_encrypt_sym_work_words(c, count) : k_encrypt_work_words(c, count); }
    // plain: dense rows [count][n], or (compact) compact plaintexts; the keystream ids stream_base + id_offset .. + count
    int run(crc_ctx *c, const u64 *plain, size_t count, bool compact, u64 id_offset, u64 *d_out, u64 *w, hipStream_t st) const
    {
        if (sym) return k_encrypt_sym(c, d_sk, plain, count, key, stream_base + id_offset, d_out, w, st, out_form == CRC_NTT, compact);
        return k_encrypt(c, d_pk, plain, count, key, stream_base + id_offset, d_out, w, st, out_form == CRC_NTT, compact);
    }
};
// the tail of every refresh's work: the decryptor's rows for dec_cts ciphertexts in in_form, then -- in the same words -- the encryptor's samples for enc_cts
static size_t refresh_tail_words(const crc_ctx *c, size_t dec_cts, int in_form, bool sym, size_t enc_cts)
{
    const size_t dec = k_decrypt_work_words(c, dec_cts, 2, in_form == CRC_NTT), enc = Reenc::words(c, sym, enc_cts);
    return dec > enc ? dec : enc;
}

// The fractional refresh.  Work: [compact plaintexts [count][96]][dense plaintexts [count][n]: the public-key refresh's coefficient-form results only][the tail]
struct RefreshWork { u64 *compact, *dense, *w; };
static RefreshWork refresh_layout(const crc_ctx *c, size_t count, int in_form, bool sym, WorkArena &a)
{
    RefreshWork L{};
    L.compact = a.take<u64>(count * (size_t)CRC_PLAIN_COMPACT_WORDS);
    if (!sym) L.dense = a.take<u64>(count * (size_t)c->n);
    L.w = a.take<u64>(refresh_tail_words(c, count, in_form, sym, count));
    return L;
}
static size_t refresh_bytes(const crc_ctx *c, size_t count, int in_form, bool sym)
{
    if (!c || !ct_form_ok(in_form)) return 0;
    WorkArena a;
    refresh_layout(c, count, in_form, sym, a);
    return a.bytes();
}
static int refresh_impl(crc_ctx *c, const Reenc &R, const u64 *d_in, size_t count, int in_form, u64 *d_out, float *d_vals, void *d_work, hipStream_t st)
{
    CHECK_CTX(c); if (!R.ok() || !d_in || !d_out || !d_work || !ct_form_ok(in_form)) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena a(d_work);
    const RefreshWork L = refresh_layout(c, count, in_form, R.sym, a);
    // decrypt -> decode -> float -> encode leaves the 96-word compact plaintexts (only the 96 coefficients the decoder reads are ever scaled), which the
    // secret-key encryptor reads for either result form (the NTT form is its definition) and the NTT-form public-key encryptor reads as they are ...
    RUN(k_decrypt_recode(c, R.d_sk, d_in, count, in_form == CRC_NTT, L.compact, d_vals, L.w, st));
    if (R.sym || R.out_form == CRC_NTT) return R.run(c, L.compact, count, true, 0, d_out, L.w, st);
    // ... the coefficient-form public-key encryptor adds Delta m from dense rows
    RUN(k_plain_expand(c, L.compact, count, L.dense, st));
    return R.run(c, L.dense, count, false, 0, d_out, L.w, st);
}
extern "C" size_t crc_refresh_dev_work_bytes(const crc_ctx *c, size_t count, int in_form) { return refresh_bytes(c, count, in_form, false); }
extern "C" int crc_refresh_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t seed,
                               int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream)
{
    return refresh_impl(c, Reenc::seeded(d_sk, d_pk, false, seed, out_form), d_ct_in, count, in_form, d_ct_out, d_values_out, d_work, S(stream));
}
extern "C" int crc_refresh_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form,
                                   const uint8_t *key, uint64_t stream_base, int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream)
{
    return refresh_impl(c, Reenc::keyed(d_sk, d_pk, false, key, stream_base, out_form), d_ct_in, count, in_form, d_ct_out, d_values_out, d_work, S(stream));
}
// ---- encryption under the secret key and the refresh that uses it (kernels_client.hip: k_encrypt_sym) ----
extern "C" size_t crc_encrypt_sym_dev_work_bytes(const crc_ctx *c, size_t count) { return c ? work_bytes(k_encrypt_sym_work_words(c, count)) : 0; }
extern "C" int crc_encrypt_sym_dev_key_forms(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_plain, size_t count, const uint8_t *key, uint64_t stream_base,
                                             int out_form, uint64_t *d_ct, void *d_work, void *stream)
{
    if (!d_sk || !d_plain || !d_ct || !d_work || !key || !ct_form_ok(out_form)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return k_encrypt_sym(c, d_sk, d_plain, count, chacha_load_key(key), stream_base, d_ct, work_base(d_work), S(stream), out_form == CRC_NTT, false);
}
extern "C" int crc_encrypt_sym_dev_forms(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_plain, size_t count, uint64_t seed, int out_form, uint64_t *d_ct,
                                         void *d_work, void *stream)
{
    if (!d_sk || !d_plain || !d_ct || !d_work || !ct_form_ok(out_form)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return k_encrypt_sym(c, d_sk, d_plain, count, chacha_seed_key(seed), 0, d_ct, work_base(d_work), S(stream), out_form == CRC_NTT, false);
}
extern "C" size_t crc_refresh_sym_dev_work_bytes(const crc_ctx *c, size_t count, int in_form) { return refresh_bytes(c, count, in_form, true); }
extern "C" int crc_refresh_sym_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t seed, int out_form,
                                   uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream)
{
    return refresh_impl(c, Reenc::seeded(d_sk, nullptr, true, seed, out_form), d_ct_in, count, in_form, d_ct_out, d_values_out, d_work, S(stream));
}
extern "C" int crc_refresh_sym_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t count, int in_form, const uint8_t *key,
                                       uint64_t stream_base, int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream)
{
    return refresh_impl(c, Reenc::keyed(d_sk, nullptr, true, key, stream_base, out_form), d_ct_in, count, in_form, d_ct_out, d_values_out, d_work, S(stream));
}
// ---- the refresh of a slot-batched tensor: crc_decrypt_dev, the rescale kernel in place on the plaintexts, the matching encryptor ----
// Work: [plaintexts [count][n]][the tail]
struct SlotsRefreshWork { u64 *plain, *w; };
static SlotsRefreshWork slots_refresh_layout(const crc_ctx *c, size_t count, int in_form, bool sym, WorkArena &a)
{
    SlotsRefreshWork L{};
    L.plain = a.take<u64>(count * (size_t)c->n);
    L.w = a.take<u64>(refresh_tail_words(c, count, in_form, sym, count));
    return L;
}
static size_t slots_refresh_bytes(const crc_ctx *c, size_t count, int in_form, bool sym)
{
    if (!c || !ct_form_ok(in_form)) return 0;
    WorkArena a;
    slots_refresh_layout(c, count, in_form, sym, a);
    return a.bytes();
}
static int slots_refresh_impl(crc_ctx *c, const Reenc &R, const u64 *d_in, size_t count, int in_form, u64 divisor, u64 *d_out, void *d_work, hipStream_t st)
{
    CHECK_CTX(c);
    RUN(slots_rescale_args_ok(c, d_in, d_out, divisor));
    if (!R.ok() || !d_work || !ct_form_ok(in_form)) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena a(d_work);
    const SlotsRefreshWork L = slots_refresh_layout(c, count, in_form, R.sym, a);
    RUN(k_decrypt(c, R.d_sk, d_in, count, 2, in_form == CRC_NTT, L.plain, L.w, st));
    RUN(k_slots_rescale(c, L.plain, count, divisor, L.plain, st));
    return R.run(c, L.plain, count, false, 0, d_out, L.w, st);
}
extern "C" size_t crc_slots_refresh_dev_work_bytes(const crc_ctx *c, size_t count, int in_form) { return slots_refresh_bytes(c, count, in_form, false); }
extern "C" size_t crc_slots_refresh_sym_dev_work_bytes(const crc_ctx *c, size_t count, int in_form) { return slots_refresh_bytes(c, count, in_form, true); }
extern "C" int crc_slots_refresh_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor,
                                     uint64_t seed, int out_form, uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_impl(c, Reenc::seeded(d_sk, d_pk, false, seed, out_form), d_ct_in, count, in_form, divisor, d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form,
                                         uint64_t divisor, const uint8_t *key, uint64_t stream_base, int out_form, uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_impl(c, Reenc::keyed(d_sk, d_pk, false, key, stream_base, out_form), d_ct_in, count, in_form, divisor, d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_sym_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor, uint64_t seed,
                                         int out_form, uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_impl(c, Reenc::seeded(d_sk, nullptr, true, seed, out_form), d_ct_in, count, in_form, divisor, d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_sym_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor,
                                             const uint8_t *key, uint64_t stream_base, int out_form, uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_impl(c, Reenc::keyed(d_sk, nullptr, true, key, stream_base, out_form), d_ct_in, count, in_form, divisor, d_ct_out, d_work, S(stream));
}
// ---- client-side activation of a slot-batched tensor (kernels_slots.hip: k_slots_act) and the refresh that applies it between decrypt and encrypt ----
// the checks of every act entry point, in the order of the rescale's: the context's slots, then the values; in / out are the two tensors
static int slots_act_args_ok(const crc_ctx *c, const void *in, const void *out, size_t planes, const Window &w, uint64_t divisor, int relu, uint64_t cap)
{
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;
    if (!in || !out || divisor < 1 || divisor > ((uint64_t)1 << 62) || (relu != 0 && relu != 1) || cap > ((c->t - 1) >> 1) || !w.ok()) return CRC_ERR_INVALID_ARGUMENT;
    if (((unsigned __int128)planes * (uint64_t)w.xd * (uint64_t)w.yd * (uint64_t)c->n) >> 60) return CRC_ERR_INVALID_ARGUMENT;
    return CRC_OK;
}
static bool slots_act_in_place_ok(const Window &w) { return w.xf == 1 && w.yf == 1 && w.xs == 1 && w.ys == 1; }
extern "C" int crc_slots_act(crc_ctx *c, const uint64_t *h_plain_in, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, uint64_t divisor, int relu,
                             uint64_t cap, uint64_t *h_plain_out)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    const Window w{xd, yd, xs, ys, xf, yf};
    RUN(slots_act_args_ok(c, h_plain_in, h_plain_out, planes, w, divisor, relu, cap));
    return k_slots_act_host(c, h_plain_in, planes, w, divisor, relu, cap, h_plain_out);
}
extern "C" int crc_slots_act_dev(crc_ctx *c, const uint64_t *d_plain_in, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, uint64_t divisor, int relu,
                                 uint64_t cap, uint64_t *d_plain_out, void *stream)
{
    CHECK_CTX(c);
    const Window w{xd, yd, xs, ys, xf, yf};
    RUN(slots_act_args_ok(c, d_plain_in, d_plain_out, planes, w, divisor, relu, cap));
    if (((uintptr_t)d_plain_in & 15) || ((uintptr_t)d_plain_out & 15)) return CRC_ERR_INVALID_ARGUMENT;
    // a workgroup reads window rows that other workgroups write as outputs unless every output row is its own only input row
    const uintptr_t ib = (uintptr_t)d_plain_in, ie = ib + planes * (size_t)xd * yd * c->n * 8, ob = (uintptr_t)d_plain_out, oe = ob + planes * (size_t)w.P64() * c->n * 8;
    if (ib < oe && ob < ie && !(ib == ob && slots_act_in_place_ok(w))) return CRC_ERR_INVALID_ARGUMENT;
    return k_slots_act(c, d_plain_in, planes, w, divisor, relu, cap, d_plain_out, S(stream));
}
// Work: [decrypted plaintexts [planes xd yd][n]][activated plaintexts [planes xo yo][n]: none for a 1 x 1 window of stride 1, which works in place][the tail:
// the decryptor's rows for the inputs, the encryptor's samples for the outputs]
struct SlotsRefreshActWork { u64 *plain, *act, *w; };
static SlotsRefreshActWork slots_refresh_act_layout(const crc_ctx *c, size_t planes, const Window &w, int in_form, bool sym, WorkArena &a)
{
    const size_t in_cts = planes * (size_t)w.xd * w.yd, out_cts = planes * (size_t)w.P64();
    SlotsRefreshActWork L{};
    L.plain = a.take<u64>(in_cts * (size_t)c->n);
    L.act = slots_act_in_place_ok(w) ? L.plain : a.take<u64>(out_cts * (size_t)c->n);
    L.w = a.take<u64>(refresh_tail_words(c, in_cts, in_form, sym, out_cts));
    return L;
}
static size_t slots_refresh_act_bytes(const crc_ctx *c, size_t planes, const Window &w, int in_form, bool sym)
{
    if (!c || !ct_form_ok(in_form) || !w.ok() || (((unsigned __int128)planes * (uint64_t)w.xd * (uint64_t)w.yd * (uint64_t)c->n) >> 60)) return 0;
    WorkArena a;
    slots_refresh_act_layout(c, planes, w, in_form, sym, a);
    return a.bytes();
}
struct SlotsActParams { size_t planes; Window w; u64 divisor; int relu; u64 cap; };
static int slots_refresh_act_impl(crc_ctx *c, const Reenc &R, const u64 *d_in, const SlotsActParams &p, int in_form, u64 *d_out, void *d_work, hipStream_t st)
{
    CHECK_CTX(c);
    RUN(slots_act_args_ok(c, d_in, d_out, p.planes, p.w, p.divisor, p.relu, p.cap));
    if (!R.ok() || !d_work || !ct_form_ok(in_form)) return CRC_ERR_INVALID_ARGUMENT;
    if (!p.planes) return CRC_OK;
    WorkArena a(d_work);
    const SlotsRefreshActWork L = slots_refresh_act_layout(c, p.planes, p.w, in_form, R.sym, a);
    RUN(k_decrypt(c, R.d_sk, d_in, p.planes * (size_t)p.w.xd * p.w.yd, 2, in_form == CRC_NTT, L.plain, L.w, st));
    RUN(k_slots_act(c, L.plain, p.planes, p.w, p.divisor, p.relu, p.cap, L.act, st));
    return R.run(c, L.act, p.planes * (size_t)p.w.P64(), false, 0, d_out, L.w, st);
}
extern "C" size_t crc_slots_refresh_act_dev_work_bytes(const crc_ctx *c, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, int in_form)
{
    return slots_refresh_act_bytes(c, planes, Window{xd, yd, xs, ys, xf, yf}, in_form, false);
}
extern "C" size_t crc_slots_refresh_act_sym_dev_work_bytes(const crc_ctx *c, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, int in_form)
{
    return slots_refresh_act_bytes(c, planes, Window{xd, yd, xs, ys, xf, yf}, in_form, true);
}
extern "C" int crc_slots_refresh_act_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys,
                                         int xf, int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, uint64_t seed, int out_form, uint64_t *d_ct_out,
                                         void *d_work, void *stream)
{
    return slots_refresh_act_impl(c, Reenc::seeded(d_sk, d_pk, false, seed, out_form), d_ct_in, {planes, {xd, yd, xs, ys, xf, yf}, divisor, relu, cap}, in_form,
                                  d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_act_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs,
                                             int ys, int xf, int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *key, uint64_t stream_base,
                                             int out_form, uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_act_impl(c, Reenc::keyed(d_sk, d_pk, false, key, stream_base, out_form), d_ct_in, {planes, {xd, yd, xs, ys, xf, yf}, divisor, relu, cap},
                                  in_form, d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_act_sym_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf,
                                             int in_form, uint64_t divisor, int relu, uint64_t cap, uint64_t seed, int out_form, uint64_t *d_ct_out, void *d_work,
                                             void *stream)
{
    return slots_refresh_act_impl(c, Reenc::seeded(d_sk, nullptr, true, seed, out_form), d_ct_in, {planes, {xd, yd, xs, ys, xf, yf}, divisor, relu, cap}, in_form,
                                  d_ct_out, d_work, S(stream));
}
extern "C" int crc_slots_refresh_act_sym_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys, int xf,
                                                 int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *key, uint64_t stream_base, int out_form,
                                                 uint64_t *d_ct_out, void *d_work, void *stream)
{
    return slots_refresh_act_impl(c, Reenc::keyed(d_sk, nullptr, true, key, stream_base, out_form), d_ct_in, {planes, {xd, yd, xs, ys, xf, yf}, divisor, relu, cap},
                                  in_form, d_ct_out, d_work, S(stream));
}
// ---- several plain moduli: the CRT lift of the slots of r plaintext tensors, the activation on the lifted integers, the refresh that applies it ----
extern "C" int crc_slots_crt_supported(crc_ctx *const *ctxs, int r)
{
    if (!ctxs || r < 1 || r > CRC_SLOTS_CRT_MAX) return 0;
    for (int j = 0; j < r; j++) if (!ctxs[j] || ctxs[j]->n != ctxs[0]->n || ctxs[j]->device != ctxs[0]->device || !crc_slots_supported(ctxs[j])) return 0;
    SlotsCrtBase B;
    return k_slots_crt_base(ctxs, r, &B) ? 1 : 0;
}
// the refusals every entry point shares, in the header's order: the base itself (invalid, then parameters), leaving its constants in B
static int slots_crt_base_ok(crc_ctx *const *ctxs, int r, SlotsCrtBase &B)
{
    if (!ctxs || r < 1 || r > CRC_SLOTS_CRT_MAX) return CRC_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < r; j++) if (!ctxs[j]) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_slots_crt_supported(ctxs, r) || !k_slots_crt_base(ctxs, r, &B)) return CRC_ERR_PARAMETERS;
    return CRC_OK;
}
// an array of r row pointers: none null, none misaligned (align = 1 for host memory)
static bool slots_crt_rows_ok(const uint64_t *const *rows, int r, uintptr_t align)
{
    if (!rows) return false;
    for (int j = 0; j < r; j++) if (!rows[j] || ((uintptr_t)rows[j] & (align - 1))) return false;
    return true;
}
static int slots_crt_decompose_args_ok(const crc_ctx *c, int r, const uint64_t *const *plain, const void *values, int slots, size_t item_stride, size_t slot_stride,
                                       uintptr_t align)
{
    if (!slots_crt_rows_ok(plain, r, align) || !values || slots < 1 || slots > c->n || !item_stride || !slot_stride) return CRC_ERR_INVALID_ARGUMENT;
    if (align > 1 && ((uintptr_t)values & 7)) return CRC_ERR_INVALID_ARGUMENT;
    return CRC_OK;
}
// an output row tensor may be its own input; it overlaps nothing else
static int slots_crt_act_args_ok(const crc_ctx *c, const SlotsCrtBase &B, const uint64_t *const *in, size_t count, uint64_t divisor, int relu, uint64_t cap,
                                 uint64_t *const *out, uintptr_t align)
{
    if (divisor < 1 || divisor > ((uint64_t)1 << 62) || (relu != 0 && relu != 1) || cap > ((B.T - 1) >> 1)) return CRC_ERR_INVALID_ARGUMENT;
    if (!slots_crt_rows_ok(in, B.r, align) || !slots_crt_rows_ok(out, B.r, align)) return CRC_ERR_INVALID_ARGUMENT;
    if (((unsigned __int128)count * (uint64_t)c->n) >> 60) return CRC_ERR_INVALID_ARGUMENT;
    const uintptr_t bytes = count * (size_t)c->n * 8;
    for (int j = 0; j < B.r; j++) {
        const uintptr_t ob = (uintptr_t)out[j], oe = ob + bytes;
        for (int i = 0; i < B.r; i++) {
            const uintptr_t ib = (uintptr_t)in[i], pb = (uintptr_t)out[i];
            if (ib < oe && ob < ib + bytes && !(i == j && ib == ob)) return CRC_ERR_INVALID_ARGUMENT;
            if (i != j && pb < oe && ob < pb + bytes) return CRC_ERR_INVALID_ARGUMENT;
        }
    }
    return CRC_OK;
}
extern "C" int crc_slots_crt_decompose(crc_ctx *const *ctxs, int r, const uint64_t *const *h_plain, size_t count, int slots, int64_t *h_values, size_t item_stride,
                                       size_t slot_stride)
{
    SlotsCrtBase B;
    RUN(slots_crt_base_ok(ctxs, r, B));
    RUN(slots_crt_decompose_args_ok(ctxs[0], r, h_plain, h_values, slots, item_stride, slot_stride, 1));
    return k_slots_crt_decompose_host(ctxs, B, h_plain, count, slots, (long long *)h_values, item_stride, slot_stride);
}
extern "C" int crc_slots_crt_decompose_dev(crc_ctx *const *ctxs, int r, const uint64_t *const *d_plain, size_t count, int slots, int64_t *d_values,
                                           size_t item_stride, size_t slot_stride, void *stream)
{
    SlotsCrtBase B;
    if (!ctxs || r < 1 || r > CRC_SLOTS_CRT_MAX) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(ctxs[0]);
    RUN(slots_crt_base_ok(ctxs, r, B));
    RUN(slots_crt_decompose_args_ok(ctxs[0], r, d_plain, d_values, slots, item_stride, slot_stride, 16));
    return k_slots_crt_decompose(ctxs, B, d_plain, count, slots, (long long *)d_values, item_stride, slot_stride, S(stream));
}
extern "C" int crc_slots_crt_act(crc_ctx *const *ctxs, int r, const uint64_t *const *h_in, size_t count, uint64_t divisor, int relu, uint64_t cap,
                                 uint64_t *const *h_out)
{
    SlotsCrtBase B;
    RUN(slots_crt_base_ok(ctxs, r, B));
    RUN(slots_crt_act_args_ok(ctxs[0], B, h_in, count, divisor, relu, cap, h_out, 1));
    return k_slots_crt_act_host(ctxs, B, h_in, count, divisor, relu, cap, h_out);
}
extern "C" int crc_slots_crt_act_dev(crc_ctx *const *ctxs, int r, const uint64_t *const *d_in, size_t count, uint64_t divisor, int relu, uint64_t cap,
                                     uint64_t *const *d_out, void *stream)
{
    SlotsCrtBase B;
    if (!ctxs || r < 1 || r > CRC_SLOTS_CRT_MAX) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(ctxs[0]);
    RUN(slots_crt_base_ok(ctxs, r, B));
    RUN(slots_crt_act_args_ok(ctxs[0], B, d_in, count, divisor, relu, cap, d_out, 16));
    return k_slots_crt_act(ctxs, B, d_in, count, divisor, relu, cap, d_out, S(stream));
}
// Work: [decrypted plaintexts of modulus j [count][n], j < r: the activation works on them in place][the tail: the largest over the r contexts and over both
// encryptors, so that one size serves either call]
struct SlotsCrtRefreshWork { u64 *plain[CRC_SLOTS_CRT_MAX]; u64 *w; };
static SlotsCrtRefreshWork slots_crt_refresh_layout(crc_ctx *const *ctxs, int r, size_t count, int in_form, WorkArena &a)
{
    SlotsCrtRefreshWork L{};
    size_t w = 0;
    for (int j = 0; j < r; j++) {
        L.plain[j] = a.take<u64>(count * (size_t)ctxs[j]->n);
        for (const bool sym : {false, true}) { const size_t s = refresh_tail_words(ctxs[j], count, in_form, sym, count); w = s > w ? s : w; }
    }
    L.w = a.take<u64>(w);
    return L;
}
extern "C" size_t crc_slots_crt_refresh_dev_work_bytes(crc_ctx *const *ctxs, int r, size_t count, int in_form)
{
    SlotsCrtBase B;
    if (slots_crt_base_ok(ctxs, r, B) || !ct_form_ok(in_form)) return 0;
    WorkArena a;
    slots_crt_refresh_layout(ctxs, r, count, in_form, a);
    return a.bytes();
}
// member j takes the keystream ids stream_base + j count .. + count
static int slots_crt_refresh_impl(crc_ctx *const *ctxs, int r, const Reenc &R, const uint64_t *const *d_in, size_t count, int in_form, u64 divisor, int relu, u64 cap,
                                  uint64_t *const *d_out, void *d_work, hipStream_t st)
{
    SlotsCrtBase B;
    if (!ctxs || r < 1 || r > CRC_SLOTS_CRT_MAX) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(ctxs[0]);
    RUN(slots_crt_base_ok(ctxs, r, B));
    if (divisor < 1 || divisor > ((uint64_t)1 << 62) || (relu != 0 && relu != 1) || cap > ((B.T - 1) >> 1)) return CRC_ERR_INVALID_ARGUMENT;
    if (!slots_crt_rows_ok(d_in, r, 16) || !slots_crt_rows_ok(d_out, r, 16)) return CRC_ERR_INVALID_ARGUMENT;
    if (!R.ok() || !d_work || !ct_form_ok(in_form)) return CRC_ERR_INVALID_ARGUMENT;
    if (!count) return CRC_OK;
    WorkArena a(d_work);
    const SlotsCrtRefreshWork L = slots_crt_refresh_layout(ctxs, r, count, in_form, a);
    for (int j = 0; j < r; j++) RUN(k_decrypt(ctxs[j], R.d_sk, d_in[j], count, 2, in_form == CRC_NTT, L.plain[j], L.w, st));
    RUN(k_slots_crt_act(ctxs, B, L.plain, count, divisor, relu, cap, L.plain, st));
    for (int j = 0; j < r; j++) RUN(R.run(ctxs[j], L.plain[j], count, false, (u64)j * count, d_out[j], L.w, st));
    return CRC_OK;
}
extern "C" int crc_slots_crt_refresh_dev_key(crc_ctx *const *ctxs, int r, const uint64_t *d_sk, const uint64_t *d_pk, const uint64_t *const *d_ct_in, size_t count,
                                             int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *key, uint64_t stream_base, int out_form,
                                             uint64_t *const *d_ct_out, void *d_work, void *stream)
{
    return slots_crt_refresh_impl(ctxs, r, Reenc::keyed(d_sk, d_pk, false, key, stream_base, out_form), d_ct_in, count, in_form, divisor, relu, cap, d_ct_out, d_work,
                                  S(stream));
}
extern "C" int crc_slots_crt_refresh_sym_dev_key(crc_ctx *const *ctxs, int r, const uint64_t *d_sk, const uint64_t *const *d_ct_in, size_t count, int in_form,
                                                 uint64_t divisor, int relu, uint64_t cap, const uint8_t *key, uint64_t stream_base, int out_form,
                                                 uint64_t *const *d_ct_out, void *d_work, void *stream)
{
    return slots_crt_refresh_impl(ctxs, r, Reenc::keyed(d_sk, nullptr, true, key, stream_base, out_form), d_ct_in, count, in_form, divisor, relu, cap, d_ct_out, d_work,
                                  S(stream));
}
// ---- seeded secret-key ciphertexts: the packed c0 rows and a public seed -> ordinary ciphertexts (kernels_client.hip: k_seeded_expand) ----
extern "C" int crc_seeded_expand_dev(crc_ctx *c, const uint64_t *d_c0, size_t count, const uint8_t *seed, uint64_t stream_base, int out_form, uint64_t *d_ct,
                                     void *stream)
{
    if (!d_c0 || !d_ct || !seed || !ct_form_ok(out_form)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    if (count == 0) return CRC_OK;
    // every lane reads its c0 residues from the packed rows and writes them elsewhere: the two ranges must not overlap
    const size_t row = (size_t)c->n * c->k;
    if (count > (size_t)-1 / (16 * row)) return CRC_ERR_INVALID_ARGUMENT;
    const uintptr_t s0 = (uintptr_t)d_c0, s1 = s0 + 8 * count * row, t0 = (uintptr_t)d_ct, t1 = t0 + 16 * count * row;
    if ((s0 < t1 && t0 < s1) || ((s0 | t0) & 15)) return CRC_ERR_INVALID_ARGUMENT;       // (and the 16-byte accesses need their alignment)
    return k_seeded_expand(c, d_c0, count, chacha_load_key(seed), stream_base, d_ct, S(stream), out_form == CRC_NTT);
}
// ---- the seeded form produced on the device (kernels_client.hip: k_encrypt_sym_seeded) ----
// the source (`src_bytes` per ciphertext) and the key must not overlap the packed rows, which are formed in place; the 16-byte accesses need their alignment
static int seeded_enc_ranges_ok(const crc_ctx *c, const void *src, size_t src_bytes, size_t src_align, const void *d_sk, const uint64_t *d_c0, size_t count)
{
    const size_t row = (size_t)c->n * c->k;
    if (count > (size_t)-1 / (16 * row) || count > (size_t)-1 / (2 * src_bytes)) return 0;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + count * src_bytes, t0 = (uintptr_t)d_c0, t1 = t0 + 8 * count * row, k0 = (uintptr_t)d_sk, k1 = k0 + 8 * row;
    if ((s0 < t1 && t0 < s1) || (k0 < t1 && t0 < k1)) return 0;
    return !((t0 | k0) & 15) && !(s0 & (src_align - 1));
}
extern "C" int crc_encrypt_sym_seeded_dev_key(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_plain, size_t count, const uint8_t *key, const uint8_t *seed,
                                              uint64_t stream_base, uint64_t *d_c0, void *stream)
{
    if (!d_sk || !d_plain || !d_c0 || !key || !seed || !std::memcmp(key, seed, CRC_KEY_BYTES)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    if (count == 0) return CRC_OK;
    if (!seeded_enc_ranges_ok(c, d_plain, 8 * (size_t)c->n, 16, d_sk, d_c0, count)) return CRC_ERR_INVALID_ARGUMENT;
    return k_encrypt_sym_seeded(c, d_sk, d_plain, count, chacha_load_key(key), chacha_load_key(seed), stream_base, d_c0, S(stream), false);
}
extern "C" int crc_encrypt_sym_seeded_dev(crc_ctx *c, const uint64_t *d_sk, const uint64_t *d_plain, size_t count, uint64_t seed, uint64_t *d_c0, void *stream)
{
    if (!d_sk || !d_plain || !d_c0) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    if (count == 0) return CRC_OK;
    if (!seeded_enc_ranges_ok(c, d_plain, 8 * (size_t)c->n, 16, d_sk, d_c0, count)) return CRC_ERR_INVALID_ARGUMENT;
    // what crc_encrypt_sym_seeded derives: private key = the expansion of seed, public seed = crc_seeded_public_seed(seed) = the expansion of ~seed
    return k_encrypt_sym_seeded(c, d_sk, d_plain, count, chacha_seed_key(seed), chacha_seed_key(~seed), 0, d_c0, S(stream), false);
}
// pixels in, packed rows out: work = [compact plaintexts [count][96]]
extern "C" size_t crc_encrypt_f32_seeded_dev_work_bytes(const crc_ctx *c, size_t count) { return c ? work_bytes(count * (size_t)CRC_PLAIN_COMPACT_WORDS) : 0; }
static int encrypt_f32_seeded_impl(crc_ctx *c, const u64 *d_sk, const float *d_values, size_t count, const ChaChaKey &key, const ChaChaKey &seed, u64 stream_base,
                                   u64 *d_c0, void *d_work, hipStream_t st)
{
    if (count == 0) return CRC_OK;
    if (c->n <= CRC_PLAIN_COMPACT_WORDS) return CRC_ERR_INVALID_ARGUMENT;
    if (count > (size_t)-1 / (16 * (size_t)CRC_PLAIN_COMPACT_WORDS)) return CRC_ERR_INVALID_ARGUMENT;
    u64 *compact = work_base(d_work);
    // the encoder writes the compact plaintexts while other workgroups still read floats: the two must not overlap either
    { const uintptr_t v0 = (uintptr_t)d_values, v1 = v0 + 4 * count, w0 = (uintptr_t)compact, w1 = w0 + 8 * count * (size_t)CRC_PLAIN_COMPACT_WORDS;
      if (v0 < w1 && w0 < v1) return CRC_ERR_INVALID_ARGUMENT; }
    if (!seeded_enc_ranges_ok(c, d_values, 4, 4, d_sk, d_c0, count) ||
        !seeded_enc_ranges_ok(c, compact, 8 * (size_t)CRC_PLAIN_COMPACT_WORDS, 16, d_sk, d_c0, count)) return CRC_ERR_INVALID_ARGUMENT;
    RUN(k_fra_encode_compact(c, d_values, count, compact, st));
    return k_encrypt_sym_seeded(c, d_sk, compact, count, key, seed, stream_base, d_c0, st, true);
}
extern "C" int crc_encrypt_f32_seeded_dev_key(crc_ctx *c, const uint64_t *d_sk, const float *d_values, size_t count, const uint8_t *key, const uint8_t *seed,
                                              uint64_t stream_base, uint64_t *d_c0, void *d_work, void *stream)
{
    if (!d_sk || !d_values || !d_c0 || !d_work || !key || !seed || !std::memcmp(key, seed, CRC_KEY_BYTES)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return encrypt_f32_seeded_impl(c, d_sk, d_values, count, chacha_load_key(key), chacha_load_key(seed), stream_base, d_c0, d_work, S(stream));
}
extern "C" int crc_encrypt_f32_seeded_dev(crc_ctx *c, const uint64_t *d_sk, const float *d_values, size_t count, uint64_t seed, uint64_t *d_c0, void *d_work,
                                          void *stream)
{
    if (!d_sk || !d_values || !d_c0 || !d_work) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return encrypt_f32_seeded_impl(c, d_sk, d_values, count, chacha_seed_key(seed), chacha_seed_key(~seed), 0, d_c0, d_work, S(stream));
}
extern "C" int crc_square(crc_ctx *c, const uint64_t *d_x, size_t count, uint64_t *d_y3, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y3 || !d_work) return CRC_ERR_INVALID_ARGUMENT;
    u64 *w = work_base(d_work);
    for (size_t o = 0, step = square_chunk(c); o < count; o += step) {
        const size_t ch = pass_len(count, o, step);
        RUN(k_square(c, d_x + o * crc_ct_words(c, 2), ch, d_y3 + o * crc_ct_words(c, 3), w, S(stream)));
    }
    return CRC_OK;
}
extern "C" int crc_relinearize(crc_ctx *c, const uint64_t *d_x3, size_t count, const uint64_t *d_evk, int dbc, uint64_t *d_y, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x3 || !d_y || !d_evk || !d_work || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    u64 *w = work_base(d_work);
    for (size_t o = 0, step = square_chunk(c); o < count; o += step) {
        const size_t ch = pass_len(count, o, step);
        RUN(k_relinearize(c, d_x3 + o * crc_ct_words(c, 3), ch, d_evk, dbc, d_y + o * crc_ct_words(c, 2), w + k_relin_keys_words(c, dbc), w, S(stream), false,
            false, o != 0));
    }
    return CRC_OK;
}
extern "C" int crc_square_relin_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc, uint64_t *d_y, int out_form,
                                      void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, count, 1, 1, dbc, 0, a);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step);
        RUN(k_square(c, d_x + o * crc_ct_words(c, 2), ch, L.y3, L.rest, S(stream), in_form == CRC_NTT, true));
        RUN(k_relinearize(c, L.y3, ch, d_evk, dbc, d_y + o * crc_ct_words(c, 2), L.rest, L.kp, S(stream), out_form == CRC_NTT, true, o != 0));
    }
    return CRC_OK;
}
// Square + relinearise + sum pooling as ONE key switch per pooled ciphertext (kernels_relin64.hip: relin_digits_pool_f64_kernel).  Internal passes take whole
// channel planes (act_layout)
extern "C" int crc_square_pool_relin_supported(const crc_ctx *c, int dbc, int xf, int yf)
{
    return c && dbc_ok(dbc) && c->tune.sq_path != 1 && c->tune.relin_path != 1 && k_relin64_pool_supported(c, dbc, xf * yf) ? 1 : 0;
}
static size_t pool_act_bytes(const crc_ctx *c, int B, int zd, const Window &w, int dbc, int regions)
{
    if (!c || w.xd < w.xf || w.yd < w.yf || w.xs < 1 || w.ys < 1 || !dbc_ok(dbc)) return 0;
    return act_bytes(c, (size_t)B * zd, (size_t)w.xd * w.yd, (size_t)w.P64(), dbc, regions);
}
extern "C" size_t crc_square_pool_relin_work_bytes(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int dbc)
{
    return pool_act_bytes(c, B, zd, {xd, yd, xs, ys, xf, yf}, dbc, 0);
}
extern "C" int crc_square_pool_relin_forms(crc_ctx *c, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
                                           const uint64_t *d_evk, int dbc, const uint64_t *d_div_ntt, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    if (d_div_ntt && out_form != CRC_NTT) return CRC_ERR_INVALID_ARGUMENT;           // the divisor multiplies slot-wise
    if (B < 0 || zd < 1 || xd < xf || yd < yf || xs < 1 || ys < 1 || xf < 1 || yf < 1) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_square_pool_relin_supported(c, dbc, xf, yf)) return CRC_ERR_UNSUPPORTED;
    const PoolGeom pg = pool_geom({xd, yd, xs, ys, xf, yf});
    const size_t planes = (size_t)B * zd, pin = (size_t)xd * yd, pout = (size_t)pg.xo * pg.yo;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, planes, pin, pout, dbc, 0, a);
    for (size_t o = 0; o < planes; o += L.step) {
        const size_t pp = pass_len(planes, o, L.step), cin = pp * pin, cout = pp * pout;
        RUN(k_square(c, d_x + o * pin * crc_ct_words(c, 2), cin, L.y3, L.rest, S(stream), in_form == CRC_NTT, true));
        if (o == 0) RUN(k_relin64_prepare_keys(c, d_evk, dbc, L.kp, L.rest, S(stream)));
        // (the (c0, c1) of a window are added up where the key switch's result meets them: relin_inv_crt_kernel)
        RUN(k_relinearize64(c, L.y3, 3, 2, L.y3, 3, cout, dbc, d_y + o * pout * crc_ct_words(c, 2), L.rest, L.kp, S(stream), out_form == CRC_NTT, &pg, d_div_ntt));
    }
    return CRC_OK;
}
// ---- degree-2 polynomial activation: c2 x^2 + c1 x + c0 in one key switch ----
// The square and the key switch are crc_square_relin_forms' / crc_square_pool_relin_forms'; the ring-linear terms P2 (*) . + P1 (*) Sum_w xh_w + P0 join the NTT-form
// result in the key switch's last kernel (tune.poly_tail = 0, where the key switch runs over the fp64 primes) or in poly2_tail_kernel.  A coefficient-form input is
// transformed pass by pass into work space ([xh of one pass] in front of the square's work space) when P1 needs it, a coefficient-form output is transformed
// back at the end.
static bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}
extern "C" size_t crc_poly2_relin_work_bytes(const crc_ctx *c, size_t count, int dbc) { return c && dbc_ok(dbc) ? act_bytes(c, count, 1, 1, dbc, ACT_XH) : 0; }
extern "C" int crc_poly2_relin_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc, const uint64_t *d_p2_ntt,
                                     const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    if (!d_p2_ntt && !d_p1_ntt && !d_p0_ntt) return crc_square_relin_forms(c, d_x, in_form, count, d_evk, dbc, d_y, out_form, d_work, stream);
    const size_t ctw = crc_ct_words(c, 2);
    // the P1 term reads the NTT-form input after the result's rows are written: the two tensors must not share memory then
    if (d_p1_ntt && in_form == CRC_NTT && ranges_overlap(d_x, 8 * count * ctw, d_y, 8 * count * ctw)) return CRC_ERR_INVALID_ARGUMENT;
    const bool own_xh = d_p1_ntt && in_form == CRC_COEFF;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, count, 1, 1, dbc, own_xh ? ACT_XH : 0, a);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step);
        const u64 *xin = d_x + o * ctw;
        if (own_xh) { RUN(ntt_copy(c, xin, ch, L.xh, stream)); xin = L.xh; }
        u64 *yo = d_y + o * ctw;
        RUN(k_square(c, xin, ch, L.y3, L.rest, S(stream), own_xh || in_form == CRC_NTT, true));
        const PolyTail pt{xin, d_p1_ntt, d_p0_ntt};
        bool fused = false;
        RUN(k_relinearize(c, L.y3, ch, d_evk, dbc, yo, L.rest, L.kp, S(stream), true, true, o != 0, d_p2_ntt, &pt, &fused));
        if (!fused) RUN(k_poly2_tail(c, yo, xin, ch, {1, 1, 1, 1, 1, 1}, d_p2_ntt, d_p1_ntt, d_p0_ntt, S(stream)));
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, count, 2, stream));
    return CRC_OK;
}
extern "C" int crc_poly2_pool_relin_supported(const crc_ctx *c, int dbc, int xf, int yf) { return crc_square_pool_relin_supported(c, dbc, xf, yf); }
extern "C" size_t crc_poly2_pool_relin_work_bytes(const crc_ctx *c, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int dbc)
{
    return pool_act_bytes(c, B, zd, {xd, yd, xs, ys, xf, yf}, dbc, ACT_XH);
}
extern "C" int crc_poly2_pool_relin_forms(crc_ctx *c, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
                                          const uint64_t *d_evk, int dbc, const uint64_t *d_p2_ntt, const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt,
                                          uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    if (B < 0 || zd < 1 || xd < xf || yd < yf || xs < 1 || ys < 1 || xf < 1 || yf < 1) return CRC_ERR_INVALID_ARGUMENT;
    if (!crc_poly2_pool_relin_supported(c, dbc, xf, yf)) return CRC_ERR_UNSUPPORTED;
    if (!d_p2_ntt && !d_p1_ntt && !d_p0_ntt)
        return crc_square_pool_relin_forms(c, d_x, in_form, B, zd, xd, yd, xs, ys, xf, yf, d_evk, dbc, nullptr, d_y, out_form, d_work, stream);
    const PoolGeom pg = pool_geom({xd, yd, xs, ys, xf, yf});
    const size_t planes = (size_t)B * zd, pin = (size_t)xd * yd, pout = (size_t)pg.xo * pg.yo, ctw = crc_ct_words(c, 2);
    if (d_p1_ntt && in_form == CRC_NTT && ranges_overlap(d_x, 8 * planes * pin * ctw, d_y, 8 * planes * pout * ctw)) return CRC_ERR_INVALID_ARGUMENT;
    const bool own_xh = d_p1_ntt && in_form == CRC_COEFF;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, planes, pin, pout, dbc, own_xh ? ACT_XH : 0, a);
    const bool fused = k_relin64_poly_fused(c);
    for (size_t o = 0; o < planes; o += L.step) {
        const size_t pp = pass_len(planes, o, L.step), cin = pp * pin, cout = pp * pout;
        const u64 *xin = d_x + o * pin * ctw;
        if (own_xh) { RUN(ntt_copy(c, xin, cin, L.xh, stream)); xin = L.xh; }
        u64 *yo = d_y + o * pout * ctw;
        RUN(k_square(c, xin, cin, L.y3, L.rest, S(stream), own_xh || in_form == CRC_NTT, true));
        if (o == 0) RUN(k_relin64_prepare_keys(c, d_evk, dbc, L.kp, L.rest, S(stream)));
        const PolyTail pt{xin, d_p1_ntt, d_p0_ntt};
        RUN(k_relinearize64(c, L.y3, 3, 2, L.y3, 3, cout, dbc, yo, L.rest, L.kp, S(stream), true, &pg, fused ? d_p2_ntt : nullptr, fused ? &pt : nullptr));
        if (!fused) RUN(k_poly2_tail(c, yo, xin, pp, {xd, yd, xs, ys, xf, yf}, d_p2_ntt, d_p1_ntt, d_p0_ntt, S(stream)));
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, planes * pout, 2, stream));
    return CRC_OK;
}
// ---- ciphertext x ciphertext multiply, and the degree-3 polynomial activation built on it ----
// Evaluator::multiply for size-2 inputs (k_multiply: the square's chain with the tensor product (ac, ad + bc, bd)); passes, key packing and work layout are
// crc_square_relin_forms'.  The result may not share memory with an input: a pass writes its results while later passes have not read their inputs, and the
// size-3 result of crc_multiply has another stride than its inputs -- every overlap is refused rather than some allowed.  d_x == d_y is the square.
extern "C" size_t crc_multiply_relin_work_bytes(const crc_ctx *c, size_t count, int dbc) { return c && dbc_ok(dbc) ? act_bytes(c, count, 1, 1, dbc, ACT_MULTIPLY) : 0; }
extern "C" int crc_multiply(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_y, size_t count, uint64_t *d_out3, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_out3 || !d_work) return CRC_ERR_INVALID_ARGUMENT;
    const size_t ctw = crc_ct_words(c, 2), ctw3 = crc_ct_words(c, 3);
    if (ranges_overlap(d_x, 8 * count * ctw, d_out3, 8 * count * ctw3) || ranges_overlap(d_y, 8 * count * ctw, d_out3, 8 * count * ctw3)) return CRC_ERR_INVALID_ARGUMENT;
    u64 *w = work_base(d_work);
    for (size_t o = 0, step = square_chunk(c); o < count; o += step) {
        const size_t ch = pass_len(count, o, step);
        RUN(k_multiply(c, d_x + o * ctw, d_y + o * ctw, ch, d_out3 + o * ctw3, w, S(stream)));
    }
    return CRC_OK;
}
extern "C" int crc_multiply_relin_forms(crc_ctx *c, const uint64_t *d_x, const uint64_t *d_y, int in_form, size_t count, const uint64_t *d_evk, int dbc,
                                        uint64_t *d_out, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_y || !d_out || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t ctw = crc_ct_words(c, 2);
    if (ranges_overlap(d_x, 8 * count * ctw, d_out, 8 * count * ctw) || ranges_overlap(d_y, 8 * count * ctw, d_out, 8 * count * ctw)) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, count, 1, 1, dbc, ACT_MULTIPLY, a);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step);
        RUN(k_multiply(c, d_x + o * ctw, d_y + o * ctw, ch, L.y3, L.rest, S(stream), in_form == CRC_NTT, true));
        RUN(k_relinearize(c, L.y3, ch, d_evk, dbc, d_out + o * ctw, L.rest, L.kp, S(stream), out_form == CRC_NTT, true, o != 0));
    }
    return CRC_OK;
}
// c3 x^3 + c2 x^2 + c1 x + c0:  s = relin(x^2), u = relin(s x), result = P3 (*) u + P2 (*) s + P1 (*) x + P0 slot-wise in NTT form (two key switches, depth 2).
// The ring-linear terms join in poly2_tail_kernel; the work space holds x in NTT form and s for one pass in front of crc_multiply_relin_forms' (act_layout)
extern "C" size_t crc_poly3_relin_work_bytes(const crc_ctx *c, size_t count, int dbc) { return c && dbc_ok(dbc) ? act_bytes(c, count, 1, 1, dbc, ACT_XH | ACT_S | ACT_MULTIPLY) : 0; }
extern "C" int crc_poly3_relin_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc, const uint64_t *d_p3_ntt,
                                     const uint64_t *d_p2_ntt, const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt, uint64_t *d_out, int out_form, void *d_work,
                                     void *stream)
{
    CHECK_CTX(c); if (!d_x || !d_out || !d_evk || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t ctw = crc_ct_words(c, 2);
    if (ranges_overlap(d_x, 8 * count * ctw, d_out, 8 * count * ctw)) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena a(d_work);
    const ActWork L = act_layout(c, count, 1, 1, dbc, ACT_XH | ACT_S | ACT_MULTIPLY, a);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step);
        const u64 *xin = d_x + o * ctw;
        if (in_form == CRC_COEFF) { RUN(ntt_copy(c, xin, ch, L.xh, stream)); xin = L.xh; }
        u64 *yo = d_out + o * ctw;
        RUN(k_square(c, xin, ch, L.y3, L.rest, S(stream), true, true));
        RUN(k_relinearize(c, L.y3, ch, d_evk, dbc, L.s, L.rest, L.kp, S(stream), true, true, o != 0));
        RUN(k_multiply(c, L.s, xin, ch, L.y3, L.rest, S(stream), true, true));
        RUN(k_relinearize(c, L.y3, ch, d_evk, dbc, yo, L.rest, L.kp, S(stream), true, true, true));
        RUN(k_poly2_tail(c, yo, L.s, ch, {1, 1, 1, 1, 1, 1}, d_p3_ntt, d_p2_ntt, nullptr, S(stream)));
        RUN(k_poly2_tail(c, yo, xin, ch, {1, 1, 1, 1, 1, 1}, nullptr, d_p1_ntt, d_p0_ntt, S(stream)));
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_out, count, 2, stream));
    return CRC_OK;
}
// ---- Galois automorphisms: Evaluator::apply_galois, rotate_rows, rotate_columns, and the sum over all slots ----
// A step is galois_permute_kernel (kernels_galois.hip) into the size-3 rows (sigma(c0), 0, sigma(c1) (q/q_i)^-1), then relinearisation's key switch with the
// element's key: its tail adds the first two polynomials, which is SEAL's + (temp0, 0).  Steps run one after the other over the whole tensor, each in internal
// passes of whole ciphertexts; the result of a step lives in d_y (a pass is read into work space before its rows are written), so the work space is one pass':
// [coefficient copy of an NTT-form pass][prepared keys of the step's element, made by its pass 0][size-3 rows][scratch of the key switch]
struct GalWork { u64 *xc, *kp, *x3, *rest; size_t step; };
static GalWork gal_layout(const crc_ctx *c, size_t count, int dbc, WorkArena &a)
{
    GalWork L{};
    L.step = square_chunk(c);
    const size_t ch = count < L.step ? count : L.step;
    L.xc = a.take<u64>(ch * crc_ct_words(c, 2));
    L.kp = a.take<u64>(k_relin_keys_words(c, dbc));
    L.x3 = a.take<u64>(ch * crc_ct_words(c, 3));
    L.rest = a.take<u64>(k_relin_work_words(c, ch, dbc));
    return L;
}
static size_t gal_bytes(const crc_ctx *c, size_t count, int dbc)
{
    if (!c || !dbc_ok(dbc)) return 0;
    WorkArena a;
    gal_layout(c, count, dbc, a);
    return a.bytes();
}
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// one step over the whole tensor: src (src_form) -> d_y (coefficient form, or NTT form where out_ntt); src may be d_y itself
static int gal_step(crc_ctx *c, const GalWork &L, const u64 *src, int src_form, size_t count, u64 g, bool accumulate, const u64 *d_key, int dbc, u64 *d_y, bool out_ntt,
                    void *stream)
{
    const size_t ctw = crc_ct_words(c, 2);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step);
        const u64 *xin = src + o * ctw;
        if (src_form == CRC_NTT) { RUN(k_ntt_ct(c, true, xin, L.xc, ch, 2, false, S(stream), nullptr, 0, 0, 0)); xin = L.xc; }
        RUN(k_galois_permute(c, xin, ch, g, accumulate, L.x3, S(stream)));
        RUN(k_relinearize(c, L.x3, ch, d_key, dbc, d_y + o * ctw, L.rest, L.kp, S(stream), out_ntt, true, o != 0));
    }
    return CRC_OK;
}
static int gal_args_ok(const crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_gk, const uint64_t *elts, int n_elts, int dbc,
                       const uint64_t *d_y, int out_form, const void *d_work)
{
    if (!d_x || !d_y || !d_work || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc) || n_elts < 0 || (n_elts && (!elts || !d_gk))) return 0;
    if (!aligned16(d_x) || !aligned16(d_y) || !aligned16(d_gk)) return 0;
    const size_t ctw = crc_ct_words(c, 2), wb = gal_bytes(c, count, dbc);
    if (ranges_overlap(d_work, wb, d_x, 8 * count * ctw) || ranges_overlap(d_work, wb, d_y, 8 * count * ctw)) return 0;     // (every pass is staged there)
    return ranges_overlap(d_x, 8 * count * ctw, d_y, 8 * count * ctw) ? 0 : 1;
}
extern "C" int crc_galois_permute_dev(crc_ctx *c, const uint64_t *d_x, size_t count, uint64_t g, int accumulate, uint64_t *d_x3, void *stream)
{
    CHECK_CTX(c);
    if (!d_x || !d_x3 || !aligned16(d_x) || !aligned16(d_x3) || !crc_galois_elt_valid(c, g)) return CRC_ERR_INVALID_ARGUMENT;
    if (ranges_overlap(d_x, 8 * count * crc_ct_words(c, 2), d_x3, 8 * count * crc_ct_words(c, 3))) return CRC_ERR_INVALID_ARGUMENT;
    return k_galois_permute(c, d_x, count, g, accumulate != 0, d_x3, S(stream));
}
extern "C" size_t crc_apply_galois_work_bytes(const crc_ctx *c, size_t count, int dbc) { return gal_bytes(c, count, dbc); }
extern "C" int crc_apply_galois_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, uint64_t g, const uint64_t *d_gk, const uint64_t *elts, int n_elts,
                                      int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!gal_args_ok(c, d_x, in_form, count, d_gk, elts, n_elts, dbc, d_y, out_form, d_work) || !crc_galois_elt_valid(c, g)) return CRC_ERR_INVALID_ARGUMENT;
    int plan[64];
    const int ns = crc_galois_plan(c, g, elts, n_elts, plan, 64);      // (at most log2 n steps: fewer than 64)
    if (ns < 0) return ns;
    if (count == 0) return CRC_OK;
    const size_t ctw = crc_ct_words(c, 2), kw = crc_evk_words(c, dbc);
    if (ns == 0) {                                                     // g = 1: the same ciphertext in the requested form
        HIPCHK(hipMemcpyAsync(d_y, d_x, 8 * count * ctw, hipMemcpyDeviceToDevice, S(stream)));
        if (in_form == out_form) return CRC_OK;
        return out_form == CRC_NTT ? crc_ntt_fwd(c, d_y, count, 2, stream) : crc_ntt_inv(c, d_y, count, 2, stream);
    }
    WorkArena a(d_work);
    const GalWork L = gal_layout(c, count, dbc, a);
    for (int s = 0; s < ns; s++)
        RUN(gal_step(c, L, s ? d_y : d_x, s ? CRC_COEFF : in_form, count, elts[plan[s]], false, d_gk + (size_t)plan[s] * kw, dbc, d_y,
                     s == ns - 1 && out_form == CRC_NTT, stream));
    return CRC_OK;
}
extern "C" int crc_rotate_rows_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, int steps, const uint64_t *d_gk, const uint64_t *elts, int n_elts,
                                     int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;            // "encryption parameters do not support batching", evaluator.cpp:1790
    const u64 g = crc_galois_elt_rows(c, steps);
    if (!g) return CRC_ERR_INVALID_ARGUMENT;
    return crc_apply_galois_forms(c, d_x, in_form, count, g, d_gk, elts, n_elts, dbc, d_y, out_form, d_work, stream);
}
extern "C" int crc_rotate_columns_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_gk, const uint64_t *elts, int n_elts, int dbc,
                                        uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;
    return crc_apply_galois_forms(c, d_x, in_form, count, crc_galois_elt_columns(c), d_gk, elts, n_elts, dbc, d_y, out_form, d_work, stream);
}
// y = x; y += rotate_rows(y, 2^j) for j < log2(n/2); y += rotate_columns(y): every slot holds the sum of all n.  A step is the permute's accumulate form --
// (sigma(c0) + c0, c1, sigma(c1) ...) -- so the key switch's tail forms y + rotate(y) and no add kernel runs.  Every element must have its own key in the set
extern "C" size_t crc_sum_slots_work_bytes(const crc_ctx *c, size_t count, int dbc) { return gal_bytes(c, count, dbc); }
extern "C" int crc_sum_slots_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_gk, const uint64_t *elts, int n_elts, int dbc,
                                   uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!crc_slots_supported(c)) return CRC_ERR_PARAMETERS;
    if (!gal_args_ok(c, d_x, in_form, count, d_gk, elts, n_elts, dbc, d_y, out_form, d_work)) return CRC_ERR_INVALID_ARGUMENT;
    int idx[64], ns = 0;
    for (int j = 0; j < c->logn; j++) {
        const u64 g = j < c->logn - 1 ? crc_galois_elt_rows(c, 1 << j) : crc_galois_elt_columns(c);
        int at = -1;
        for (int i = 0; i < n_elts; i++) if (elts[i] == g) { at = i; break; }
        if (at < 0) return CRC_ERR_INVALID_ARGUMENT;
        idx[ns++] = at;
    }
    if (count == 0) return CRC_OK;
    const size_t kw = crc_evk_words(c, dbc);
    WorkArena a(d_work);
    const GalWork L = gal_layout(c, count, dbc, a);
    for (int s = 0; s < ns; s++)
        RUN(gal_step(c, L, s ? d_y : d_x, s ? CRC_COEFF : in_form, count, elts[idx[s]], true, d_gk + (size_t)idx[s] * kw, dbc, d_y,
                     s == ns - 1 && out_form == CRC_NTT, stream));
    return CRC_OK;
}
// ---- hoisted rotations: many automorphisms of one ciphertext from one digit decomposition, and the diagonal product that consumes them ----
// With the conjugated key K'_g = sigma_g^-1(K_g) (crc_galois_conjugate_keys),  H_g(ct) := sigma_g((c0, 0) + KeySwitch(c1; K'_g))  decrypts to sigma_g(m).  The key
// switch reads c1 itself, so the digits and their transforms (K1) are made once per pass and serve every element; per element run K2 + K3 into NTT form and the
// NTT-domain gather.  Where the fp64 key switch does not apply, k_relinearize runs per element with the conjugated key: the same exact function on Z_q.
// Every entry point of the family is the same driver around its own consumer kernel.  After the argument checks it carves the work space and builds one
// HoistCall; hoist_prepare_keys makes the fp64 form of the call's keys; then, per pass of L.step ciphertexts, hoist_pass_head makes the digits of the pass and
// hoist_group turns GALOIS_DIAG_MAX elements at a time into the operands z[] of the consumer.  A stage that rotates sums it has just formed (the giant stage, the
// dense layer's outer stage) takes each through hoist_switch_own.
// Work: [coefficient copy of an NTT-form pass][size-3 rows (c0, 0, c1 (q/q_i)^-1)][zc key-switch results of a pass][nk prepared keys][scratch of the key
// switch].  A pass is square_chunk ciphertexts, fewer once more than 8 results are kept at once: it shrinks with R.
struct HoistWork { u64 *xc, *x3, *z, *kp, *rest, *u; size_t step, kpw; };
enum { HOIST_Z_PASSES = 8 };
// uc: further ciphertexts a pass keeps besides the zc results (the inner sums of crc_diag_mac_bsgs_forms; none elsewhere), in L.u behind every other region
static HoistWork hoist_layout(const crc_ctx *c, size_t count, int nk, int zc, int dbc, WorkArena &a, int uc = 0)
{
    HoistWork L{};
    // (the zc results kept at once may take the room of HOIST_Z_PASSES passes' ciphertexts: up to 8 of them leave the pass whole, 32 make it a quarter)
    L.step = square_chunk(c) * HOIST_Z_PASSES / ((size_t)zc + (size_t)uc);
    if (L.step > square_chunk(c)) L.step = square_chunk(c);
    if (L.step < 1) L.step = 1;
    const size_t ch = count < L.step ? count : L.step;
    L.kpw = (k_relin_keys_words(c, dbc) + 31) & ~(size_t)31;
    L.xc = a.take<u64>(ch * crc_ct_words(c, 2));
    L.x3 = a.take<u64>(ch * crc_ct_words(c, 3));
    L.z = a.take<u64>((size_t)zc * ch * crc_ct_words(c, 2));
    L.kp = a.take<u64>((size_t)nk * L.kpw);
    const size_t one = k_relin_work_words(c, ch, dbc), two = k_relin64_supported(c, dbc) ? k_relin64_work_words_multi(c, ch, dbc, 2) : 0;
    L.rest = a.take<u64>(one > two ? one : two);                        // (either setting of hoist_rt: a tuning switch does not change the size)
    if (uc) L.u = a.take<u64>((size_t)uc * ch * crc_ct_words(c, 2));
    return L;
}
// keys per digit load in K2: HOIST_RT_DEFAULT unless the tuning key "hoist_rt" says otherwise (profiles/galois_hoisted.md has both measured)
enum { HOIST_RT_DEFAULT = 2 };
static int hoist_rt(const crc_ctx *c) { return c->tune.hoist_rt ? c->tune.hoist_rt : (int)HOIST_RT_DEFAULT; }
static int diag_zc(int R) { return R < GALOIS_DIAG_MAX ? R : (int)GALOIS_DIAG_MAX; }
static size_t hoist_bytes(const crc_ctx *c, size_t count, int R, int zc, int dbc)
{
    if (!c || !dbc_ok(dbc) || R < 1) return 0;
    WorkArena a;
    hoist_layout(c, count, R, zc, dbc, a);
    return a.bytes();
}
// the key of every element of gs in the set (-1 for g = 1); false where one is invalid or missing
static bool hoist_keys(const crc_ctx *c, const uint64_t *gs, int R, const uint64_t *elts, int n_elts, int *at)
{
    for (int r = 0; r < R; r++) {
        if (!crc_galois_elt_valid(c, gs[r])) return false;
        at[r] = -1;
        if (gs[r] == 1) continue;
        for (int i = 0; i < n_elts; i++) if (elts[i] == gs[r]) { at[r] = i; break; }
        if (at[r] < 0) return false;
    }
    return true;
}
static int hoist_args_ok(const crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gs, int R, const uint64_t *d_cgk, const uint64_t *elts,
                         int n_elts, int dbc, const uint64_t *d_y, size_t y_cts, int out_form, const void *d_work, size_t wb)
{
    if (!d_x || !d_y || !d_work || !gs || R < 1 || !form_ok(in_form) || !form_ok(out_form) || !dbc_ok(dbc) || n_elts < 0 || (n_elts && (!elts || !d_cgk))) return 0;
    if (!aligned16(d_x) || !aligned16(d_y) || !aligned16(d_cgk)) return 0;
    const size_t ctw = crc_ct_words(c, 2);
    if (ranges_overlap(d_work, wb, d_x, 8 * count * ctw) || ranges_overlap(d_work, wb, d_y, 8 * y_cts * ctw)) return 0;
    return ranges_overlap(d_x, 8 * count * ctw, d_y, 8 * y_cts * ctw) ? 0 : 1;
}
// the read-only operand of a consumer (plaintext rows, packed weights): there, aligned, and apart from everything the call writes
static int hoist_operand_ok(const crc_ctx *c, const uint64_t *d_op, size_t op_bytes, const uint64_t *d_y, size_t y_cts, const void *d_work, size_t wb)
{
    if (!d_op || !aligned16(d_op)) return 0;
    return ranges_overlap(d_op, op_bytes, d_y, 8 * y_cts * crc_ct_words(c, 2)) || ranges_overlap(d_op, op_bytes, d_work, wb) ? 0 : 1;
}
// One call of the family, built once after the argument checks.  at[r]: the key of element r in the set (hoist_keys), whose prepared form lives in slot r of L.kp
// unless a caller says otherwise; elements [0, n) are the ones hoist_group serves (further ones: the giant elements).  f64: the fp64 key switch runs; pair: two
// keys per digit load in its K2; keyed: one of the n elements has a key, so the digits of a pass are needed at all
struct HoistCall { crc_ctx *c; HoistWork L; const u64 *d_cgk; int dbc; void *stream; std::vector<int> at; bool f64, pair, keyed; };
static HoistCall hoist_call(crc_ctx *c, const HoistWork &L, const u64 *d_cgk, int dbc, void *stream, std::vector<int> at, int n)
{
    HoistCall H{c, L, d_cgk, dbc, stream, std::move(at), false, false, false};
    H.f64 = c->tune.relin_path != 1 && k_relin64_supported(c, dbc);
    H.pair = H.f64 && hoist_rt(c) == 2;
    for (int r = 0; r < n; r++) H.keyed = H.keyed || H.at[r] >= 0;
    return H;
}
// the fp64 form of the keys of elements [first, first + n) into their slots, once per call.  The preparation borrows the scratch, so it runs before the first
// pass puts E there.  (The other path prepares a key inside the first k_relinearize that uses it: hoist_switch's `first`.)
static int hoist_prepare_keys(const HoistCall &H, int first, int n)
{
    if (!H.f64) return CRC_OK;
    const size_t kw = crc_evk_words(H.c, H.dbc);
    for (int r = first; r < first + n; r++)
        if (H.at[r] >= 0) RUN(k_relin64_prepare_keys(H.c, H.d_cgk + (size_t)H.at[r] * kw, H.dbc, H.L.kp + (size_t)r * H.L.kpw, H.L.rest, S(H.stream)));
    return CRC_OK;
}
// one pass' operand and digits: xin (in_form) -> L.x3 = (c0, 0, c1 (q/q_i)^-1) and, on the fp64 path, E in L.rest
static int hoist_pass_head(const HoistCall &H, const u64 *xin, int in_form, size_t ch)
{
    const HoistWork &L = H.L;
    if (in_form == CRC_NTT) { RUN(k_ntt_ct(H.c, true, xin, L.xc, ch, 2, false, S(H.stream), nullptr, 0, 0, 0)); xin = L.xc; }
    RUN(k_galois_permute(H.c, xin, ch, 1, false, L.x3, S(H.stream)));
    return H.f64 ? k_relin64_digits(H.c, L.x3, 3, 2, ch, H.dbc, L.rest, S(H.stream)) : CRC_OK;
}
// (c0, 0) + KeySwitch(c1; K'_g) of the pass in NTT form -> z, for element r with its prepared key in `slot`.  first: nothing has prepared that slot yet
static int hoist_switch(const HoistCall &H, size_t ch, int r, int slot, bool first, u64 *z)
{
    const HoistWork &L = H.L;
    if (H.f64) return k_relin64_from_digits(H.c, L.x3, 3, ch, H.dbc, z, L.rest, L.kp + (size_t)slot * L.kpw, S(H.stream), true);
    return k_relinearize(H.c, L.x3, ch, H.d_cgk + (size_t)H.at[r] * crc_evk_words(H.c, H.dbc), H.dbc, z, L.rest, L.kp + (size_t)slot * L.kpw, S(H.stream), true, true,
                         !first);
}
// the same for the two elements ra, rb with one read of the digit values (fp64 path only)
static int hoist_switch2(const HoistCall &H, size_t ch, int ra, int rb, u64 *za, u64 *zb)
{
    const HoistWork &L = H.L;
    return k_relin64_from_digits2(H.c, L.x3, 3, ch, H.dbc, za, zb, L.rest, L.kp + (size_t)ra * L.kpw, L.kp + (size_t)rb * L.kpw, S(H.stream), true);
}
// a key switch of an inner sum on its own digits: u (NTT form, ch ciphertexts) -> inverse transform, (c0, 0, c1 (q/q_i)^-1), K1, K2 + K3 under the key of
// element r -> over u, which nothing reads any more
static int hoist_switch_own(const HoistCall &H, u64 *u, size_t ch, int r, int slot, bool first)
{
    RUN(hoist_pass_head(H, u, CRC_NTT, ch));
    return hoist_switch(H, ch, r, slot, first, u);
}
// The operands of elements [r0, r0 + rn) of one pass, rn <= the zc of the layout: z[i] is (c0, 0) + KeySwitch(c1; K'_g) in slot i of L.z for a keyed element
// and the pass itself in NTT form for g = 1 -- xin on NTT input, otherwise ONE transformed copy per group that its elements 1 share.  Where two keys go per digit
// load a keyed element waits for the next keyed one of the group and the two share a K2; the last runs alone.  first: as hoist_switch
static int hoist_group(const HoistCall &H, const u64 *xin, int in_form, size_t ch, bool first, int r0, int rn, const u64 **z)
{
    const size_t uj = ch * crc_ct_words(H.c, 2);
    const u64 *same = in_form == CRC_NTT ? xin : nullptr;
    int held = -1;
    for (int i = 0; i < rn; i++) {
        const int r = r0 + i;
        u64 *zi = H.L.z + (size_t)i * uj;
        z[i] = zi;
        if (H.at[r] < 0) {
            if (!same) { RUN(ntt_copy(H.c, xin, ch, zi, H.stream)); same = zi; }
            z[i] = same;
        }
        else if (!H.pair) RUN(hoist_switch(H, ch, r, r, first, zi));
        else if (held < 0) held = i;
        else { RUN(hoist_switch2(H, ch, r0 + held, r, H.L.z + (size_t)held * uj, zi)); held = -1; }
    }
    if (held >= 0) RUN(hoist_switch(H, ch, r0 + held, r0 + held, first, H.L.z + (size_t)held * uj));
    return CRC_OK;
}
extern "C" int crc_galois_permute_ntt_dev(crc_ctx *c, const uint64_t *d_in, size_t rows, uint64_t g, uint64_t *d_out, void *stream)
{
    CHECK_CTX(c);
    if (!d_in || !d_out || !aligned16(d_in) || !aligned16(d_out) || !crc_galois_elt_valid(c, g)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t bytes = 8 * rows * (size_t)c->k * c->n;
    if (ranges_overlap(d_in, bytes, d_out, bytes)) return CRC_ERR_INVALID_ARGUMENT;
    return k_galois_permute_ntt(c, d_in, rows * (size_t)c->k, g, d_out, S(stream));
}
extern "C" int crc_galois_conjugate_keys_dev(crc_ctx *c, const uint64_t *elts, int n_elts, int dbc, const uint64_t *d_gk, uint64_t *d_out, void *stream)
{
    CHECK_CTX(c);
    if (!dbc_ok(dbc) || n_elts < 0 || (n_elts && (!elts || !d_gk || !d_out)) || !aligned16(d_gk) || !aligned16(d_out)) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_elts; e++) if (!crc_galois_elt_valid(c, elts[e]) || elts[e] == 1) return CRC_ERR_INVALID_ARGUMENT;
    const size_t kw = crc_evk_words(c, dbc);
    if (ranges_overlap(d_gk, 8 * kw * n_elts, d_out, 8 * kw * n_elts)) return CRC_ERR_INVALID_ARGUMENT;
    const u64 mask = 2 * (u64)c->n - 1;
    for (int e = 0; e < n_elts; e++) {
        u64 h = 1;                                                      // g^-1 = g^(n - 1) mod 2n
        for (u64 x = elts[e] & mask, p = (u64)c->n - 1; p; p >>= 1, x = x * x & mask) if (p & 1) h = h * x & mask;
        RUN(k_galois_permute_ntt(c, d_gk + (size_t)e * kw, kw / c->n, h, d_out + (size_t)e * kw, S(stream)));
    }
    return CRC_OK;
}
// ---- seeded key-switching keys: first rows made on the device, and their expansion into ordinary blobs (kernels_seeded_keys.hip) ----
// ids: 0 (the evaluation key) or valid Galois elements; conjugate: 0 and 1 have no conjugated key
static bool seeded_key_ids_ok(const crc_ctx *c, const uint64_t *ids, int n_ids, bool conjugate)
{
    for (int e = 0; e < n_ids; e++) if ((ids[e] && !crc_galois_elt_valid(c, ids[e])) || (conjugate && ids[e] <= 1)) return false;
    return true;
}
static int gen_keys_seeded_dev_impl(crc_ctx *c, const ChaChaKey &key, const ChaChaKey &seed, const u64 *d_sk, int dbc, const uint64_t *ids, int n_ids, u64 *d_first,
                                    hipStream_t st)
{
    if (!own_gadget(c)) return CRC_ERR_PARAMETERS;                      // a level with an inherited gadget takes its keys from above (crc_keys_restrict*)
    if (!dbc_ok(dbc) || n_ids < 0) return CRC_ERR_INVALID_ARGUMENT;
    if (n_ids == 0) return CRC_OK;
    if (!ids || !d_first || !aligned16(d_sk) || !aligned16(d_first) || !k_seeded_keys_grid_ok(c, dbc, n_ids) || !seeded_key_ids_ok(c, ids, n_ids, false))
        return CRC_ERR_INVALID_ARGUMENT;
    // the rows are formed in place while every lane reads the secret key: the two must not overlap
    if (ranges_overlap(d_sk, 8 * (size_t)c->k * c->n, d_first, 4 * crc_evk_words(c, dbc) * n_ids)) return CRC_ERR_INVALID_ARGUMENT;
    return k_gen_keys_seeded(c, d_sk, dbc, ids, n_ids, key, seed, d_first, st);
}
extern "C" int crc_gen_keys_seeded_dev_key(crc_ctx *c, const uint8_t *key, const uint8_t *seed, const uint64_t *d_sk, int dbc, const uint64_t *ids, int n_ids,
                                           uint64_t *d_first, void *stream)
{
    if (!key || !seed || !d_sk || !std::memcmp(key, seed, CRC_KEY_BYTES)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    return gen_keys_seeded_dev_impl(c, chacha_load_key(key), chacha_load_key(seed), d_sk, dbc, ids, n_ids, d_first, S(stream));
}
extern "C" int crc_gen_keys_seeded_dev(crc_ctx *c, uint64_t seed, const uint64_t *d_sk, int dbc, const uint64_t *ids, int n_ids, uint64_t *d_first, void *stream)
{
    if (!d_sk) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    // what crc_gen_keys_seeded derives: private key = the expansion of seed, public seed = crc_seeded_public_seed(seed)
    return gen_keys_seeded_dev_impl(c, chacha_seed_key(seed), chacha_seed_key(~seed), d_sk, dbc, ids, n_ids, d_first, S(stream));
}
extern "C" int crc_seeded_keys_expand_dev(crc_ctx *c, const uint64_t *d_first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *seed, int conjugate,
                                          uint64_t *d_out, void *stream)
{
    if (!seed || (conjugate != 0 && conjugate != 1)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(c);
    if (!dbc_ok(dbc) || n_ids < 0) return CRC_ERR_INVALID_ARGUMENT;
    if (n_ids == 0) return CRC_OK;
    if (!d_first || !ids || !d_out || !aligned16(d_first) || !aligned16(d_out) || !k_seeded_keys_grid_ok(c, dbc, n_ids) ||
        !seeded_key_ids_ok(c, ids, n_ids, conjugate != 0)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t kw = crc_evk_words(c, dbc);
    if (ranges_overlap(d_first, 4 * kw * n_ids, d_out, 8 * kw * n_ids)) return CRC_ERR_INVALID_ARGUMENT;
    return k_seeded_keys_expand(c, d_first, ids, n_ids, dbc, chacha_load_key(seed), conjugate != 0, d_out, S(stream));
}
// ---- keys of a level from the keys of the context above it (crc_ctx_create_level; kernels_seeded_keys.hip) ----
extern "C" int crc_keys_restrict_supported(const crc_ctx *from, const crc_ctx *to) { return keys_level_of(from, to) ? 1 : 0; }
extern "C" int crc_keys_restrict_dev(crc_ctx *from, const crc_ctx *to, const uint64_t *d_keys, int n_keys, int dbc, uint64_t *d_out, void *stream)
{
    CHECK_CTX(from);
    if (!keys_level_of(from, to) || !dbc_ok(dbc) || n_keys < 0) return CRC_ERR_INVALID_ARGUMENT;
    if (n_keys == 0) return CRC_OK;
    if (!d_keys || !d_out || !aligned16(d_keys) || !aligned16(d_out) || !k_seeded_keys_grid_ok(from, dbc, n_keys) || !k_seeded_keys_grid_ok(to, dbc, n_keys))
        return CRC_ERR_INVALID_ARGUMENT;
    if (ranges_overlap(d_keys, 8 * crc_evk_words(from, dbc) * n_keys, d_out, 8 * crc_evk_words(to, dbc) * n_keys)) return CRC_ERR_INVALID_ARGUMENT;
    return k_keys_restrict(from, to, d_keys, n_keys, dbc, d_out, S(stream));
}
extern "C" int crc_seeded_keys_expand_level_dev(crc_ctx *from, const crc_ctx *to, const uint64_t *d_first, const uint64_t *ids, int n_ids, int dbc,
                                                const uint8_t *seed, int conjugate, uint64_t *d_out, void *stream)
{
    if (!seed || (conjugate != 0 && conjugate != 1)) return CRC_ERR_INVALID_ARGUMENT;
    CHECK_CTX(from);
    if (!keys_level_of(from, to) || !dbc_ok(dbc) || n_ids < 0) return CRC_ERR_INVALID_ARGUMENT;
    if (n_ids == 0) return CRC_OK;
    if (!d_first || !ids || !d_out || !aligned16(d_first) || !aligned16(d_out) || !k_seeded_keys_grid_ok(from, dbc, n_ids) || !k_seeded_keys_grid_ok(to, dbc, n_ids) ||
        !seeded_key_ids_ok(from, ids, n_ids, conjugate != 0)) return CRC_ERR_INVALID_ARGUMENT;
    if (ranges_overlap(d_first, 4 * crc_evk_words(from, dbc) * n_ids, d_out, 8 * crc_evk_words(to, dbc) * n_ids)) return CRC_ERR_INVALID_ARGUMENT;
    return k_seeded_keys_expand_level(from, to, d_first, ids, n_ids, dbc, chacha_load_key(seed), conjugate != 0, d_out, S(stream));
}
extern "C" size_t crc_rotate_hoisted_work_bytes(const crc_ctx *c, size_t count, int R, int dbc) { return hoist_bytes(c, count, R, 2, dbc); }
extern "C" int crc_rotate_hoisted_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gs, int R, const uint64_t *d_cgk,
                                        const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (R < 1 || R > (1 << 20)) return CRC_ERR_INVALID_ARGUMENT;
    if (!hoist_args_ok(c, d_x, in_form, count, gs, R, d_cgk, elts, n_elts, dbc, d_y, (size_t)R * count, out_form, d_work, hoist_bytes(c, count, R, 2, dbc)))
        return CRC_ERR_INVALID_ARGUMENT;
    std::vector<int> at((size_t)R);
    if (!hoist_keys(c, gs, R, elts, n_elts, at.data())) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    const size_t ctw = crc_ct_words(c, 2);
    std::vector<int> idx, kat;                                          // the keyed elements alone: where each result goes, its key; element i has key slot i
    std::vector<u64> kg;
    for (int r = 0; r < R; r++) {
        if (at[r] >= 0) { idx.push_back(r); kat.push_back(at[r]); kg.push_back(gs[r]); continue; }
        u64 *yr = d_y + (size_t)r * count * ctw;                       // g = 1: the same ciphertext in the requested form
        HIPCHK(hipMemcpyAsync(yr, d_x, 8 * count * ctw, hipMemcpyDeviceToDevice, S(stream)));
        if (in_form != out_form) RUN(out_form == CRC_NTT ? crc_ntt_fwd(c, yr, count, 2, stream) : crc_ntt_inv(c, yr, count, 2, stream));
    }
    const int nk = (int)idx.size();
    if (!nk) return CRC_OK;
    WorkArena a(d_work);
    const HoistCall H = hoist_call(c, hoist_layout(c, count, R, 2, dbc, a), d_cgk, dbc, stream, kat, nk);
    const int gw = H.pair ? 2 : 1;                                      // a group is what shares a K2: each keyed element with the next keyed one
    RUN(hoist_prepare_keys(H, 0, nk));
    for (size_t o = 0; o < count; o += H.L.step) {
        const size_t ch = pass_len(count, o, H.L.step);
        RUN(hoist_pass_head(H, d_x + o * ctw, in_form, ch));
        for (int r0 = 0; r0 < nk; r0 += gw) {
            const int rn = nk - r0 < gw ? nk - r0 : gw;
            const u64 *z[2];
            RUN(hoist_group(H, d_x + o * ctw, in_form, ch, o == 0, r0, rn, z));
            for (int i = 0; i < rn; i++) {
                u64 *yr = d_y + ((size_t)idx[r0 + i] * count + o) * ctw;
                RUN(k_galois_permute_ntt(c, z[i], ch * 2 * c->k, kg[r0 + i], yr, S(stream)));
                if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, yr, ch, 2, stream));
            }
        }
    }
    return CRC_OK;
}
// y = Sum_r P_r (*) H_{g_r}(x): the hoisted rotations above with galois_diag_mac_kernel in the place of the gather, GALOIS_DIAG_MAX elements at a time.  Canonical
// residues throughout: bit for bit crc_rotate_hoisted_forms, then crc_multiply_plain_ntt, then crc_add
extern "C" size_t crc_diag_mac_work_bytes(const crc_ctx *c, size_t count, int R, int dbc) { return hoist_bytes(c, count, R, diag_zc(R), dbc); }
extern "C" int crc_diag_mac_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gs, int R, const uint64_t *d_p_ntt, const uint64_t *d_cgk,
                                  const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (R < 1 || R > (1 << 20)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t wb = hoist_bytes(c, count, R, diag_zc(R), dbc), ctw = crc_ct_words(c, 2), rowp = (size_t)c->k * c->n;
    if (!hoist_args_ok(c, d_x, in_form, count, gs, R, d_cgk, elts, n_elts, dbc, d_y, count, out_form, d_work, wb) ||
        !hoist_operand_ok(c, d_p_ntt, 8 * (size_t)R * rowp, d_y, count, d_work, wb)) return CRC_ERR_INVALID_ARGUMENT;
    std::vector<int> at((size_t)R);
    if (!hoist_keys(c, gs, R, elts, n_elts, at.data())) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    const int zc = diag_zc(R);
    WorkArena a(d_work);
    const HoistCall H = hoist_call(c, hoist_layout(c, count, R, zc, dbc, a), d_cgk, dbc, stream, at, R);
    RUN(hoist_prepare_keys(H, 0, R));
    for (size_t o = 0; o < count; o += H.L.step) {
        const size_t ch = pass_len(count, o, H.L.step);
        const u64 *xin = d_x + o * ctw;
        RUN(hoist_pass_head(H, xin, in_form, ch));
        for (int r0 = 0; r0 < R; r0 += zc) {
            const int rn = R - r0 < zc ? R - r0 : zc;
            const u64 *z[GALOIS_DIAG_MAX], *p[GALOIS_DIAG_MAX];
            RUN(hoist_group(H, xin, in_form, ch, o == 0, r0, rn, z));
            for (int i = 0; i < rn; i++) p[i] = d_p_ntt + (size_t)(r0 + i) * rowp;
            RUN(k_galois_diag_mac(c, z, p, gs + r0, rn, ch, r0 != 0, d_y + o * ctw, S(stream)));
        }
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, count, 2, stream));
    return CRC_OK;
}
// ---- baby-step / giant-step: y = Sum_j H_{gg[j]}( Sum_b P[j][b] (*) H_{gb[b]}(x) ) ----
// The baby stage is crc_diag_mac_forms' with G plaintext rows per element: one digit decomposition of x, the B key-switch results Z_b kept (GALOIS_DIAG_MAX at a time),
// galois_diag_mac_multi_kernel into the G inner sums u_j.  The giant stage takes each u_j with gg[j] != 1 through the hoisted key switch on its own digits -- inverse
// transform, (c0, 0, c1 (q/q_i)^-1), K1, K2 + K3 under K'_{gg[j]} -- and writes the result over u_j, which nothing reads any more; galois_sum_permuted_kernel then
// gathers and sums all G (gg[j] = 1: u_j itself).  Every step is an exact function on Z_q with canonical residues, so the bits are those of crc_diag_mac_forms per j,
// crc_rotate_hoisted_forms per j, crc_add.  Work: hoist_layout with B + G prepared keys, min(B, GALOIS_DIAG_MAX) results and the G inner sums kept per pass.
// the inner sums: BSGS_JT_DEFAULT unless the tuning key "bsgs_jt" says otherwise (profiles/matvec_bsgs.md has both measured).  The same exact function either way
enum { BSGS_JT_DEFAULT = 2 };
static int bsgs_jt(const crc_ctx *c) { return c->tune.bsgs_jt ? c->tune.bsgs_jt : (int)BSGS_JT_DEFAULT; }
static bool bsgs_counts_ok(int B, int G) { return B >= 1 && G >= 1 && B <= GALOIS_BSGS_MAX && G <= GALOIS_BSGS_MAX; }
static size_t bsgs_bytes(const crc_ctx *c, size_t count, int B, int G, int dbc)
{
    if (!c || !dbc_ok(dbc) || !bsgs_counts_ok(B, G)) return 0;
    WorkArena a;
    hoist_layout(c, count, B + G, diag_zc(B), dbc, a, G);
    return a.bytes();
}
extern "C" size_t crc_diag_mac_bsgs_work_bytes(const crc_ctx *c, size_t count, int B, int G, int dbc) { return bsgs_bytes(c, count, B, G, dbc); }
extern "C" int crc_diag_mac_bsgs_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gb, int B, const uint64_t *gg, int G,
                                       const uint64_t *d_p_ntt, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y, int out_form,
                                       void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!bsgs_counts_ok(B, G) || !gg) return CRC_ERR_INVALID_ARGUMENT;
    const size_t wb = bsgs_bytes(c, count, B, G, dbc), ctw = crc_ct_words(c, 2), rowp = (size_t)c->k * c->n;
    if (!hoist_args_ok(c, d_x, in_form, count, gb, B, d_cgk, elts, n_elts, dbc, d_y, count, out_form, d_work, wb) ||
        !hoist_operand_ok(c, d_p_ntt, 8 * (size_t)G * B * rowp, d_y, count, d_work, wb)) return CRC_ERR_INVALID_ARGUMENT;
    std::vector<int> at((size_t)B + G);                                 // the key of every baby element, then of every giant element
    if (!hoist_keys(c, gb, B, elts, n_elts, at.data()) || !hoist_keys(c, gg, G, elts, n_elts, at.data() + B)) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    const int zc = diag_zc(B);
    WorkArena a(d_work);
    const HoistCall H = hoist_call(c, hoist_layout(c, count, B + G, zc, dbc, a, G), d_cgk, dbc, stream, at, B);
    const HoistWork &L = H.L;
    const bool flat = G == 1 && gg[0] == 1;                             // one inner sum that is the result: crc_diag_mac_forms
    std::vector<const u64 *> zs((size_t)G);
    RUN(hoist_prepare_keys(H, 0, B + G));
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step), uj = ch * ctw;
        const u64 *xin = d_x + o * ctw;
        u64 *u = flat ? d_y + o * ctw : L.u;
        if (H.keyed) RUN(hoist_pass_head(H, xin, in_form, ch));         // (no digits of x where every baby element is 1)
        for (int r0 = 0; r0 < B; r0 += zc) {
            const int rn = B - r0 < zc ? B - r0 : zc;
            const u64 *z[GALOIS_DIAG_MAX], *p[GALOIS_DIAG_MAX];
            RUN(hoist_group(H, xin, in_form, ch, o == 0, r0, rn, z));
            if (bsgs_jt(c) == 2) { RUN(k_galois_diag_mac_multi(c, z, gb + r0, r0, rn, B, d_p_ntt, G, ch, r0 != 0, u, S(stream))); continue; }
            for (int j = 0; j < G; j++) {
                for (int i = 0; i < rn; i++) p[i] = d_p_ntt + ((size_t)j * B + r0 + i) * rowp;
                RUN(k_galois_diag_mac(c, z, p, gb + r0, rn, ch, r0 != 0, u + (size_t)j * uj, S(stream)));
            }
        }
        if (flat) continue;
        for (int j = 0; j < G; j++) {
            u64 *ug = L.u + (size_t)j * uj;
            zs[j] = ug;
            if (at[B + j] >= 0) RUN(hoist_switch_own(H, ug, ch, B + j, B + j, o == 0));
        }
        RUN(k_galois_sum_permuted(c, zs.data(), gg, G, ch, false, d_y + o * ctw, S(stream)));
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, count, 2, stream));
    return CRC_OK;
}
// ---- the packed convolution over slots: y[co] = Sum_ci Sum_tau w[co][ci][tau] H_{gs[tau]}(x[ci]) with scalar weights ----
// crc_diag_mac_forms' passes over the FLAT input x [Cin][count] -- a pass is L.step consecutive ciphertexts whatever their channel, so one image of 32 channels is one
// pass, not 32 -- with galois_conv_mac_kernel in the place of the diagonal product: one digit decomposition per input ciphertext, one key switch per (input
// ciphertext, tap), and every rotated input read once per tile of conv_jt output channels.  Where every element is 1 there are no digits at all.  Every step is an
// exact function on Z_q with canonical residues, so the bits are those of crc_diag_mac_forms per (co, ci) with constant rows, crc_add over ci.
// output channels per thread: CONV_JT_DEFAULT unless the tuning key "conv_jt" says otherwise.  The same exact function at every setting
enum { CONV_JT_DEFAULT = 4, CONV_SLOTS_MAX_CH = 4096, CONV_SLOTS_MAX_T = 1024 };
static int conv_jt(const crc_ctx *c) { return c->tune.conv_jt ? c->tune.conv_jt : (int)CONV_JT_DEFAULT; }
static bool conv_counts_ok(size_t count, int Cin, int Cout, int T)
{
    return Cin >= 1 && Cout >= 1 && T >= 1 && Cin <= CONV_SLOTS_MAX_CH && Cout <= CONV_SLOTS_MAX_CH && T <= CONV_SLOTS_MAX_T && count <= ((size_t)1 << 40);
}
static size_t conv_bytes(const crc_ctx *c, size_t count, int Cin, int Cout, int T, int dbc)
{
    if (!c || !dbc_ok(dbc) || !conv_counts_ok(count, Cin, Cout, T)) return 0;
    WorkArena a;
    hoist_layout(c, (size_t)Cin * count, T, diag_zc(T), dbc, a);
    return a.bytes();
}
extern "C" int crc_conv_slots_pack_weights(const crc_ctx *c, const int64_t *h_w, size_t count, uint64_t *h_out)
{
    if (!c || (count && (!h_w || !h_out))) return CRC_ERR_INVALID_ARGUMENT;
    const int64_t t = (int64_t)c->t;
    for (int i = 0; i < c->k; i++)
        for (size_t j = 0; j < count; j++) {
            const int64_t r = h_w[j] % t;                               // (any int64: the remainder lies in (-t, t))
            const u64 v = (u64)(r < 0 ? r + t : r), qi = c->q[i];
            const u64 low = c->plain.fast ? v : v % qi;                 // plain_lift (kernels.hip) of the constant's one coefficient: every position of its NTT-form row
            h_out[(size_t)i * count + j] = v < c->plain.threshold ? low : c->plain.fast ? v + c->plain.inc[i] : (low + c->plain.inc[i]) % qi;
        }
    return CRC_OK;
}
extern "C" size_t crc_conv_slots_work_bytes(const crc_ctx *c, size_t count, int Cin, int Cout, int T, int dbc) { return conv_bytes(c, count, Cin, Cout, T, dbc); }
// the constant plaintext b mod t in delta form: floor(q / t) c (+ q mod t for the upper half) mod q_i (plain_prep_kernel's mode 2) -- a constant polynomial's
// NTT-form row holds that one word at every position
extern "C" int crc_conv_slots_pack_bias(const crc_ctx *c, const int64_t *h_b, size_t count, uint64_t *h_out)
{
    if (!c || (count && (!h_b || !h_out))) return CRC_ERR_INVALID_ARGUMENT;
    const int64_t t = (int64_t)c->t;
    for (int i = 0; i < c->k; i++)
        for (size_t j = 0; j < count; j++) {
            const int64_t r = h_b[j] % t;
            const u64 v = (u64)(r < 0 ? r + t : r);
            unsigned __int128 z = (unsigned __int128)c->plain.delta[i] * v;
            if (v >= c->plain.threshold) z += c->plain.uhi[i];
            h_out[(size_t)i * count + j] = (u64)(z % c->q[i]);
        }
    return CRC_OK;
}
// crc_conv_slots_forms (d_bias = d_mask_ntt = NULL: galois_conv_mac_kernel<jt, false>, as it always ran) and crc_conv_slots_bias_mask_forms.  With a bias or a
// mask every launch of the channel mix adds mask (.) (its own sum [+ bias on polynomial 0 where it writes the row first]): exact in Z_q, so the bits are those of
// the unmasked call into NTT form, crc_add_plain of the constant's delta row per output channel, crc_multiply_plain_ntt by the mask row, one inverse transform
static int conv_slots_run(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, int Cin, const uint64_t *gs, int T, const uint64_t *d_w, int Cout,
                          const uint64_t *d_bias, const uint64_t *d_mask_ntt, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y,
                          int out_form, void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!conv_counts_ok(count, Cin, Cout, T)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t total = (size_t)Cin * count, outs = (size_t)Cout * count, wb = conv_bytes(c, count, Cin, Cout, T, dbc), ctw = crc_ct_words(c, 2);
    if (!hoist_args_ok(c, d_x, in_form, total, gs, T, d_cgk, elts, n_elts, dbc, d_y, outs, out_form, d_work, wb) ||
        !hoist_operand_ok(c, d_w, 8 * (size_t)c->k * Cout * Cin * T, d_y, outs, d_work, wb)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t bb = 8 * (size_t)c->k * Cout, mb = 8 * (size_t)c->k * c->n, xb = 8 * total * ctw;
    if (d_bias && (!hoist_operand_ok(c, d_bias, bb, d_y, outs, d_work, wb) || ranges_overlap(d_bias, bb, d_x, xb))) return CRC_ERR_INVALID_ARGUMENT;
    if (d_mask_ntt && (!hoist_operand_ok(c, d_mask_ntt, mb, d_y, outs, d_work, wb) || ranges_overlap(d_mask_ntt, mb, d_x, xb))) return CRC_ERR_INVALID_ARGUMENT;
    std::vector<int> at((size_t)T);
    if (!hoist_keys(c, gs, T, elts, n_elts, at.data())) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    const int zc = diag_zc(T);
    WorkArena a(d_work);
    const HoistCall H = hoist_call(c, hoist_layout(c, total, T, zc, dbc, a), d_cgk, dbc, stream, at, T);
    RUN(hoist_prepare_keys(H, 0, T));
    for (size_t o = 0; o < total; o += H.L.step) {
        const size_t ch = pass_len(total, o, H.L.step);
        const u64 *xin = d_x + o * ctw;
        if (H.keyed) RUN(hoist_pass_head(H, xin, in_form, ch));         // (no digits where every element is 1)
        for (int r0 = 0; r0 < T; r0 += zc) {
            const int rn = T - r0 < zc ? T - r0 : zc;
            const u64 *z[GALOIS_DIAG_MAX];
            RUN(hoist_group(H, xin, in_form, ch, o == 0, r0, rn, z));
            RUN(k_galois_conv_mac(c, z, gs + r0, rn, d_w + r0, T, Cin, Cout, o, ch, count, r0 == 0, d_y, conv_jt(c), d_bias, d_mask_ntt, S(stream)));
        }
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, outs, 2, stream));
    return CRC_OK;
}
extern "C" int crc_conv_slots_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, int Cin, const uint64_t *gs, int T, const uint64_t *d_w, int Cout,
                                    const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    return conv_slots_run(c, d_x, in_form, count, Cin, gs, T, d_w, Cout, nullptr, nullptr, d_cgk, elts, n_elts, dbc, d_y, out_form, d_work, stream);
}
extern "C" int crc_conv_slots_bias_mask_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, int Cin, const uint64_t *gs, int T, const uint64_t *d_w,
                                              int Cout, const uint64_t *d_bias, const uint64_t *d_mask_ntt, const uint64_t *d_cgk, const uint64_t *elts, int n_elts,
                                              int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream)
{
    return conv_slots_run(c, d_x, in_form, count, Cin, gs, T, d_w, Cout, d_bias, d_mask_ntt, d_cgk, elts, n_elts, dbc, d_y, out_form, d_work, stream);
}
// ---- prepared keys that outlive a call: what k_relin64_prepare_keys leaves, per conjugated key, in a buffer of the caller's ----
// Every hoisted entry point above prepares the fp64 form of its keys at the start of every call (three launches per key); a layer with hundreds of keys prepares them
// once.  d_pk [n_elts][crc_galois_prepared_key_words], d_scratch: crc_evk_words words
extern "C" size_t crc_galois_prepared_key_words(const crc_ctx *c, int dbc) { return c && dbc_ok(dbc) && k_relin64_supported(c, dbc) ? k_relin64_keys_words(c, dbc) : 0; }
extern "C" int crc_galois_prepare_keys_dev(crc_ctx *c, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_pk, uint64_t *d_scratch,
                                           void *stream)
{
    CHECK_CTX(c);
    if (!dbc_ok(dbc) || n_elts < 0 || (n_elts && (!elts || !d_cgk || !d_pk || !d_scratch)) || !aligned16(d_cgk) || !aligned16(d_pk) || !aligned16(d_scratch))
        return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_elts; e++) if (!crc_galois_elt_valid(c, elts[e]) || elts[e] == 1) return CRC_ERR_INVALID_ARGUMENT;
    if (!k_relin64_supported(c, dbc)) return CRC_ERR_UNSUPPORTED;
    const size_t kw = crc_evk_words(c, dbc), pkw = k_relin64_keys_words(c, dbc);
    if (ranges_overlap(d_cgk, 8 * kw * n_elts, d_pk, 8 * pkw * n_elts) || ranges_overlap(d_cgk, 8 * kw * n_elts, d_scratch, 8 * kw) ||
        ranges_overlap(d_pk, 8 * pkw * n_elts, d_scratch, 8 * kw)) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_elts; e++) RUN(k_relin64_prepare_keys(c, d_cgk + (size_t)e * kw, dbc, d_pk + (size_t)e * pkw, d_scratch, S(stream)));
    return CRC_OK;
}
// ---- the dense layer over channel planes: y = Sum_j H_{gs[j]}( Sum_c P[j][c] (*) x[c] ), x [Cin][count], P [R][Cin][k][n] ----
// The OUTPUTS are rotated, not the inputs: R key switches whatever Cin is.  Per pass of ch ciphertexts per channel: one forward transform of a coefficient-form
// pass; the R inner sums u_j through galois_diag_mac_multi_kernel with every element 1 (GALOIS_DIAG_MAX channels per launch, the accumulate continuation); the
// outer stage -- crc_diag_mac_bsgs_forms' giant stage -- over the keyed steps; galois_sum_permuted_kernel over all R (gs[j] = 1: u_j itself).  The outer stage on
// the fp64 path runs in sub-batches of rb consecutive keyed steps: ONE inverse transform, (c0, 0, c1 (q/q_i)^-1), K1 over rb ch ciphertexts, then K2 with one key
// per step (relin_mac_keyed_f64_kernel) and K3, whose results go over the u_j.  Where the fp64 key switch does not apply, or at planes_batch = 1, it runs step by
// step through hoist_switch_own exactly as the giant stage does.  Every step is an exact function on Z_q with canonical residues: the bits are those
// of crc_multiply_plain_ntt + crc_add over c, crc_rotate_hoisted_forms per j, crc_add over j, at every setting and pass structure.
// Work: [key pointers of the R steps][NTT copy of a coefficient-form pass, Cin ch][the R ch inner sums][coefficient copy of a sub-batch][its size-3 rows][prepared
// keys: R -- with d_pk one, for the path that cannot use d_pk][scratch of the key switch].  A pass keeps (Cin + R) ch ciphertexts, so ch shrinks
// with them as hoist_layout's does; rb ch <= square_chunk, at least one step of one ciphertext
enum { PLANES_BATCH_DEFAULT = 2, DENSE_PLANES_MAX_CH = 4096 };
static int planes_batch(const crc_ctx *c) { return c->tune.planes_batch ? c->tune.planes_batch : (int)PLANES_BATCH_DEFAULT; }
// the HoistWork of the outer stage (xc and x3 of a sub-batch, the R inner sums in u, no z) and around it: kt the key pointers, xh the NTT copy, rb steps per sub-batch
struct PlanesWork : HoistWork { const u64 **kt; u64 *xh; size_t rb; };
static bool planes_counts_ok(size_t count, int Cin, int R)
{
    return Cin >= 1 && Cin <= DENSE_PLANES_MAX_CH && R >= 1 && R <= GALOIS_BSGS_MAX && count <= ((size_t)1 << 40);
}
static PlanesWork planes_layout(const crc_ctx *c, size_t count, int Cin, int R, int dbc, bool prepared, WorkArena &a)
{
    PlanesWork L{};
    const size_t sq = square_chunk(c);
    L.step = sq * HOIST_Z_PASSES / ((size_t)Cin + (size_t)R);
    if (L.step > sq) L.step = sq;
    if (L.step < 1) L.step = 1;
    const size_t ch = count < L.step ? count : L.step;
    L.rb = ch ? sq / ch : sq;                                          // steps per sub-batch of the outer stage: rb ch <= square_chunk
    if (L.rb < 1) L.rb = 1;
    if (L.rb > (size_t)R) L.rb = (size_t)R;
    L.kpw = (k_relin_keys_words(c, dbc) + 31) & ~(size_t)31;
    L.kt = a.take<const u64 *>((size_t)R);
    L.xh = a.take<u64>((size_t)Cin * ch * crc_ct_words(c, 2));
    L.u = a.take<u64>((size_t)R * ch * crc_ct_words(c, 2));
    L.xc = a.take<u64>(L.rb * ch * crc_ct_words(c, 2));
    L.x3 = a.take<u64>(L.rb * ch * crc_ct_words(c, 3));
    L.kp = a.take<u64>((prepared ? 1 : (size_t)R) * L.kpw);
    const size_t one = k_relin_work_words(c, ch, dbc), all = k_relin64_supported(c, dbc) ? k_relin64_work_words(c, L.rb * ch, dbc) : 0;
    L.rest = a.take<u64>(one > all ? one : all);                        // (either setting of planes_batch, either key-switch path: as hoist_layout's)
    return L;
}
static size_t planes_bytes(const crc_ctx *c, size_t count, int Cin, int R, int dbc, bool prepared)
{
    if (!c || !dbc_ok(dbc) || !planes_counts_ok(count, Cin, R)) return 0;
    WorkArena a;
    planes_layout(c, count, Cin, R, dbc, prepared, a);
    return a.bytes();
}
extern "C" size_t crc_dense_planes_work_bytes(const crc_ctx *c, size_t count, int Cin, int R, int dbc, int prepared)
{
    return planes_bytes(c, count, Cin, R, dbc, prepared != 0);
}
extern "C" int crc_dense_planes_forms(crc_ctx *c, const uint64_t *d_x, int in_form, size_t count, int Cin, const uint64_t *gs, int R, const uint64_t *d_p_ntt,
                                      const uint64_t *d_cgk, const uint64_t *elts, int n_elts, const uint64_t *d_pk, int dbc, uint64_t *d_y, int out_form,
                                      void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (!planes_counts_ok(count, Cin, R) || !aligned16(d_pk)) return CRC_ERR_INVALID_ARGUMENT;
    const bool prepared = d_pk != nullptr;
    const size_t total = (size_t)Cin * count, wb = planes_bytes(c, count, Cin, R, dbc, prepared), ctw = crc_ct_words(c, 2), rowp = (size_t)c->k * c->n;
    const size_t xb = 8 * total * ctw, yb = 8 * count * ctw, pb = 8 * (size_t)R * Cin * rowp;
    if (!hoist_args_ok(c, d_x, in_form, total, gs, R, d_cgk, elts, n_elts, dbc, d_y, count, out_form, d_work, wb) ||
        !hoist_operand_ok(c, d_p_ntt, pb, d_y, count, d_work, wb)) return CRC_ERR_INVALID_ARGUMENT;
    if (ranges_overlap(d_p_ntt, pb, d_x, xb)) return CRC_ERR_INVALID_ARGUMENT;      // (two buffers that are only read: refused because the header says so)
    std::vector<int> at((size_t)R);
    if (!hoist_keys(c, gs, R, elts, n_elts, at.data())) return CRC_ERR_INVALID_ARGUMENT;       // (a keyed step with n_elts = 0 ends here, d_pk or not)
    const size_t pkw = k_relin64_keys_words(c, dbc), pkb = 8 * pkw * (size_t)n_elts;
    if (prepared && (ranges_overlap(d_pk, pkb, d_x, xb) || ranges_overlap(d_pk, pkb, d_y, yb) || ranges_overlap(d_pk, pkb, d_p_ntt, pb) ||
                     ranges_overlap(d_pk, pkb, d_work, wb))) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    WorkArena a(d_work);
    const PlanesWork L = planes_layout(c, count, Cin, R, dbc, prepared, a);
    HoistCall H = hoist_call(c, L, d_cgk, dbc, stream, at, R);
    const bool batched = H.f64 && planes_batch(c) == 2, use_pk = H.f64 && prepared;
    if (use_pk) { H.L.kp = const_cast<u64 *>(d_pk); H.L.kpw = pkw; }   // (d_pk is only read: the fp64 path never prepares into it)
    // the prepared key of step j is at kp + slot(j) kpw
    auto slot = [&](int j) { return use_pk ? at[j] : H.f64 || !prepared ? j : 0; };    // (!f64 with d_pk: the one slot, prepared again by every step)
    if (batched && H.keyed) {
        std::vector<int> slots((size_t)R, -1);                          // the pointer table is written on the device: the slots go as kernel arguments
        for (int j = 0; j < R; j++) if (at[j] >= 0) slots[j] = slot(j);
        RUN(k_relin64_key_table(H.L.kp, H.L.kpw, slots.data(), (size_t)R, L.kt, S(stream)));
    }
    if (!use_pk) RUN(hoist_prepare_keys(H, 0, R));
    std::vector<const u64 *> zs((size_t)R), zin((size_t)Cin);
    const std::vector<u64> ones(GALOIS_DIAG_MAX, 1);
    for (size_t o = 0; o < count; o += L.step) {
        const size_t ch = pass_len(count, o, L.step), uj = ch * ctw;
        for (int ci = 0; ci < Cin; ci++) zin[ci] = d_x + ((size_t)ci * count + o) * ctw;
        if (in_form == CRC_COEFF) {                                     // one shared forward transform where the pass is contiguous, one per channel otherwise
            if (ch == count) RUN(k_ntt_ct(c, false, d_x, L.xh, total, 2, false, S(stream), nullptr, 0, 0, 0));
            else for (int ci = 0; ci < Cin; ci++) RUN(k_ntt_ct(c, false, zin[ci], L.xh + (size_t)ci * uj, ch, 2, false, S(stream), nullptr, 0, 0, 0));
            for (int ci = 0; ci < Cin; ci++) zin[ci] = L.xh + (size_t)ci * uj;
        }
        for (int c0 = 0; c0 < Cin; c0 += GALOIS_DIAG_MAX) {
            const int cn = Cin - c0 < GALOIS_DIAG_MAX ? Cin - c0 : (int)GALOIS_DIAG_MAX;
            RUN(k_galois_diag_mac_multi(c, zin.data() + c0, ones.data(), c0, cn, Cin, d_p_ntt, R, ch, c0 != 0, L.u, S(stream)));
        }
        for (int j0 = 0; j0 < R;) {
            if (at[j0] < 0) { j0++; continue; }
            int j1 = j0 + 1;                                            // a run of consecutive keyed steps, at most rb of them where they go as one batch
            while (batched && j1 < R && at[j1] >= 0 && (size_t)(j1 - j0) < L.rb) j1++;
            u64 *ub = L.u + (size_t)j0 * uj;
            if (batched) {
                const size_t cnt = (size_t)(j1 - j0) * ch;
                RUN(k_ntt_ct(c, true, ub, L.xc, cnt, 2, false, S(stream), nullptr, 0, 0, 0));
                RUN(k_galois_permute(c, L.xc, cnt, 1, false, L.x3, S(stream)));
                RUN(k_relin64_digits(c, L.x3, 3, 2, cnt, dbc, L.rest, S(stream)));
                RUN(k_relin64_from_digits_keyed(c, L.x3, 3, cnt, ch, dbc, ub, L.rest, L.kt + j0, S(stream), true));
            }
            else RUN(hoist_switch_own(H, ub, ch, j0, slot(j0), prepared || o == 0));
            j0 = j1;
        }
        for (int j = 0; j < R; j++) zs[j] = L.u + (size_t)j * uj;
        RUN(k_galois_sum_permuted(c, zs.data(), gs, R, ch, false, d_y + o * ctw, S(stream)));
    }
    if (out_form == CRC_COEFF) RUN(crc_ntt_inv(c, d_y, count, 2, stream));
    return CRC_OK;
}
extern "C" int crc_square_relin(crc_ctx *c, const uint64_t *d_x, size_t count, const uint64_t *d_evk, int dbc, uint64_t *d_y, void *d_work, void *stream)
{
    return crc_square_relin_forms(c, d_x, CRC_COEFF, count, d_evk, dbc, d_y, CRC_COEFF, d_work, stream);
}

// ---- modulus switching: a ciphertext tensor of `from` continues over the first k' moduli (kernels_modswitch.hip) ----
static bool mod_switch_args_ok(const crc_ctx *from, const crc_ctx *to, int size, int in_form, int out_form)
{
    return k_mod_switch_supported(from, to) && (size == 2 || size == 3) && form_ok(in_form) && form_ok(out_form);
}
extern "C" int crc_mod_switch_supported(const crc_ctx *from, const crc_ctx *to) { return k_mod_switch_supported(from, to) ? 1 : 0; }
extern "C" size_t crc_mod_switch_work_bytes(const crc_ctx *from, const crc_ctx *to, size_t count, int size, int in_form, int out_form)
{
    return mod_switch_args_ok(from, to, size, in_form, out_form) ? k_mod_switch_work_bytes(from, to, count * size, in_form, out_form) : 0;
}
extern "C" int crc_mod_switch_forms(crc_ctx *from, const crc_ctx *to, const uint64_t *d_in, int in_form, size_t count, int size, uint64_t *d_out, int out_form,
                                    void *d_work, void *stream)
{
    CHECK_CTX(from);
    if (!d_in || !d_out || !d_work || !mod_switch_args_ok(from, to, size, in_form, out_form)) return CRC_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t in_b = 8 * count * crc_ct_words(from, size), out_b = 8 * count * crc_ct_words(to, size);
    const size_t wb = k_mod_switch_work_bytes(from, to, count * size, in_form, out_form);
    if (ranges_overlap(d_in, in_b, d_out, out_b) || ranges_overlap(d_work, wb, d_in, in_b) || ranges_overlap(d_work, wb, d_out, out_b)) return CRC_ERR_INVALID_ARGUMENT;
    return k_mod_switch(from, to, d_in, in_form, count * size, d_out, out_form, d_work, S(stream));
}
extern "C" int crc_mod_switch(const crc_ctx *from, const crc_ctx *to, const uint64_t *h_in, int in_form, size_t count, int size, uint64_t *h_out, int out_form)
{
    if (!h_in || !h_out || !mod_switch_args_ok(from, to, size, in_form, out_form)) return CRC_ERR_INVALID_ARGUMENT;
    if (ranges_overlap(h_in, 8 * count * crc_ct_words(from, size), h_out, 8 * count * crc_ct_words(to, size))) return CRC_ERR_INVALID_ARGUMENT;
    return k_mod_switch_host(from, to, h_in, in_form, count * size, h_out, out_form);
}

// ---- noise flooding: a fresh encryption of zero with a wide uniform error joins every ciphertext of a response (kernels_flood.hip) ----
extern "C" int crc_flood_supported(const crc_ctx *c, int flood_bits) { return k_flood_supported(c, flood_bits) ? 1 : 0; }
extern "C" int crc_flood_bits(const crc_ctx *c, int budget_bits_in, int lambda_bits) { return k_flood_bits(c, budget_bits_in, lambda_bits); }
extern "C" int crc_flood_budget_bound(const crc_ctx *c, int budget_bits_in, int flood_bits) { return k_flood_budget_bound(c, budget_bits_in, flood_bits); }
extern "C" size_t crc_flood_dev_work_bytes(const crc_ctx *c, size_t count, int form) { return c && form_ok(form) ? k_flood_work_bytes(c, count) : 0; }
static int flood_dev(crc_ctx *c, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, const ChaChaKey &key, uint64_t stream_base,
                     void *d_work, void *stream)
{
    CHECK_CTX(c);
    if (count == 0) return CRC_OK;
    if (!d_pk || !d_ct || !d_work || !k_flood_supported(c, flood_bits)) return CRC_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_pk & 15) || ((uintptr_t)d_ct & 15)) return CRC_ERR_INVALID_ARGUMENT;
    if (!form_ok(form)) return CRC_ERR_UNSUPPORTED;
    const size_t ct_b = 8 * count * crc_ct_words(c, 2), pk_b = 8 * crc_ct_words(c, 2), wb = k_flood_work_bytes(c, count);
    if (ranges_overlap(d_pk, pk_b, d_ct, ct_b) || ranges_overlap(d_work, wb, d_ct, ct_b) || ranges_overlap(d_work, wb, d_pk, pk_b)) return CRC_ERR_INVALID_ARGUMENT;
    return k_flood(c, d_pk, d_ct, count, form == CRC_NTT, flood_bits, key, stream_base, d_work, S(stream));
}
extern "C" int crc_flood_dev_key(crc_ctx *c, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, const uint8_t *h_key,
                                 uint64_t stream_base, void *d_work, void *stream)
{
    if (!h_key) return CRC_ERR_INVALID_ARGUMENT;
    return flood_dev(c, d_pk, d_ct, count, form, flood_bits, chacha_load_key(h_key), stream_base, d_work, stream);
}
extern "C" int crc_flood_dev(crc_ctx *c, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, uint64_t seed, void *d_work, void *stream)
{
    return flood_dev(c, d_pk, d_ct, count, form, flood_bits, chacha_seed_key(seed), 0, d_work, stream);
}
static int flood_host(const crc_ctx *c, const uint64_t *h_pk, uint64_t *h_ct, size_t count, int form, int flood_bits, const ChaChaKey &key, uint64_t stream_base)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    if (count == 0) return CRC_OK;
    if (!h_pk || !h_ct || !k_flood_supported(c, flood_bits)) return CRC_ERR_INVALID_ARGUMENT;
    if (!form_ok(form)) return CRC_ERR_UNSUPPORTED;
    if (ranges_overlap(h_pk, 8 * crc_ct_words(c, 2), h_ct, 8 * count * crc_ct_words(c, 2))) return CRC_ERR_INVALID_ARGUMENT;
    return k_flood_host(c, h_pk, h_ct, count, form == CRC_NTT, flood_bits, key, stream_base);
}
extern "C" int crc_flood_key(const crc_ctx *c, const uint64_t *h_pk, uint64_t *h_ct, size_t count, int form, int flood_bits, const uint8_t *h_key,
                             uint64_t stream_base)
{
    if (!h_key) return CRC_ERR_INVALID_ARGUMENT;
    return flood_host(c, h_pk, h_ct, count, form, flood_bits, chacha_load_key(h_key), stream_base);
}
extern "C" int crc_flood(const crc_ctx *c, const uint64_t *h_pk, uint64_t *h_ct, size_t count, int form, int flood_bits, uint64_t seed)
{
    return flood_host(c, h_pk, h_ct, count, form, flood_bits, chacha_seed_key(seed), 0);
}
