// kernels.h -- launchers implemented in kernels.hip / kernels_square.hip (internal; the public surface is crcnn_hip.h)
#pragma once
#include "ctx.h"
#include "window.h"
#include "xcd_grid.h"

int k_ntt_ct(crc_ctx *c, bool inv, const u64 *src, u64 *dst, size_t count, int size, bool bsk, hipStream_t st,
             const u64 *addend, int add_sign, size_t add_group, int add_mod = 0, int pack_out = 0);
bool k_ntt_ct_box_supported(const crc_ctx *c, int bxf, int byf);     // the boxed forward transform (nttbox.h): this ring, these moduli, this many terms
int k_ntt_ct_box(crc_ctx *c, const u64 *src, u64 *dst, int B, int xd, int yd, int bxf, int byf, int xs, int ys, hipStream_t st);
int k_ntt_ct_fwd_mul(crc_ctx *c, u64 *ct, size_t count, const u64 *w, size_t group, hipStream_t st);
int k_ntt_ct_fwd_fma(crc_ctx *c, u64 *ct, size_t count, const u64 *u, const u64 *key, hipStream_t st);
int k_ntt_ct_fwd_negmul(crc_ctx *c, u64 *ct, size_t count, const u64 *sk, hipStream_t st);
int k_ntt_ct_poly0(crc_ctx *c, const u64 *src, u64 *dst, size_t count, hipStream_t st);
int k_ntt_ct_addct(crc_ctx *c, const u64 *src, u64 *dst, size_t count, const u64 *addct, int add_size, hipStream_t st);
int k_ntt_ct_head_add(crc_ctx *c, const u64 *src, int src_size, u64 *dst, size_t count, const u64 *addrows, hipStream_t st);
int k_spread_ntt(crc_ctx *c, const u64 *src, size_t items, u64 *dst, hipStream_t st);
int k_digit_ntt(crc_ctx *c, const u64 *src, int src_size, int src_poly, size_t count, int D, const unsigned char *dig_i, const unsigned char *dig_shift, int dbc,
                u64 *dst, hipStream_t st, int pack_out = 0);
int k_product_intt(crc_ctx *c, const u64 *x, const u64 *y, u64 *dst, size_t count, bool bsk, hipStream_t st, const u64 *opt_mul = nullptr, bool *applied = nullptr);     // y null: the square of x
int k_ntt_ct_inv_scaled(crc_ctx *c, const u64 *src, u64 *dst, size_t count, int size, const u64 *mul, const u64 *mul_s, hipStream_t st);
int k_plain_ntt(crc_ctx *c, const u64 *d_plain, size_t count, int mode, bool do_ntt, u64 *d_out, hipStream_t st);
int k_plain_expand(crc_ctx *c, const u64 *d_compact, size_t count, u64 *d_plain, hipStream_t st);
int k_rowwise(crc_ctx *c, u64 *acc, const u64 *b, size_t count, int size, int op, int sign, size_t group, size_t gmod, hipStream_t st);
int k_pool(crc_ctx *c, const u64 *x, u64 *y, int B, int zd, const Window &w, const u64 *mul, hipStream_t st, int pack_out = 0);
int k_pad(crc_ctx *c, const u64 *x, u64 *y, int B, int zd, int xd, int yd, int px0, int px1, int py0, int py1, hipStream_t st);
int k_bn_ntt(crc_ctx *c, u64 *x, int B, int zd, int hw, const u64 *mean, const u64 *invstd, hipStream_t st);
int k_mac(crc_ctx *c, const u64 *x, const u64 *w, u64 *y, const int *d_xoff, const int *d_toff, int B, int P, int F, int T, int in_cts,
          const u64 *bias_ntt, hipStream_t st, int xp = 0, int wp = 0, int yp = 0);
int k_pack28(crc_ctx *c, u64 *rows, size_t nrows, bool unpack, hipStream_t st);
int k_conv_offsets(crc_ctx *c, int *xoff, int *toff, unsigned *toffw, const LayerShape &s, hipStream_t st);
// The work space of a ciphertext product (the square: one input, the multiply: two) whose auxiliary base has `rows` rows per polynomial: per input its NTT form
// over q and its lifted rows (all QN before all LB: the lifted rows of both inputs are one array), then the three product polynomials in both bases.  Filled
// on the caller's work space it gives the pointers, on a null base it only counts (work_arena.h's idea in plain word offsets: no rounding)
struct ProductWork {
    u64 *QN[2], *LB[2], *DQ, *DB;         // QN[h] [cnt][2][k][n] | LB[h] [cnt][2][rows][n] | DQ [cnt][3][k][n] | DB [cnt][3][rows][n]
    size_t words;
};
static inline ProductWork product_work(const crc_ctx *c, size_t cnt, int inputs, size_t rows, u64 *work = nullptr)
{
    ProductWork w{};
    const size_t n = c->n, k = c->k;
    auto take = [&](size_t words) { u64 *p = work ? work + w.words : nullptr; w.words += words; return p; };
    for (int h = 0; h < inputs; h++) w.QN[h] = take(cnt * 2 * k * n);
    for (int h = 0; h < inputs; h++) w.LB[h] = take(cnt * 2 * rows * n);
    w.DQ = take(cnt * 3 * k * n);
    w.DB = take(cnt * 3 * rows * n);
    return w;
}
size_t k_square_work_words(const crc_ctx *c, size_t cnt);            // product_work counted with the rows of the larger auxiliary base (61-bit or fp64)
size_t k_multiply_work_words(const crc_ctx *c, size_t cnt);          // the product of two ciphertexts: four input polynomials per pair
size_t k_relin_work_words(const crc_ctx *c, size_t cnt, int dbc);
size_t k_relin_keys_words(const crc_ctx *c, int dbc);
// kernels_relin64.hip: key switching over the two fp64 primes
bool   k_relin64_supported(const crc_ctx *c, int dbc);
size_t k_relin64_keys_words(const crc_ctx *c, int dbc);
size_t k_relin64_work_words(const crc_ctx *c, size_t cnt, int dbc);
int k_relin64_prepare_keys(crc_ctx *c, const u64 *evk, int dbc, u64 *kp, u64 *scratch, hipStream_t st);
// a window of the sum pooling that follows a Square layer: the key switch is linear in the digit polynomials, so the digits of a window's c2's are summed before
// they are transformed and ONE key switch serves the pooled ciphertext (kernels_relin64.hip; PoolGeom: window.h)
bool k_relin64_pool_supported(const crc_ctx *c, int dbc, int window);
// the ring-linear terms of a degree-2 polynomial activation, joined to an NTT-form result while it leaves the key switch's last kernel:
// y = mul (*) y + p1 (*) Sum_w xh_w (+ p0 on poly 0); xh: the activation's NTT-form input (size-2 ciphertexts where x3 holds the size-3 squares)
struct PolyTail { const u64 *xh, *p1, *p0; };
bool k_relin64_poly_fused(const crc_ctx *c);           // tune.poly_tail = 0 and a transform radix whose last kernel has room for the tail
int k_relinearize64(crc_ctx *c, const u64 *src, int src_size, int src_poly, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y, u64 *work, const u64 *kp,
                    hipStream_t st, bool out_ntt, const PoolGeom *pool = nullptr, const u64 *mul = nullptr, const PolyTail *poly = nullptr);
// its two halves: the digit transforms into E at the front of `work` (K1), then inner products, lift and tail from an E that is there (K2 + K3)
int k_relin64_digits(crc_ctx *c, const u64 *src, int src_size, int src_poly, size_t cnt, int dbc, u64 *work, hipStream_t st, const PoolGeom *pool = nullptr);
int k_relin64_from_digits(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y, u64 *work, const u64 *kp, hipStream_t st, bool out_ntt,
                          const PoolGeom *pool = nullptr, const u64 *mul = nullptr, const PolyTail *poly = nullptr);
// K2 + K3 of two prepared keys on one E, the digit values read once for both (work: k_relin64_work_words_multi(.., 2)): the bits of two k_relin64_from_digits
size_t k_relin64_work_words_multi(const crc_ctx *c, size_t cnt, int dbc, int keys);
int k_relin64_from_digits2(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, int dbc, u64 *y0, u64 *y1, u64 *work, const u64 *kp0, const u64 *kp1,
                           hipStream_t st, bool out_ntt);
// K2 + K3 with one prepared key per step of the batch (relin_mac_keyed_f64_kernel): cnt = steps x per_key ciphertexts, those of step j under kp_table[j] -- a DEVICE
// array of pointers to prepared keys; E over all cnt is there; work: k_relin64_work_words(cnt).  The bits of k_relin64_from_digits per step
int k_relin64_from_digits_keyed(crc_ctx *c, const u64 *x3, int add_size, size_t cnt, size_t per_key, int dbc, u64 *y, u64 *work, const u64 *const *kp_table,
                                hipStream_t st, bool out_ntt);
// its kp_table, written by a kernel: table[j] = base + slots[j] kpw (words), null where slots[j] < 0; `slots` is a host array, consumed before the call returns
int k_relin64_key_table(const u64 *base, size_t kpw, const int *slots, size_t steps, const u64 **table, hipStream_t st);
// the same terms in a kernel of their own (kernels.hip: poly2_tail_kernel), in place on y [planes][xo][yo]
int k_poly2_tail(crc_ctx *c, u64 *y, const u64 *xh, size_t planes, const Window &w, const u64 *p2, const u64 *p1, const u64 *p0, hipStream_t st);
int k_square(crc_ctx *c, const u64 *x, size_t cnt, u64 *y3, u64 *work, hipStream_t st, bool in_ntt = false, bool premul_c2 = false);
// kernels_square64.hip: the square's auxiliary base over the engine's fp64 primes
bool k_square64_supported(const crc_ctx *c);
int k_square64(crc_ctx *c, const u64 *x, size_t cnt, u64 *y3, u64 *work, hipStream_t st, bool in_ntt, bool premul_c2);
// Evaluator::multiply of size-2 ciphertexts x[i] . y[i] -> size-3 y3[i] (x == y allowed: the square); forms and premul_c2 as k_square
int k_multiply(crc_ctx *c, const u64 *x, const u64 *y, size_t cnt, u64 *y3, u64 *work, hipStream_t st, bool in_ntt = false, bool premul_c2 = false);
int k_multiply64(crc_ctx *c, const u64 *x, const u64 *y, size_t cnt, u64 *y3, u64 *work, hipStream_t st, bool in_ntt, bool premul_c2);
int k_relinearize(crc_ctx *c, const u64 *x3, size_t cnt, const u64 *evk, int dbc, u64 *y, u64 *work, u64 *kp, hipStream_t st, bool out_ntt = false,
                  bool c2_premul = false, bool keys_ready = false, const u64 *p2 = nullptr, const struct PolyTail *poly = nullptr, bool *poly_fused = nullptr);
// kernels_galois.hip: sigma_g of size-2 coefficient-form ciphertexts as the size-3 rows k_relinearize(..., c2_premul = true) takes: (sigma(c0) [+ c0], 0 [c1],
// sigma(c1) (q/q_i)^-1); g a valid Galois element, x and x3 disjoint and 16-byte aligned
int k_galois_permute(crc_ctx *c, const u64 *x, size_t cnt, u64 g, bool accumulate, u64 *x3, hipStream_t st);
// sigma_g on NTT-form rows [rows][n] (any modulus: a gather by index alone), out = NTT(sigma_g(INTT(in))); in and out disjoint and 16-byte aligned
int k_galois_permute_ntt(crc_ctx *c, const u64 *in, size_t rows, u64 g, u64 *out, hipStream_t st);
// y [cnt][2][k][n] (+)= Sum_r p[r] (*) sigma_{g[r]}(z[r]) on NTT-form ciphertexts z[r] [cnt][2][k][n] and plaintext rows p[r] [k][n]; R <= GALOIS_DIAG_MAX
enum { GALOIS_DIAG_MAX = 32 };
int k_galois_diag_mac(crc_ctx *c, const u64 *const *z, const u64 *const *p, const u64 *g, int R, size_t cnt, bool accumulate, u64 *y, hipStream_t st);
// baby-step / giant-step: u [G][cnt][2][k][n] (+)= Sum_{r < R} P[j][b0 + r] (*) sigma_{g[r]}(z[r]) for every j < G, P [G][B][k][n]; GALOIS_MULTI_JT giant indices share one
// gather of the z[r] (galois_diag_mac_multi_kernel); R <= GALOIS_DIAG_MAX, G <= GALOIS_BSGS_MAX
enum { GALOIS_MULTI_JT = 4, GALOIS_BSGS_MAX = 1 << 16 };
int k_galois_diag_mac_multi(crc_ctx *c, const u64 *const *z, const u64 *g, int b0, int R, int B, const u64 *p, int G, size_t cnt, bool accumulate, u64 *u,
                            hipStream_t st);
// the packed convolution's channel mix (galois_conv_mac_kernel<jt>): y [Cout][count] (+)= Sum_ci Sum_{r < R} w[.][co][ci][r] sigma_{g[r]}(z[r][ci count + ct - o]) over the
// flat ciphertexts [o, o + ch) of x [Cin][count] that the pass holds; w = &W[0][0][0][r0] of the scalar weights W [k][Cout][Cin][T], first: r0 = 0 (rows whose channel 0
// lies in the pass are written, every other row accumulated into); R <= GALOIS_DIAG_MAX, jt in {2, 4, 8}.  bias [k][Cout] / mask [k][n] (either may be null): each
// launch adds mask (.) (its own sum [+ bias on polynomial 0 where it writes the row first]) -- galois_conv_mac_kernel<jt, true>; both null: <jt, false>
int k_galois_conv_mac(crc_ctx *c, const u64 *const *z, const u64 *g, int R, const u64 *w, int T, int Cin, int Cout, size_t o, size_t ch, size_t count, bool first,
                      u64 *y, int jt, const u64 *bias, const u64 *mask, hipStream_t st);
// y [cnt][2][k][n] (+)= Sum_r sigma_{g[r]}(z[r]) on NTT-form ciphertexts, any R (GALOIS_DIAG_MAX per launch); y disjoint from every z[r]
int k_galois_sum_permuted(crc_ctx *c, const u64 *const *z, const u64 *g, int R, size_t cnt, bool accumulate, u64 *y, hipStream_t st);
int k_mac2(crc_ctx *c, const u64 *x, const u64 *w, u64 *y, const int *d_xoff, const int *d_toff, int B, const LayerShape &s, const u64 *bias_ntt,
           const unsigned *d_toffw, hipStream_t st, int xp = 0, int wp = 0, int yp = 0);
int k_fold_pool(crc_ctx *c, const u64 *w, const u64 *bias, const u64 *div, u64 *wout, u64 *bout, int nf, int zd, int xf, int yf, int cxs, int cys,
                int pxf, int pyf, hipStream_t st, bool hoisted = false);
size_t k_encrypt_work_words(const crc_ctx *c, size_t cnt);
struct ChaChaKey;
int k_encrypt(crc_ctx *c, const u64 *pk, const u64 *plain, size_t cnt, const ChaChaKey &key, u64 stream_base, u64 *ct, u64 *work, hipStream_t st, bool out_ntt = false,
              bool plain_compact = false);
void k_encrypt_cdt(u64 *out19);                 // the 19 thresholds of the device encryptor's noise magnitudes (tests)
// encryption under the secret key (sk: [k][n], NTT form); plain: dense rows or compact plaintexts, either result form
size_t k_encrypt_sym_work_words(const crc_ctx *c, size_t cnt);
int k_encrypt_sym(crc_ctx *c, const u64 *sk, const u64 *plain, size_t cnt, const ChaChaKey &key, u64 stream_base, u64 *ct, u64 *work, hipStream_t st, bool out_ntt,
                  bool plain_compact);
// seeded secret-key ciphertexts: c0 [cnt][k][n] packed NTT-form rows -> ct [cnt][2][k][n], c1 = A(seed, stream_base + m) regenerated (chacha.h)
int k_seeded_expand(crc_ctx *c, const u64 *c0, size_t cnt, const ChaChaKey &seed, u64 stream_base, u64 *ct, hipStream_t st, bool out_ntt);
// the seeded form produced on the device: c0 [cnt][k][n] = NTT(e + Delta m) - A(seed) . s, formed in place (no work buffer, no c1 row); the host twin is
// crc_encrypt_sym_seeded_key (client.cpp)
int k_encrypt_sym_seeded(crc_ctx *c, const u64 *sk, const u64 *plain, size_t cnt, const ChaChaKey &key, const ChaChaKey &seed, u64 stream_base, u64 *c0,
                         hipStream_t st, bool plain_compact);
// kernels_decrypt.hip: Decryptor::decrypt and the fractional encoder on the device (the refresh of Network::forward)
size_t k_decrypt_work_words(const crc_ctx *c, size_t cnt, int size, bool in_ntt);
int k_decrypt(crc_ctx *c, const u64 *sk, const u64 *ct, size_t cnt, int size, bool in_ntt, u64 *plain, u64 *work, hipStream_t st);
int k_decrypt_recode(crc_ctx *c, const u64 *sk, const u64 *ct, size_t cnt, bool in_ntt, u64 *compact, float *vals_out, u64 *work, hipStream_t st);
int k_fra_decode(crc_ctx *c, const u64 *plain, size_t cnt, double *out, hipStream_t st);
int k_fra_encode(crc_ctx *c, const void *src, int mode, size_t cnt, u64 *plain, float *vals_out, hipStream_t st);
int k_fra_encode_compact(crc_ctx *c, const float *src, size_t cnt, u64 *compact, hipStream_t st);      // floats -> compact plaintexts [cnt][96]
// V = work [cnt][k][n]: c0 + c1 s (+ c2 s^2) in coefficient form (work: k_decrypt_work_words)
int k_decrypt_rows(crc_ctx *c, const u64 *sk, const u64 *ct, size_t cnt, int size, bool in_ntt, u64 *work, hipStream_t st);
// kernels_budget.hip: Decryptor::invariant_noise_budget of every ciphertext of a tensor (work: k_decrypt_work_words)
int k_noise_budget(crc_ctx *c, const u64 *sk, const u64 *ct, size_t cnt, int size, bool in_ntt, int32_t *bits, int32_t *min_out, u64 *work, hipStream_t st);
int k_budget_bits_host(const crc_ctx *c, const u64 *h_v, size_t cnt, int32_t *h_bits);

// kernels_slots.hip: slot batching -- values (item c, slot i) at values[c item_stride + i slot_stride] <-> plaintexts [count][n]; *_host: the host twins
int k_slots_compose(crc_ctx *c, const long long *d_values, size_t count, int slots, size_t item_stride, size_t slot_stride, u64 *d_plain, hipStream_t st);
int k_slots_decompose(crc_ctx *c, const u64 *d_plain, size_t count, int slots, long long *d_values, size_t item_stride, size_t slot_stride, hipStream_t st);
int k_slots_compose_host(crc_ctx *c, const long long *values, size_t count, int slots, size_t item_stride, size_t slot_stride, u64 *plain);
int k_slots_decompose_host(crc_ctx *c, const u64 *plain, size_t count, int slots, long long *values, size_t item_stride, size_t slot_stride);
// every slot of a plaintext -> floor(slot / divisor + 1/2), 1 <= divisor <= 2^62 (the caller checks); in == out allowed
int k_slots_rescale(crc_ctx *c, const u64 *d_in, size_t count, u64 divisor, u64 *d_out, hipStream_t st);
int k_slots_rescale_host(crc_ctx *c, const u64 *plain_in, size_t count, u64 divisor, u64 *plain_out);
// client-side activation of plaintext rows [planes][w.xd][w.yd][n] -> [planes][w.xo()][w.yo()][n]: window maximum, division, ReLU, cap, slot by slot
int k_slots_act(crc_ctx *c, const u64 *d_in, size_t planes, const Window &w, u64 divisor, int relu, u64 cap, u64 *d_out, hipStream_t st);
int k_slots_act_host(crc_ctx *c, const u64 *plain_in, size_t planes, const Window &w, u64 divisor, int relu, u64 cap, u64 *plain_out);
// several plain moduli: r <= CRC_SLOTS_CRT_MAX contexts of one n with pairwise distinct slot primes t_j, T = t_0 ... t_{r-1} < 2^63.  P[j] = t_0 ... t_{j-1},
// Pinv[j] = P[j]^-1 mod t_j with its Shoup companion (Garner's mixed-radix constants).  k_slots_crt_base: false where the t_j are no such base
struct SlotsCrtBase { int r; u64 t[CRC_SLOTS_CRT_MAX], P[CRC_SLOTS_CRT_MAX], Pinv[CRC_SLOTS_CRT_MAX], Pinv_s[CRC_SLOTS_CRT_MAX], T; };
bool k_slots_crt_base(crc_ctx *const *ctxs, int r, SlotsCrtBase *B);
// row tensors plain[j] [count][n] mod t_j -> the centred integers mod T of the first `slots` slots, strided as k_slots_decompose's values
int k_slots_crt_decompose(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *d_plain, size_t count, int slots, long long *d_values, size_t item_stride,
                          size_t slot_stride, hipStream_t st);
int k_slots_crt_decompose_host(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *plain, size_t count, int slots, long long *values, size_t item_stride,
                               size_t slot_stride);
// every slot's integer V mod T -> min(max(floor(V / divisor + 1/2), 0 if relu), cap if cap), reduced mod every t_j again; out[j] == in[j] allowed
int k_slots_crt_act(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *d_in, size_t count, u64 divisor, int relu, u64 cap, u64 *const *d_out, hipStream_t st);
int k_slots_crt_act_host(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *plain_in, size_t count, u64 divisor, int relu, u64 cap, u64 *const *plain_out);

// kernels_seeded_keys.hip: seeded key-switching keys (chacha.h CHACHA_DOM_KSK_*; ids is a HOST array of key ids: 0 = evaluation key, else a Galois element).
// first / rows [n_ids][P][k][n] NTT form, formed in place without work space; out [n_ids][crc_evk_words]; the host twins are crc_gen_keys_seeded_key and
// crc_seeded_keys_expand (client.cpp)
bool k_seeded_keys_grid_ok(const crc_ctx *c, int dbc, int n_ids);
int k_gen_keys_seeded(crc_ctx *c, const u64 *sk, int dbc, const u64 *ids, int n_ids, const ChaChaKey &key, const ChaChaKey &seed, u64 *first, hipStream_t st);
int k_seeded_keys_expand(crc_ctx *c, const u64 *rows, const u64 *ids, int n_ids, int dbc, const ChaChaKey &seed, bool conjugate, u64 *out, hipStream_t st);
// keys of `from` for `to`, a level of it (ctx.h keys_level_of): expanded blobs restricted -- [n_keys][crc_evk_words(from)] -> [n_keys][crc_evk_words(to)] --, and
// from's seeded rows expanded straight into to's blobs (= the restriction of k_seeded_keys_expand).  Launched on from's device; host twins: crc_keys_restrict,
// crc_seeded_keys_expand_level (client.cpp)
int k_keys_restrict(crc_ctx *from, const crc_ctx *to, const u64 *keys, int n_keys, int dbc, u64 *out, hipStream_t st);
int k_seeded_keys_expand_level(crc_ctx *from, const crc_ctx *to, const u64 *rows, const u64 *ids, int n_ids, int dbc, const ChaChaKey &seed, bool conjugate, u64 *out,
                               hipStream_t st);
// kernels_modswitch.hip: modulus switching from `from` to a context over a proper prefix of its moduli -- tensors of `polys` polynomials [polys][k][n] -> [polys][k'][n],
// either side CRC_COEFF or CRC_NTT (work: k_mod_switch_work_bytes); *_host: the host twin
bool   k_mod_switch_supported(const crc_ctx *from, const crc_ctx *to);
size_t k_mod_switch_work_bytes(const crc_ctx *from, const crc_ctx *to, size_t polys, int in_form, int out_form);
int k_mod_switch(crc_ctx *from, const crc_ctx *to, const u64 *d_in, int in_form, size_t polys, u64 *d_out, int out_form, void *d_work, hipStream_t st);
int k_mod_switch_host(const crc_ctx *from, const crc_ctx *to, const u64 *in, int in_form, size_t polys, u64 *out, int out_form);
// kernels_flood.hip: noise flooding of size-2 ciphertext tensors [cnt][2][k][n], in place, CRC_NTT (ntt_form) or CRC_COEFF; B = flood_bits (k_flood_supported);
// the pure arithmetic of crc_flood_bits / crc_flood_budget_bound (a negative status for what they refuse); *_host: the host twin
bool   k_flood_supported(const crc_ctx *c, int B);
int    k_flood_bits(const crc_ctx *c, int budget_in, int lambda);
int    k_flood_budget_bound(const crc_ctx *c, int budget_in, int B);
size_t k_flood_work_bytes(const crc_ctx *c, size_t cnt);
int k_flood(crc_ctx *c, const u64 *d_pk, u64 *d_ct, size_t cnt, bool ntt_form, int B, const ChaChaKey &key, u64 stream_base, void *d_work, hipStream_t st);
int k_flood_host(const crc_ctx *c, const u64 *pk, u64 *ct, size_t cnt, bool ntt_form, int B, const ChaChaKey &key, u64 stream_base);

// kernels_mfma.hip: conv / dense multiply-accumulate as an int8 limb GEMM on the matrix cores (operand form CRC_NTTL)
bool   k_limb_supported(const crc_ctx *c, int T);
size_t k_limb_tensor_bytes(const crc_ctx *c, int B, int zd, int npos);
size_t k_limb_weights_bytes(const crc_ctx *c, int nf, int zd, int xf, int yf);
int    k_limb_flat_zdc(int zd);                        // channel bytes per position of the flat form (layers of fewer than 32 channels), 0: blocked form
int    k_limb_steps(int zd, int xf, int yf);           // 32-term reduction steps of a layer
size_t k_limb_result_words(const crc_ctx *c, int B, int nf, int P);
int k_limb_pack_tensor(crc_ctx *c, const u64 *x, signed char *xl, int B, int zd, int npos, bool packed, hipStream_t st, int Btot = 0, int b0 = 0, bool scalar = false);
int k_limb_pack_weights(crc_ctx *c, const u64 *w, signed char *wl, int nf, int zd, int xf, int yf, hipStream_t st, int f0 = 0, int ft = -1);
int k_limb_result_to_rows(crc_ctx *c, const u64 *ys, u64 *y, size_t rows, bool pack_out, hipStream_t st);
int k_limb_result_to_limb(crc_ctx *c, const u64 *ys, signed char *xl, int B, int zd, hipStream_t st, bool scalar = false);
bool k_limb_direct_dense(int P);
int k_limb_mac(crc_ctx *c, const signed char *xl, const signed char *wl, u64 *ys, signed char *xl_out, const u64 *bias_ntt, int B, const LayerShape &s, hipStream_t st,
               bool scalar = false);
// scalar form (CRC_NTTLS): the weights of a slot-batched network are constant polynomials, one residue per modulus; the n GEMMs of a modulus run as one
size_t k_scalar_weights_bytes(const crc_ctx *c, int nf, int zd, int xf, int yf);
bool   k_scalar_supported(const crc_ctx *c, int B, const LayerShape &s);
int k_scalar_pack_weights(crc_ctx *c, const u64 *w, size_t wstride, signed char *wl, int nf, int zd, int xf, int yf, int *constant, hipStream_t st);
// kernels_mfma1.hip: one-channel convolutions (conv1 [+ pool1]) on the matrix cores (weight form CRC_NTTL1)
bool   k_limb_conv1_shape(const crc_ctx *c, const LayerShape &s);
int    k_limb_conv1_form(const crc_ctx *c, int xf, int yf, int nf);          // 1 plane-major, 2 pixel-major image and limb-folded weights
size_t k_limb_conv1_weights_bytes(const crc_ctx *c);                         // enough for either form
size_t k_limb_conv1_weights_bytes_for(const crc_ctx *c, int nf, int xf, int yf);
size_t k_limb_conv1_image_bytes(const crc_ctx *c, int B, const Window &w, int nf);
int k_limb_conv1_pack_weights(crc_ctx *c, const u64 *w, signed char *wl, int nf, int xf, int yf, hipStream_t st);
// a bxf x byf box (window sum of the input at the layer's stride, made by the image pack) in front of the layer with base window xf x yf; in: the window on the
// INPUT image -- the kernel reads in.boxed(bxf, byf)
int k_limb_conv1(crc_ctx *c, const u64 *x, bool packed, signed char *xr, const signed char *wl, u64 *ys, signed char *xl_out, int Bout, int b0, const u64 *bias_ntt, int B,
                 const Window &in, int nf, hipStream_t st, int bxf = 1, int byf = 1);
bool   k_limb_conv1_box_shape(const crc_ctx *c, const LayerShape &s, int bxf, int byf);
