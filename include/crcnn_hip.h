/*
 * crcnn_hip.h -- C ABI of the MI355X-native encrypted-CNN evaluation engine (libcrcnn_hip.so).
 *
 * Drop-in boundary for the reference's hot path.  The reference (CrCNN) has no FFI layer: its
 * evaluation path is `Layer::forward(ciphertext3D)` (CrCNN/src/layer.h:10-31) calling ten SEAL 2.3.1 `Evaluator`
 * methods (SEAL/seal/evaluator.cpp).  Each entry point below names the reference function(s) it replaces.  The C++
 * classes in crcnn_amd/host/ (Layer, ConvolutionalLayer, ..., Network, CnnBuilder) mirror the reference's interface
 * one-to-one and are implemented purely on top of this header.
 *
 * Conventions
 *   - plain C types only; every pointer named d_* is a DEVICE pointer (HBM), h_* is a host pointer.
 *   - a ciphertext of `size` polynomials is uint64[size][k][n], residues canonical in [0,q_i)  (SEAL keeps
 *     [size][k][n+1] with a dead zero pad word, ciphertext.cpp:103-130: crc_import/export_seal convert).
 *   - a ciphertext tensor is [B][C][H][W] of ciphertexts, row-major (CrCNN's ciphertext3D is [z][x][y]; B = image batch).
 *   - plaintext polynomials are uint64[n] coefficient vectors in [0,t); "ntt form" weights are uint64[k][n];
 *     "delta form" plaintexts (pre-scaled for add_plain/sub_plain) are uint64[k][n].
 *   - `form` flags say whether a ciphertext tensor is in coefficient form (CRC_COEFF, what the reference's layers
 *     exchange) or in NTT form (CRC_NTT, SEAL's transform_to_ntt ordering: slot j holds a(psi^(2*bitrev(j)+1))).
 *   - all functions return 0 on success or a negative crc_status; nothing throws across the ABI.  The reference
 *     signals errors by C++ exceptions (std::invalid_argument, evaluator.cpp:1549-1556) -- the C++ host classes turn a
 *     non-zero status back into std::invalid_argument / std::runtime_error.
 *   - a context is immutable after creation (crc_ctx_set_tuning excepted: tools and tests only, on a context nobody is launching on) and may be used
 *     from several host threads at once, provided every concurrent call has its own stream and its own `d_work`: every launch goes to the HIP
 *     stream passed in (`stream` is a hipStream_t cast to void*, NULL = default stream), no entry point keeps state between calls, and the one
 *     piece of context scratch (crc_checksum64's accumulators) is handed out per call (tests/test_gpu_threads.py: two host threads, two streams,
 *     a convolution on one and square + relinearise on the other, both against the reference's goldens).  No entry point allocates, frees or
 *     synchronises unless its name says so; scratch memory is passed in (`d_work`, sized by *_work_bytes).  The C++ host classes
 *     (crcnn_amd/host/crcnn_host.h) are NOT thread-safe: like the reference they keep the context, the keys and a work buffer in globals
 *     (CrCNN/src/globals.h:18-26) and launch on the default stream.
 *   - host-side calls that work item by item (crc_encode_f32 / _f64 / _compact, crc_encrypt / crc_encrypt_key) spread their items over up to CRC_HOST_THREADS
 *     std::threads (default: the hardware's, at most 16) drawn from one budget per process, so callers that are themselves pool threads do not multiply
 *     thread counts; results do not depend on the split (one keystream per ciphertext, one weight per plaintext)
 */
#ifndef CRCNN_HIP_H
#define CRCNN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crc_ctx crc_ctx;

typedef enum {
    CRC_OK = 0,
    CRC_ERR_INVALID_ARGUMENT = -1,   /* bad shape / null pointer / unsupported parameter (std::invalid_argument in the reference) */
    CRC_ERR_PARAMETERS = -2,         /* (n, q[], t) rejected: SEALContext::validate, context.cpp:15-169 */
    CRC_ERR_HIP = -3,                /* a HIP runtime call failed; crc_last_hip_error() has the code */
    CRC_ERR_UNSUPPORTED = -4,        /* valid in the reference but not implemented here (e.g. more than 48 relinearisation digits) */
    CRC_ERR_IO = -5,                 /* file could not be read / not an HDF5 file we understand */
    CRC_ERR_NOT_FOUND = -6,          /* dataset name missing in the model file */
    CRC_ERR_COMM = -7                /* an RCCL call failed; crc_last_comm_error() has the ncclResult_t */
} crc_status;

enum { CRC_COEFF = 0, CRC_NTT = 1,
       /* NTT form with every residue stored as its two 28-bit limbs (lo | hi << 32): the operand form of the multiply-accumulate
        * kernels (no 64x64 multiplier on gfx950; 3 v_mad_u64_u32 per product on 28-bit limbs).  Only crc_conv2d_forms /
        * crc_dense_forms take or produce it (weights and the tensors that travel between conv / dense layers); crc_pack28 converts.
        * Needs coefficient moduli below 2^56. */
       CRC_NTTP = 2,
       /* "limb form": the operand form of the matrix-core multiply-accumulate (kernels_mfma.hip).  Every residue as the seven balanced base-256 digits of
        * its centred representative (int8), SLOT-MAJOR: tensors [k][n][B][7][positions][2 polys][channels rounded up to 32] (a dense layer's input, one
        * position, is
        * K-blocked instead: [k][n][7][channels / 32][B * 2 rows = (image, poly)][32]), weights
        * [k][n][tap][channel block][7][filters rounded up to 64][32] (times 2^64 mod q: the kernel's Montgomery reduction divides it out).  Exact integer
        * arithmetic on v_mfma_i32_16x16x64_i8 (49 limb products per modular
        * multiply, int32 accumulators, one reduction per output): the same ciphertexts as every other form, about 4x the throughput of the vector-ALU
        * kernel on long reductions.  crc_limb_pack_weights makes the weights; crc_conv2d_forms / crc_dense_forms take w_form = CRC_NTTL, convert a
        * CRC_COEFF / CRC_NTT / CRC_NTTP input themselves and produce any form (out_form = CRC_NTTL hands the tensor to a DENSE layer: channels =
        * (filter, x, y) flattened, 1 x 1 positions).  Needs coefficient moduli below 2^55 (at most 55 significant bits: |centred residue| < 2^54 fits seven
        * balanced
        * bytes) and reductions of at most 18 000 terms; crc_limb_supported answers for a context and shape. */
       CRC_NTTL = 3,
       /* weights of a ONE-CHANNEL convolution (CrCNN's conv1, alone or fused with its pooling layer: window <= 8 x 8, <= 32 filters) for the matrix-core
        * kernel specialised for it (kernels_mfma1.hip): [k][n][2][7][32 filters][32 window taps], tap = 8 kx + ky.  w_form only (crc_limb_conv1_*). */
       CRC_NTTL1 = 4,
       /* out_form only, with w_form = CRC_NTTL1: the result as the limb tensor a CONVOLUTION reads with in_form = CRC_NTTL
        * ([k][n][B][7][xo*yo][2][32 channels]; CRC_NTTL as out_form flattens for a dense consumer instead) */
       CRC_NTTLC = 5,
       /* "scalar limb form": CRC_NTTL for a slot-batched network (crc_slots_*: n images per ciphertext), whose weights are constant polynomials -- one residue
        * per modulus, the same at all n slots.  The n per-slot GEMMs of a modulus share their weights and run as ONE GEMM over the n B images e = s B + b.
        *   weights (w_form)       [k][step][7][Fp][32] int8, CRC_NTTL's container for a one-slot ring: crc_scalar_pack_weights, crc_limb_weights_bytes / n bytes
        *   convolution tensors    byte-identical to CRC_NTTL ([slot][B] images ARE [modulus][n B] images): pass in_form = CRC_NTTL
        *   dense input / output   [k][7][zdp / 32][(e, poly)][32]: in_form / out_form = CRC_NTTLS (differs from CRC_NTTL's per-slot K-blocking)
        * crc_conv2d_forms / crc_dense_forms take w_form = CRC_NTTLS with any in_form / out_form of CRC_NTTL besides; biases stay ordinary NTT rows.
        * crc_scalar_supported answers for a context and shape. */
       CRC_NTTLS = 6 };

const char *crc_strerror(int status);
int         crc_last_hip_error(void);
int         crc_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * context   replaces: SEALContext (context.cpp:15-169) + Evaluator ctor tables (evaluator.cpp:19-121) + BaseConverter
 *           ctor (util/baseconverter.cpp:20-353) + SmallNTTTables (util/smallntt.cpp:37-92) as built by
 *           CrCNN setParameters (CrCNN/src/globals.cpp:25-56).  q may be any explicit list (coeff_modulus_128(n) or a
 *           prefix of it, as BASELINE.json's configs ask).
 * ------------------------------------------------------------------------------------------------------------- */
int  crc_ctx_create(int n, const uint64_t *q, int k, uint64_t t, int device, crc_ctx **out);
void crc_ctx_destroy(crc_ctx *ctx);
/* SEAL's default 128-bit-security moduli (util/globals.cpp:25-90); returns count, copies min(count,cap) */
int  crc_default_coeff_modulus_128(int n, uint64_t *q, int cap);
int  crc_ctx_n(const crc_ctx *ctx);
int  crc_ctx_k(const crc_ctx *ctx);
int  crc_ctx_kbsk(const crc_ctx *ctx);                 /* |Bsk| */
int  crc_ctx_device(const crc_ctx *ctx);
size_t crc_ct_words(const crc_ctx *ctx, int size);     /* size*k*n */
size_t crc_evk_words(const crc_ctx *ctx, int dbc);     /* words of an evaluation-key blob: sum_l 2*L_l*k*n (0 for a dbc outside 1..60: every call that
                                                          takes a dbc refuses those with CRC_ERR_INVALID_ARGUMENT, every size query gives 0) */
/* named host-side table read-out (tests): "root","const_ratio","delta","upper_half_increment","bsk","bsk_root",
 * "root_powers:<i>","inv_root_powers_div_two:<i>", "slots_root", "slots_index_map" (slot batching, below), "f64_primes" (the two fp64 primes of relinearisation's key switching), "sq64_primes" (the fp64 primes that
 * carry the square's auxiliary base: B' = all but the last, m_sk' = the last; empty when the parameters do not fit twelve of them), "key_q" (the moduli of the
 * key-switching gadget: q, or an ancestor's list on a level of crc_ctx_create_level), "inv_qhat" ((q/q_i)^-1 mod q_i) and "ksk_inv_qhat" ((Q_key/q_i)^-1 mod
 * q_i: what a polynomial is multiplied by before a key switch cuts its digits; equal to "inv_qhat" except on such a level); returns word count */
int  crc_ctx_table(const crc_ctx *ctx, const char *name, uint64_t *h_out, int cap);
/* Tuning switches of tools/ and the tests (none is needed for normal use).  The engine reads its environment (CRC_MFMA_VARIANT, CRC_CONV1_PASS_BYTES, ...)
 * exactly
 * once, inside crc_ctx_create; this call changes one switch of a context nobody is launching on: "mfma_variant", "mfma_order", "mfma_ring", "conv1_waves",
 * "conv1_narrow" (0: a one-channel convolution with 17-20 filters runs its second filter group like a full one), "conv1_pass_bytes", "conv1_box" (crc_plan_conv1_box), "box_ntt" (CRC_BOX_NTT; a boxed one-channel layer on coefficient-form input sums the window in front of its input transform, crc_ntt_fwd_box: 0 off, 1 the default block order, 2 the other order), "hoist_pool" (crc_plan_hoist_pool), "limb_pack_group", "mac2_cfg", "mac_order", "mac_regstage", "ntt_inv61_loose", "ntt_split", "mfma_min_steps", "scalar_mac" (crc_plan_mac_scalar), "f64_radix",
 * "relin_mac_ct", "poly_tail" (crc_poly2_relin_forms),
 * "relin_path" (1: key switching over the coefficient moduli, as the reference does it, instead of over two fp64 primes), "sq_path" (1: the square's auxiliary
 * base is SEAL's 61-bit
 * one instead of the engine's fp64 primes; 2: force the latter), "sq_chunk" (ciphertexts per internal pass of square + relinearise; changes
 * crc_square_relin_work_bytes),
 * "sq_fuse" (1: an NTT-resident square lifts to its auxiliary base inside the forward transforms, 0: in a kernel of its own, -1: by the number of moduli),
 * "f64_wave" (bit mask of the fp64 row kernels that run with one workgroup barrier per transform at n = 8192 / 16384: 1 sq64_inv, 2 the digit kernel, 4 K3, 8
 * the lifting
 * forward kernel, 16 K3's 64-bit forward transform; -1: the measured choice, 0: the round-4 kernels), "ntt_wave" (the same for the 64-bit row transforms: 1 n =
 * 8192, 2 n = 4096, 4 n = 16384, 8 n = 16384 with the square's prologues, 16 inverse butterflies that halve at every stage as in round 4 instead of scaling once
 * at the end; -1: the measured choice = 15).
 * Every path gives the same ciphertexts.  CRC_ERR_NOT_FOUND for anything else. */
int  crc_ctx_set_tuning(crc_ctx *ctx, const char *name, long long value);

/* thin device-memory helpers so that C / C++ / ctypes callers need not link HIP themselves */
int crc_mem_info(crc_ctx *ctx, size_t *free_bytes, size_t *total_bytes);      /* hipMemGetInfo of the context's device */
int crc_malloc(crc_ctx *ctx, size_t bytes, void **d_ptr);
int crc_free(crc_ctx *ctx, void *d_ptr);
int crc_memcpy_h2d(crc_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, void *stream);
int crc_memcpy_d2h(crc_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, void *stream);
int crc_memcpy_d2d(crc_ctx *ctx, void *d_dst, const void *d_src, size_t bytes, void *stream);
int crc_memset(crc_ctx *ctx, void *d_dst, int value, size_t bytes, void *stream);
int crc_stream_sync(crc_ctx *ctx, void *stream);
/* Streams of the caller's own (hipStream_t behind void*, created non-blocking: no implicit ordering against the default stream) and page-locked host memory:
 * what a host needs to upload the next chunk of encrypted images while the current one is evaluated -- the reference's driver encrypts, evaluates and decrypts
 * one image after the other (CrCNN/src/mainparams.cpp:85-112).  crc_stream_wait_event makes `stream` wait for an event recorded on another one. */
int crc_stream_create(crc_ctx *ctx, void **stream);
int crc_stream_destroy(crc_ctx *ctx, void *stream);
int crc_stream_wait_event(crc_ctx *ctx, void *stream, void *event);
int crc_host_alloc(crc_ctx *ctx, size_t bytes, void **h_ptr);
int crc_host_free(crc_ctx *ctx, void *h_ptr);
/* threads the host-side item loops of this process use (the reference's th_count fan-out, convolutionalLayer.cpp:177-191, has no process-wide cap):
 * CRC_HOST_THREADS,
 * else the hardware's, at most 16, divided by the ranks that share the node (LOCAL_WORLD_SIZE / CRC_LOCAL_WORLD) */
int crc_host_thread_limit(void);
/* HIP events (hipEvent_t behind void*): record on the stream the kernels go to, read the time between two of them (waits for the second) */
int crc_event_create(crc_ctx *ctx, void **event);
int crc_event_destroy(crc_ctx *ctx, void *event);
int crc_event_record(crc_ctx *ctx, void *event, void *stream);
int crc_event_elapsed_ms(crc_ctx *ctx, void *event_start, void *event_end, float *ms);

/* ---------------------------------------------------------------------------------------------------------------
 * encoding (host)   replaces: FractionalEncoder(t, x^n+1, 64, 32, 3)::encode/decode (encoder.cpp:1013-1076,
 *           1226-1270; instantiated at CrCNN/src/globals.cpp:52) as used by CnnBuilder::build*Layer (cnnBuilder.cpp:25-105)
 * ------------------------------------------------------------------------------------------------------------- */
/* values are widened float32 -> double exactly as `fraencoder->encode(weights[w])` does.  h_coeff_count (optional)
 * receives SEAL's Plaintext::coeff_count() for each value (needed only for wire-format compatibility). */
int    crc_encode_f32(const crc_ctx *ctx, const float *h_values, size_t count, uint64_t *h_plain /*[count][n]*/, int32_t *h_coeff_count);
int    crc_encode_f64(const crc_ctx *ctx, const double *h_values, size_t count, uint64_t *h_plain, int32_t *h_coeff_count);
double crc_decode(const crc_ctx *ctx, const uint64_t *h_plain /*[n]*/);
/* the same plaintexts in COMPACT form: the encoder only ever sets coefficients 0..63 (integer part: at most ceil(64 / log2 3) + 1 = 42 digits) and n-32..n-1
 * (fraction), so a weight travels as CRC_PLAIN_COMPACT_WORDS words -- words 0..63 = coefficients 0..63, words 64..95 = coefficients n-32..n-1 -- and
 * crc_plain_expand (below) zero-extends it on the device.  PlainModelWoPad's fc3 at n = 16384: 0.3 GB over PCIe instead of 52 GB. */
#define CRC_PLAIN_COMPACT_LOW   64
#define CRC_PLAIN_COMPACT_HIGH  32
#define CRC_PLAIN_COMPACT_WORDS 96
int    crc_encode_f32_compact(const crc_ctx *ctx, const float *h_values, size_t count, uint64_t *h_compact /*[count][96]*/, int32_t *h_coeff_count);
/* batch-norm parameters: invstd = float(1/sqrt(double(var)+0.00001))  (cnnBuilder.cpp:100-102) */
int    crc_bn_invstd_f32(const float *h_var, size_t count, float *h_invstd);

/* ---------------------------------------------------------------------------------------------------------------
 * plaintext preparation (device)
 *   crc_plain_to_ntt     replaces Evaluator::transform_to_ntt(Plaintext&) (evaluator.cpp:1418-1493): lift to each q_i
 *                        (c >= (t+1)/2 ? c + q_i - t : c) and forward NTT.     d_plain [count][n] -> d_out [count][k][n]
 *   crc_plain_to_delta   the Delta*m term of add_plain/sub_plain (evaluator.cpp:1168-1191): floor(q/t)*c (+ q mod t for
 *                        "negative" c) mod q_i.  form=CRC_NTT additionally NTTs it (for NTT-resident tensors).
 * ------------------------------------------------------------------------------------------------------------- */
int crc_plain_to_ntt(crc_ctx *ctx, const uint64_t *d_plain, size_t count, uint64_t *d_out, void *stream);
/* compact plaintexts on the device (crc_encode_f32_compact, copied down as they are) -> dense [count][n] for the two calls around this one */
int crc_plain_expand(crc_ctx *ctx, const uint64_t *d_compact /*[count][96]*/, size_t count, uint64_t *d_plain /*[count][n]*/, void *stream);
int crc_plain_to_delta(crc_ctx *ctx, const uint64_t *d_plain, size_t count, int form, uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * NTT   replaces Evaluator::transform_to_ntt(Ciphertext&) / transform_from_ntt (evaluator.cpp:1495-1539) ->
 *       ntt_negacyclic_harvey / inverse_ntt_negacyclic_harvey (util/smallntt.h:210-258, smallntt.cpp:195-375).
 *       In place on `count` ciphertexts of `size` polys each; canonical output.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_ntt_fwd(crc_ctx *ctx, uint64_t *d_ct, size_t count, int size, void *stream);
int crc_ntt_inv(crc_ctx *ctx, uint64_t *d_ct, size_t count, int size, void *stream);
/* The forward transform of window sums, out of place (d_src != d_dst): d_src = B images of xd x yd coefficient-form size-2 ciphertexts with canonical residues,
 * d_dst = B images of xdo x ydo = (xd - (bxf-1) xs) x (yd - (byf-1) ys) NTT-form ones, pixel (r, c) = NTT(sum over a < bxf, b < byf of src(r + a xs, c + b ys)
 * mod q) -- bit for bit the sum mod q of the terms' crc_ntt_fwd.  The sum is taken while the transform loads its row.  CRC_ERR_UNSUPPORTED for rings other than
 * 2048 / 4096 / 8192 / 16384, moduli outside 45..57 bits, the ring's bit of "ntt_wave" off, and boxes of more than 9 terms. */
int crc_ntt_fwd_box(crc_ctx *ctx, const uint64_t *d_src, uint64_t *d_dst, int B, int xd, int yd, int bxf, int byf, int xs, int ys, void *stream);
/* same over the Bsk moduli (rows are [count][kbsk][n]); exposed for unit tests of the Square pipeline */
int crc_ntt_fwd_bsk(crc_ctx *ctx, uint64_t *d_rows, size_t count, void *stream);
int crc_ntt_inv_bsk(crc_ctx *ctx, uint64_t *d_rows, size_t count, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * element-wise Evaluator ops on `count` size-2 ciphertexts
 *   crc_add              Evaluator::add (evaluator.cpp:254-294)                      d_acc += d_b
 *   crc_add_plain        Evaluator::add_plain / sub_plain (:1145-1241) with a pre-scaled delta-form plaintext
 *                        shared by `group` consecutive ciphertexts (d_delta [count/group][k][n]); sign=+1/-1
 *   crc_multiply_plain_ntt  Evaluator::multiply_plain_ntt (:1541-1585): NTT-form ct times NTT-form plaintext
 *   crc_multiply_plain   Evaluator::multiply_plain generic path (:1343-1415): coefficient-form ct in, coefficient-form
 *                        out, NTT-form plaintext given (the reference re-NTTs it on every call)
 * ------------------------------------------------------------------------------------------------------------- */
int crc_add(crc_ctx *ctx, uint64_t *d_acc, const uint64_t *d_b, size_t count, int size, void *stream);
int crc_add_plain(crc_ctx *ctx, uint64_t *d_ct, const uint64_t *d_delta, size_t count, size_t group, int sign, void *stream);
int crc_multiply_plain_ntt(crc_ctx *ctx, uint64_t *d_ct, const uint64_t *d_w_ntt, size_t count, size_t group, int size, void *stream);
int crc_multiply_plain(crc_ctx *ctx, uint64_t *d_ct, const uint64_t *d_w_ntt, size_t count, size_t group, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * layers (batched over B images).  in_form / out_form: CRC_COEFF reproduces the reference layer exactly (coefficient
 * form in and out); CRC_NTT keeps tensors NTT-resident between layers (bit-identical after the final INTT).
 *
 *   crc_conv2d   ConvolutionalLayer::forward / convolution3d (CrCNN/src/convolutionalLayer.cpp:159-197, 56-93):
 *                y[b][f][i][j] = sum_{z,kx,ky} x[b][z][i*xs+kx][j*ys+ky] (*) w[f][z][kx][ky] + Delta*bias[f],
 *                valid padding, xo=(xd-xf)/xs+1, yo=(yd-yf)/ys+1.   d_w_ntt [nf][zd][xf][yf][k][n],
 *                d_bias_delta [nf][k][n] in the form of the OUTPUT (coeff for CRC_COEFF, NTT for CRC_NTT).
 *   crc_dense    FullyConnectedLayer::forward (fullyConnectedLayer.cpp:113-168) incl. reshapeInput (:38-56):
 *                x is [B][in_dim] cts in z,x,y row-major order; d_w_ntt [out_dim][in_dim][k][n].
 *   crc_pool     PoolingLayer::forward (poolingLayer.cpp:22-44) and AvgPoolingLayer::forward (avgPoolingLayer.cpp:16-45):
 *                window sum; if d_div_ntt != NULL multiply by that NTT-form plaintext (encode(1./(xf*yf))).
 *                form = CRC_NTTP: NTT-form input, output in the packed operand form (hand-over to a conv / dense layer).
 *   crc_batchnorm BatchNormLayer::forward (batchNormLayer.cpp:29-40): (x - Delta*mean[z]) (*) invstd[z].
 *                d_mean_delta [C][k][n] in the form of the INPUT, d_invstd_ntt [C][k][n].
 *   crc_square_relin  SquareLayer::forward (squareLayer.cpp:22-74) = Evaluator::square (evaluator.cpp:702-884) +
 *                relinearize (:886-1069) with decomposition-bit-count `dbc` keys.  Coefficient form in and out.
 *                d_evk: for l<k: [2*L_l][k][n] (= evaluation_keys.data()[0][l], pad words dropped), values may be
 *                SEAL's lazy non-canonical residues.  The result is the reference's ciphertext bit for bit; HOW it is computed differs where
 *                BFV leaves the evaluator a choice of moduli: BEHZ's auxiliary base (baseconverter.cpp:47-56 takes 61-bit primes) and the key-switching
 *                inner products (evaluator.cpp:997-1030 transforms every digit under every q_j) run over 47-bit primes of the engine's own in exact fp64
 *                arithmetic; crc_ctx_set_tuning "sq_path" / "relin_path" = 1 select kernels that follow the reference step by step.
 * ------------------------------------------------------------------------------------------------------------- */
size_t crc_conv2d_work_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int in_form);
int crc_conv2d(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_w_ntt, const uint64_t *d_bias_delta,
               int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf,
               int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream);
/* Algebraic fusion of a convolution with the sum/average pooling that follows it (ConvolutionalLayer + PoolingLayer /
 * AvgPoolingLayer, convolutionalLayer.cpp:159-197 + poolingLayer.cpp:22-44 / avgPoolingLayer.cpp:16-45): both are linear over Z_q,
 * so pool(conv_w(x) + b) = conv_w'(x) + b' exactly, with w'[f][z][u][v] = div * sum_{a,b} w[f][z][u-a*cxs][v-b*cys], b' = div*pxf*pyf*b.
 * Produces the pooled kernel [nf][zd][xf'][yf'][k][n] (xf' = (pxf-1)*cxs + xf) and bias [nf][k][n], all in NTT form; run it with
 * crc_conv2d(..., xs = cxs*pxs, ys = cys*pys, xf', yf', out_form = CRC_NTT).  The final network output is bit-identical; only the
 * (unobservable in NTT-resident mode) intermediate tensor disappears.  d_div_ntt = NULL for sum pooling. */
int crc_conv2d_fold_pool(crc_ctx *ctx, const uint64_t *d_w_ntt, const uint64_t *d_bias_delta_ntt, const uint64_t *d_div_ntt, int nf, int zd, int xf, int yf,
                         int cxs, int cys, int pxf, int pyf, uint64_t *d_w_out, uint64_t *d_bias_out, void *stream);
/* The other way round for a stride-1 convolution whose input comes from another convolution (crc_plan_hoist_pool): the pool's window sum is HOISTED in front of
 * the convolution, pool(conv_w(x) + b) = conv_w'(S) + b' with S[u][v] = sum_{a<pxf, b<pyf} x[u+a][v+b], w' = div * w (the window stays xf x yf), b' = div*pxf*pyf*b.
 * S is the layer in front with a (pxf x pyf, stride 1) sum pool folded into ITS weights (crc_conv2d_fold_pool, d_div_ntt = NULL); this entry produces w' [nf][zd][xf][yf][k][n]
 * and b' [nf][k][n]; run them with crc_conv2d(..., xd - pxf + 1, yd - pyf + 1, xs = pxs, ys = pys, xf, yf).  Exact mod q: the same ciphertexts as the folded pair. */
int crc_conv2d_hoist_pool(crc_ctx *ctx, const uint64_t *d_w_ntt, const uint64_t *d_bias_delta_ntt, const uint64_t *d_div_ntt, int nf, int zd, int xf, int yf,
                          int pxf, int pyf, uint64_t *d_w_out, uint64_t *d_bias_out, void *stream);
/* the same two layers with the packed operand form: in_form / out_form may also be CRC_NTTP, w_form says how d_w_ntt is stored
 * (CRC_NTT canonical, CRC_NTTP packed by crc_pack28).  Same ciphertexts; nothing is re-split inside the kernels. */
int crc_conv2d_forms(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_w_ntt, int w_form, const uint64_t *d_bias_delta,
                     int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf,
                     int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream);
int crc_dense_forms(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_w_ntt, int w_form, const uint64_t *d_bias_delta,
                    int B, int in_dim, int out_dim, int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream);
/* limb form (CRC_NTTL): sizes, weight conversion (from CRC_NTT canonical weights; d_wl: crc_limb_weights_bytes), and the work space of
 * crc_conv2d_forms / crc_dense_forms when w_form = CRC_NTTL (crc_conv2d_work_bytes covers the other weight forms) */
int    crc_limb_supported(const crc_ctx *ctx, int zd, int xf, int yf);
size_t crc_limb_tensor_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd);
size_t crc_limb_weights_bytes(const crc_ctx *ctx, int nf, int zd, int xf, int yf);
int    crc_limb_pack_weights(crc_ctx *ctx, const uint64_t *d_w_ntt, int nf, int zd, int xf, int yf, void *d_wl, void *stream);
/* the same a filter tile at a time: d_w_tile_ntt holds filters f0 .. f0 + ft of the layer's nf ([ft][zd][xf][yf][k][n]); the tiles must be packed in order from
 * f0 = 0 (that call zeroes the padding of d_wl).  A layer whose canonical NTT-form weights and limb copy do not fit in HBM together (PlainModelWoPad's fc3 at
 * n = 16384: 202 + 177 GiB) is built this way straight from its plaintexts: encode -> crc_plain_to_ntt -> (batch-norm fold) -> tile, the canonical tile being
 * scratch */
int    crc_limb_pack_weights_tile(crc_ctx *ctx, const uint64_t *d_w_tile_ntt, int nf, int f0, int ft, int zd, int xf, int yf, void *d_wl, void *stream);
/* Kernel selection -- the ONE statement of the policy, asked by every host (crcnn_amd/netrun.py and the C++ classes of crcnn_amd/host):
 *   crc_plan_mac        the weight form (= kernel) of a conv / dense layer launched on B images (B <= 0: do not apply the rows-per-launch guard):
 *                       CRC_NTTL1 one-channel convolution on the matrix cores, CRC_NTTL limb GEMM (>= 8 reduction steps of 32 channels and >= 32 rows = images
 *                       x
 *                       2 polys x output pixels per launch), CRC_NTTP the vector-ALU kernel on 28-bit limb pairs, CRC_NTT canonical (moduli above 55 bits).
 *                       A dense layer is the 1 x 1 convolution zd = in_dim, nf = out_dim.  matrix_cores = 0 keeps everything on the vector ALU.
 *   crc_plan_fold_pool  whether folding a pooling layer into the convolution in front of it (crc_conv2d_fold_pool) pays, by the cost model of DESIGN.md section
 *   4
 *   crc_plan_hoist_pool whether the pool behind a stride-1 convolution is hoisted in front of it instead (crc_conv2d_hoist_pool): u... is the geometry of the layer in
 *                       front AS IT RUNS (already folded), a resident convolution -- uzd = 0 where there is no such layer (nothing in front, another kind of layer, a
 *                       refresh in between, streamed or tile-wise weights).  No unless the convolution has stride 1, the pool decimates and crc_plan_fold_pool folds
 *                       it, the layer in front takes the enlarged window on the kernel family it runs on, and the pair costs less that way on B images per launch
 *                       (same units; the one-channel kernel's two forms are priced at the K they pay for).  Tuning key hoist_pool = 0 / CRC_HOIST_POOL=0: always no */
int    crc_plan_mac(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int B, int matrix_cores, int *w_form);
/* Scalar form (CRC_NTTLS), for networks under slot batching:
 *   crc_scalar_weights_bytes   size of the packed weights (crc_limb_weights_bytes / n)
 *   crc_scalar_supported       pure host query, 0 / 1: can crc_conv2d_forms run the layer with w_form = CRC_NTTLS on B images per slot?  The limb form's limits (moduli
 *                              of at most 55 bits, at most 18 000 terms, at most 8 moduli) and the kernel's 32-bit offsets: a modulus' limb tensor and its result of n B
 *                              images each below 4 GiB.  Where it says 0 the forms call returns CRC_ERR_UNSUPPORTED and launches nothing
 *   crc_scalar_pack_weights    d_w: canonical NTT-form weight rows [nf][zd][xf][yf][k][n] (w_stride = n) or one residue per modulus [nf][zd][xf][yf][k] (w_stride = 1)
 *                              -> d_ws.  Synchronises once (a start-up path).  A row whose n words are not all equal is no constant polynomial: *constant = 0 and
 *                              CRC_ERR_INVALID_ARGUMENT, d_ws is not written; *constant = 1 in every other case, refusals of the arguments included
 *   crc_plan_mac_scalar        crc_plan_mac for a layer of a slot-batched network: CRC_NTTLS where crc_scalar_supported and zd >= 2, else crc_plan_mac's answer
 *                              with the matrix cores on (one-channel convolutions keep CRC_NTTL1, moduli above 55 bits their kernels).  Tuning key scalar_mac /
 *                              CRC_SCALAR_MAC (default 1: the form beat the row path on every layer measured, profiles/scalar_mac.md): 0 gives crc_plan_mac's
 *                              answer everywhere */
size_t crc_scalar_weights_bytes(const crc_ctx *ctx, int nf, int zd, int xf, int yf);
int    crc_scalar_supported(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf);
int    crc_scalar_pack_weights(crc_ctx *ctx, const uint64_t *d_w, int w_stride, int nf, int zd, int xf, int yf, void *d_ws, int *constant, void *stream);
int    crc_plan_mac_scalar(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int B, int *w_form);
int    crc_plan_fold_pool(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int pxs, int pys, int pxf, int pyf, int *fold);
int    crc_plan_hoist_pool(const crc_ctx *ctx, int uzd, int uxd, int uyd, int uxs, int uys, int uxf, int uyf, int unf, int zd, int xd, int yd, int xs, int ys,
                           int xf, int yf, int nf, int pxs, int pys, int pxf, int pyf, int B, int matrix_cores, int *hoist);
/* The box of a one-channel convolution (CRC_NTTL1): the layer reads the bxf x byf WINDOW SUMS of its input, taken at its own stride (xs, ys) by the image pack --
 * conv_W(box x) = conv_{W * box}(x) over Z_q, so the upstream layer of a hoisted pair keeps its base window W instead of the enlarged one.  (xd, yd) is the full
 * image, (xf, yf) the BASE window; the result has ((xd - (bxf-1) xs - xf) / xs + 1) x ((yd - (byf-1) ys - yf) / ys + 1) positions; the bias is the caller's (a
 * folded sum pool's is bxf byf b).
 *   crc_limb_conv1_box_supported    pure host query, 0 / 1: the base window takes the pixel-major form of the kernel (at most 40 taps, not 17-20 filters), bxf byf
 *                                   <= 9, and the summed image is a shape crc_limb_conv1_supported accepts
 *   crc_conv2d_box_forms[_work_bytes]  crc_conv2d_forms' arguments plus the box; w_form must be CRC_NTTL1 (weights: crc_limb_conv1_pack_weights of the base
 *                                   window) unless the box is 1 x 1, which IS crc_conv2d_forms.  CRC_ERR_UNSUPPORTED (work bytes: 0) where the query says 0
 *   crc_plan_conv1_box              does the box execution cost less than the enlarged window (crc_plan_hoist_pool's units, plus the pack's extra reads)?  No where
 *                                   the query says 0, with matrix_cores = 0, and under the tuning key conv1_box = 0 / CRC_CONV1_BOX=0 */
int    crc_limb_conv1_box_supported(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf);
size_t crc_conv2d_box_forms_work_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf, int in_form,
                                       int w_form, int out_form);
int    crc_conv2d_box_forms(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_w, int w_form, const uint64_t *d_bias_delta, int B, int zd, int xd, int yd,
                            int xs, int ys, int xf, int yf, int nf, int bxf, int byf, int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream);
int    crc_plan_conv1_box(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int bxf, int byf, int B, int matrix_cores, int *box);
/* an NTT-form tensor (CRC_NTT canonical or CRC_NTTP) -> limb form; crc_conv2d_forms does this itself for such inputs, the separate entry point lets a
 * caller convert once and reuse (d_xl: crc_limb_tensor_bytes) */
int    crc_limb_pack_tensor(crc_ctx *ctx, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, void *d_xl, void *stream);
/* the same for images b0 .. b0 + B of a limb tensor of Btot images (d_xl: crc_limb_tensor_bytes(Btot, ...)): several chunks assemble the input of one
 * dense-layer launch
 * (a dense layer streams all of its weights per launch, so it is run on as many images as fit: netrun's / Network's two-level chunking) */
int    crc_limb_pack_tensor_at(crc_ctx *ctx, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, void *d_xl, int Btot, int b0, void *stream);
/* one-channel convolutions on the matrix cores (w_form = CRC_NTTL1): eligibility of a shape, size of the weights, conversion from CRC_NTT weights */
int    crc_limb_conv1_supported(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf);
size_t crc_limb_conv1_weights_bytes(const crc_ctx *ctx);
/* the kernel has two forms (tuning key conv1_form / CRC_CONV1_FORM: 0 by shape, 1 plane-major image, 2 pixel-major image with limb-folded weights, windows of at
 * most 40 taps; a forced form the shape cannot take falls back to the other).  The weights are packed for the form in force when crc_limb_conv1_pack_weights runs:
 * set the key before that and leave it alone afterwards.  crc_limb_conv1_weights_bytes is enough for either form, ..._for what the layer's own form needs;
 * crc_limb_conv1_form reports the form a shape runs (0: not a one-channel matrix-core shape) */
size_t crc_limb_conv1_weights_bytes_for(const crc_ctx *ctx, int nf, int xf, int yf);
int    crc_limb_conv1_form(const crc_ctx *ctx, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf);
int    crc_limb_conv1_pack_weights(crc_ctx *ctx, const uint64_t *d_w_ntt, int nf, int xf, int yf, void *d_wl, void *stream);
size_t crc_conv2d_forms_work_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf, int in_form, int w_form,
int out_form);
/* in-place CRC_NTT <-> CRC_NTTP conversion of `rows` residue rows (unpack = 0: pack, 1: unpack) */
int crc_pack28(crc_ctx *ctx, uint64_t *d_rows, size_t rows, int unpack, void *stream);
size_t crc_dense_work_bytes(const crc_ctx *ctx, int B, int in_dim, int out_dim, int in_form);
int crc_dense(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_w_ntt, const uint64_t *d_bias_delta,
              int B, int in_dim, int out_dim, int in_form, int out_form, uint64_t *d_y, void *d_work, void *stream);
int crc_pool(crc_ctx *ctx, const uint64_t *d_x, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
             const uint64_t *d_div_ntt /* NULL = sum pool */, int form, uint64_t *d_y, void *stream);
int crc_batchnorm(crc_ctx *ctx, uint64_t *d_x, int B, int zd, int xd, int yd, const uint64_t *d_mean_delta,
                  const uint64_t *d_invstd_ntt, int form, void *stream);
/* Zero padding (no layer of the reference: its convolution is valid-only).  d_x [B][zd][xd][yd] ciphertexts -> d_y [B][zd][px0 + xd + px1][py0 + yd + py1]:
 * the input in the interior, bit for bit, and all-zero ciphertexts -- the additive identity of BFV in either form -- on the border.  form: CRC_COEFF or
 * CRC_NTT, kept (the packed and limb operand forms are refused).  CRC_ERR_INVALID_ARGUMENT for a negative pad, a null or not 16-byte aligned pointer and a
 * d_y that overlaps d_x; a zero pad is a plain copy. */
int crc_pad(crc_ctx *ctx, const uint64_t *d_x, int B, int zd, int xd, int yd, int px0, int px1, int py0, int py1, int form, uint64_t *d_y, void *stream);
size_t crc_square_relin_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int crc_square_relin(crc_ctx *ctx, const uint64_t *d_x, size_t count, const uint64_t *d_evk, int dbc,
                     uint64_t *d_y, void *d_work, void *stream);
/* the same layer between NTT-resident neighbours: with in_form = CRC_NTT the given NTT values feed the products
 * and one inverse transform supplies the coefficients for the base extension; with out_form = CRC_NTT the tail adds
 * NTT(c0, c1) to the key-switched c2 instead of transforming back.  Identical ciphertexts in the requested form; 4k row
 * transforms fewer per ciphertext than converting outside. */
int crc_square_relin_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc,
                           uint64_t *d_y, int out_form, void *d_work, void *stream);
/* Square followed by a SUM pooling (CrCNN's act1 -> pool2; Network::fuse pairs them): relinearisation is linear in the digit polynomials of c2, so the digits
 * of
 * a window's ciphertexts are added and ONE key switch serves the pooled ciphertext --
 *     Sum_w relin(ct_w) = Sum_w (c0, c1)_w + Sum_g (Sum_w digit_g(c2'_w)) (*) key_g
 * -- the same element of Z_q as squaring, relinearising and pooling one after the other (evaluator.cpp:934-1069, poolingLayer.cpp:22-44), hence the same bits,
 * with xo yo / (xd yd) of the key switch's transforms and inner products (16 / 25 for CrCNN's 5 x 5 -> 4 x 4 pool2).  d_x: [B][zd][xd][yd] ciphertexts, d_y:
 * [B][zd][xo][yo].  d_div_ntt: an average pooling's divisor (NTT-form plaintext [k][n], as crc_pool takes it), multiplied in while an NTT-form result leaves
 * the
 * last kernel (out_form must be CRC_NTT then).  crc_square_pool_relin_supported: the key switch over
 * the fp64 primes must hold the window's larger integers (n D W 2^dbc q at most 2^92, a quarter of p_0 p_1) and a residue at most four digits. */
int    crc_square_pool_relin_supported(const crc_ctx *ctx, int dbc, int xf, int yf);
size_t crc_square_pool_relin_work_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int dbc);
int    crc_square_pool_relin_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
                                   const uint64_t *d_evk, int dbc, const uint64_t *d_div_ntt /* NULL = sum pool */, uint64_t *d_y, int out_form, void *d_work,
                                   void *stream);
/* Degree-2 polynomial activation c2 x^2 + c1 x + c0 (no layer of the reference, whose one non-linearity is x^2), defined per ciphertext x as the Evaluator sequence
 *     s = relinearize(square(x), evk);  s = multiply_plain(s, encode(c2));  s = add(s, multiply_plain(x, encode(c1)));  s = add_plain(s, encode(c0))
 * in coefficient form (a step is left out for c2 == 1, c1 == 0, c0 == 0).  c1 x and c0 are ring-linear in the ciphertext, so they join the key switch's result
 * while it leaves the last kernel, and the pooled form keeps ONE key switch per pooled ciphertext:
 *     Sum_w (c2 x_w^2 + c1 x_w + c0) = c2 Sum_w relin(x_w^2) + c1 Sum_w x_w + W c0.
 * d_p2_ntt / d_p1_ntt: NTT-form plaintext rows [k][n] (crc_plain_to_ntt of encode(c2) / encode(c1)); d_p0_ntt: the delta-form row of encode(c0) in NTT form
 * (crc_plain_to_delta, form = CRC_NTT), added to c0 only.  Any of them may be NULL: 1, 0 and 0 (all three NULL is crc_square_relin_forms /
 * crc_square_pool_relin_forms, bit for bit).  For the pooled call the HOST folds the window count and an average pooling's divisor into the rows (exact ring
 * arithmetic, done once): p2' = div (*) p2, p1' = div (*) p1, p0' = W div (*) p0 -- the call computes
 *     y = p2 (*) (Sum_w relin(x_w^2)) + p1 (*) (Sum_w NTT(x_w)) + [poly 0] p0.
 * Either form in and out: a coefficient-form side is transformed at the boundary inside the call, the result is the sequence's ciphertext in the requested
 * form.  With d_p1_ntt and in_form = CRC_NTT, d_y must not overlap d_x (CRC_ERR_INVALID_ARGUMENT).  crc_ctx_set_tuning "poly_tail": 0 the terms are added in the
 * key switch's last kernel wherever that runs over the fp64 primes, 1 always in a slot-wise kernel of their own (poly2_tail_kernel, which also serves
 * "sq_path" / "relin_path" = 1 and the moduli the fp64 key switch refuses).  crc_poly2_pool_relin_supported: the conditions of crc_square_pool_relin_supported. */
size_t crc_poly2_relin_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int    crc_poly2_relin_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc, const uint64_t *d_p2_ntt,
                             const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt, uint64_t *d_y, int out_form, void *d_work, void *stream);
int    crc_poly2_pool_relin_supported(const crc_ctx *ctx, int dbc, int xf, int yf);
size_t crc_poly2_pool_relin_work_bytes(const crc_ctx *ctx, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int dbc);
int    crc_poly2_pool_relin_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, int B, int zd, int xd, int yd, int xs, int ys, int xf, int yf,
                                  const uint64_t *d_evk, int dbc, const uint64_t *d_p2_ntt, const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt, uint64_t *d_y,
                                  int out_form, void *d_work, void *stream);
/* Ciphertext x ciphertext multiply: Evaluator::multiply of SEAL 2.3.1 (evaluator.cpp:356-700) for size-2 inputs x = (a, b), y = (c, d) -- BEHZ steps 0-4 with the
 * tensor product (ac, ad + bc, bd); the reference forms the middle term by Karatsuba, the same residue -- bit for bit on every kernel selection ("sq_path",
 * "f64_wave", ...), as the square.  d_x, d_y: [count] size-2 ciphertexts, multiplied pairwise; d_x == d_y is allowed and is the square (crc_square /
 * crc_square_relin_forms, to the bit); swapped arguments give equal bytes.
 *   crc_multiply              coefficient form in, size-3 ciphertexts out (unit tests; d_work: crc_multiply_relin_work_bytes with any valid dbc)
 *   crc_multiply_relin_forms  relinearize(multiply(x, y), evk); both inputs share in_form; forms as crc_square_relin_forms (CRC_COEFF or CRC_NTT only)
 * The result must not overlap either input: CRC_ERR_INVALID_ARGUMENT, like null pointers, a bad dbc and the packed or limb forms -- nothing is written then.
 * Cost: the lift and the forward transforms run for both inputs, floor and key switch once -- see profiles/ct_multiply.md. */
size_t crc_multiply_relin_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int    crc_multiply(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_y, size_t count, uint64_t *d_out3, void *d_work, void *stream);
int    crc_multiply_relin_forms(crc_ctx *ctx, const uint64_t *d_x, const uint64_t *d_y, int in_form, size_t count, const uint64_t *d_evk, int dbc,
                                uint64_t *d_out, int out_form, void *d_work, void *stream);
/* Degree-3 polynomial activation c3 x^3 + c2 x^2 + c1 x + c0, per ciphertext x the Evaluator sequence (coefficient form)
 *     s = relinearize(square(x), evk);  u = relinearize(multiply(s, x), evk);  r = multiply_plain(u, encode(c3));
 *     r = add(r, multiply_plain(s, encode(c2)));  r = add(r, multiply_plain(x, encode(c1)));  r = add_plain(r, encode(c0))
 * (a step is left out for c3 == 1, c2 == 0, c1 == 0, c0 == 0).  TWO key switches and a multiplicative depth of 2: the parameters must leave noise budget for
 * a second multiplication -- CrCNN's published (4096, two moduli, t = 2^29) leave none.  The rows are NTT-form plaintext rows [k][n] as crc_poly2_relin_forms
 * takes them (d_p0_ntt in delta form); NULL means 1, 0, 0, 0.  The lower terms are added slot-wise in NTT form, the same ring elements as the sequence.  d_out
 * must not overlap d_x (CRC_ERR_INVALID_ARGUMENT). */
size_t crc_poly3_relin_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int    crc_poly3_relin_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_evk, int dbc, const uint64_t *d_p3_ntt,
                             const uint64_t *d_p2_ntt, const uint64_t *d_p1_ntt, const uint64_t *d_p0_ntt, uint64_t *d_out, int out_form, void *d_work,
                             void *stream);
/* the two halves separately (unit tests): square -> size-3 ciphertexts; relinearize -> size 2 */
int crc_square(crc_ctx *ctx, const uint64_t *d_x, size_t count, uint64_t *d_y3, void *d_work, void *stream);
int crc_relinearize(crc_ctx *ctx, const uint64_t *d_x3, size_t count, const uint64_t *d_evk, int dbc, uint64_t *d_y,
                    void *d_work, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * SEAL memory/wire layout <-> engine layout (host)   ciphertext.cpp:103-130 ([size][k][n+1], pad word zero)
 * ------------------------------------------------------------------------------------------------------------- */
int crc_import_seal(const crc_ctx *ctx, const uint64_t *h_seal, int size, uint64_t *h_out);
int crc_export_seal(const crc_ctx *ctx, const uint64_t *h_in, int size, uint64_t *h_seal);
/* SEAL 2.3.1 wire formats (byte-compatible with Ciphertext::save ciphertext.cpp:103-113, EvaluationKeys::save
 * evaluationkeys.cpp:8-39, PublicKey/SecretKey::save publickey.h:81-98 / secretkey.h:86-107), incl. the 32-byte SHA3-256
 * parameter hash (encryptionparams.cpp:69-100) that SEAL checks on every object.  *_load rejects a wrong hash / shape with
 * CRC_ERR_INVALID_ARGUMENT ("not valid for encryption parameters").  Buffers are host memory. */
int    crc_params_hash(const crc_ctx *ctx, uint64_t out[4]);
size_t crc_seal_ct_bytes(const crc_ctx *ctx, int size);
size_t crc_seal_evk_bytes(const crc_ctx *ctx, int dbc);
size_t crc_seal_pk_bytes(const crc_ctx *ctx);
size_t crc_seal_sk_bytes(const crc_ctx *ctx);
int crc_seal_ct_save(const crc_ctx *ctx, const uint64_t *h_ct, int size, void *buf, size_t cap, size_t *written);
int crc_seal_ct_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_ct, int max_size, int *size, size_t *consumed);
int crc_seal_evk_save(const crc_ctx *ctx, const uint64_t *h_evk, int dbc, void *buf, size_t cap, size_t *written);
int crc_seal_evk_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_evk, int *dbc);
int crc_seal_pk_save(const crc_ctx *ctx, const uint64_t *h_pk, void *buf, size_t cap, size_t *written);
int crc_seal_pk_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_pk);
int crc_seal_sk_save(const crc_ctx *ctx, const uint64_t *h_sk_ntt, void *buf, size_t cap, size_t *written);
int crc_seal_sk_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_sk_ntt);

/* ---------------------------------------------------------------------------------------------------------------
 * model loader (host)   replaces LoadH5::getDataVfloat (CrCNN/src/H5Easy.cpp:584-644) as used by
 *           CnnBuilder::getPretrained (cnnBuilder.cpp:20-23): flat float32 read of dataset `name` (e.g.
 *           "pool1_features.conv1.weight") from an HDF5 file written by PlainModel/ToH5.py.
 *           Two readers behind these entry points: a built-in one for the files the reference ships (superblock v0, contiguous little-endian
 *           float32 datasets; no dependency), and -- for every other layout: newer superblocks, chunked / compressed datasets, other float
 *           types -- libhdf5 itself, the library the reference links, loaded with dlopen when the machine has it (CRC_LIBHDF5 names one;
 *           CRC_H5_BACKEND=lite|hdf5 forces a reader).  A file neither can read gives CRC_ERR_IO.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_h5_backend_available(void);                               /* 1 when libhdf5 (>= 1.10) could be loaded */
int crc_h5_dataset_count(const char *path, const char *name, size_t *count);
int crc_h5_read_f32(const char *path, const char *name, float *h_out, size_t cap, size_t *count);
int crc_h5_list(const char *path, char *h_names, size_t cap);   /* newline-separated dataset names */

/* ---------------------------------------------------------------------------------------------------------------
 * client side (host CPU; SURVEY 8f-2, outside the accelerated path): keygen / encrypt / decrypt so that a user of
 * CrCNN's globals.cpp (setParameters, encryptImage, decryptImage: globals.cpp:25-56,127-157,207-230) finds them.
 *
 * Randomness.  SEAL 2.3.1 draws from std::random_device (randomgen.cpp:7), so the reference fixes sampling LAWS (uniform
 * ternary secret / encryption sample, clipped normal sigma 3.19 cut at 6 sigma: util/globals.cpp:13-15), not bits.  Here every
 * sample comes from ChaCha20 keystreams under a 256-bit key:
 *   *_key entry points   take the key (CRC_KEY_BYTES bytes).  Draw it with crc_random_key (getrandom(2)) -- that is the
 *                        secure way and what the C++ host classes do on every setParameters().  One key may serve keygen,
 *                        evaluation keys and any number of encryptions: each use has its own stream (domain, `stream_base` +
 *                        ciphertext index, coefficient).  NEVER encrypt two different batches under the same (key, stream_base).
 *   uint64 seed variants expand a PUBLIC 64-bit seed into the key.  Deterministic by design: tests, bench, golden vectors.
 *                        NOT SECURE -- anyone who knows the seed can decrypt.
 * ------------------------------------------------------------------------------------------------------------- */
#define CRC_KEY_BYTES 32
int crc_random_key(uint8_t *h_key /*[CRC_KEY_BYTES]*/);
/* one ChaCha20 block (RFC 8439: 32-byte key, 32-bit block counter, 12-byte nonce -> 64 bytes): known-answer access to the generator */
int crc_chacha20_block(const uint8_t *h_key, uint32_t counter, const uint8_t *h_nonce /*[12]*/, uint8_t *h_out /*[64]*/);
int crc_keygen_key(const crc_ctx *ctx, const uint8_t *h_key, uint64_t *h_sk_ntt /*[k][n]*/, uint64_t *h_pk /*[2][k][n]*/);
int crc_gen_evk_key(const crc_ctx *ctx, const uint8_t *h_key, const uint64_t *h_sk_ntt, int dbc, uint64_t *h_evk);
int crc_encrypt_key(const crc_ctx *ctx, const uint64_t *h_pk, const uint64_t *h_plain, size_t count, const uint8_t *h_key, uint64_t stream_base,
                    uint64_t *h_ct /*[count][2][k][n]*/);
int crc_keygen(const crc_ctx *ctx, uint64_t seed, uint64_t *h_sk_ntt /*[k][n]*/, uint64_t *h_pk /*[2][k][n]*/);
int crc_gen_evk(const crc_ctx *ctx, uint64_t seed, const uint64_t *h_sk_ntt, int dbc, uint64_t *h_evk);
int crc_encrypt(const crc_ctx *ctx, const uint64_t *h_pk, const uint64_t *h_plain, size_t count, uint64_t seed, uint64_t *h_ct /*[count][2][k][n]*/);
int crc_decrypt(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_ct, size_t count, int size, uint64_t *h_plain /*[count][n]*/);
int crc_noise_budget(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_ct, int size);

/* Encryptor::encrypt (encryptor.cpp:71-134) on the device, for the 784 encryptions per image that dominate the client's
 * latency in the reference: d_pk = the public key of crc_keygen copied to the device ([2][k][n], NTT form), d_plain =
 * [count][n] plaintext coefficients (< t), d_ct = [count][2][k][n] coefficient form.  Sampling (ternary u, clipped-normal
 * e1/e2) is ChaCha20 in counter mode, one stream (one block) per (ciphertext, coefficient pair): same laws as crc_encrypt, different bits.
 * d_work: crc_encrypt_dev_work_bytes(count). */
size_t crc_encrypt_dev_work_bytes(const crc_ctx *ctx, size_t count);
int crc_encrypt_dev_key(crc_ctx *ctx, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, const uint8_t *h_key, uint64_t stream_base,
                        uint64_t *d_ct, void *d_work, void *stream);
int crc_encrypt_dev(crc_ctx *ctx, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, uint64_t seed, uint64_t *d_ct, void *d_work, void *stream);
/* The same with the form of the result chosen: CRC_COEFF (as above) or CRC_NTT -- c_p = NTT(e_p (+ Delta m)) + pk_p . NTT(u), three forward transforms per
 * modulus and no inverse one; the residues are those of crc_ntt_fwd applied to the coefficient-form result of the same (seed / key, stream) -- for a network
 * whose first layer takes NTT-form inputs (every convolution here does: the transform it would run on a coefficient-form image is skipped). */
int crc_encrypt_dev_key_forms(crc_ctx *ctx, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, const uint8_t *h_key, uint64_t stream_base, int out_form,
                              uint64_t *d_ct, void *d_work, void *stream);
int crc_encrypt_dev_forms(crc_ctx *ctx, const uint64_t *d_pk, const uint64_t *d_plain, size_t count, uint64_t seed, int out_form, uint64_t *d_ct, void *d_work,
                          void *stream);
/* The device encryptor samples its noise integers e in [-19, 19] directly from their law (the reference's N(0, 3.19^2) clipped at 6 sigma and truncated,
 * encryptor.cpp:237-240): |e| = the number of these 19 thresholds T_a = floor(2^64 P(|e| <= a)) that a uniform 64-bit word reaches.  For tests. */
void crc_encrypt_dev_noise_thresholds(uint64_t *h_out19);

/* Decryptor::decrypt (SEAL decryptor.cpp:107-236) on the device: d_sk_ntt = the secret key of crc_keygen copied to the device ([k][n], NTT form), d_ct =
 * [count][size][k][n] ciphertexts of `size` 2 or 3 in `in_form` CRC_COEFF or CRC_NTT (an NTT-resident tensor is decrypted as it stands: c0 + c1 s is formed in
 * the NTT domain and ONE inverse transform per residue follows), d_plain = [count][n] plaintext coefficients below t -- the polynomial crc_decrypt and the
 * reference produce, bit for bit (dot product with the secret key, inverse transform, BEHZ correction with the auxiliary prime gamma:
 * util/baseconverter.cpp:744-797).  d_work: crc_decrypt_dev_work_bytes(count, size, in_form).  Asynchronous on `stream`. */
size_t crc_decrypt_dev_work_bytes(const crc_ctx *ctx, size_t count, int size, int in_form);
int crc_decrypt_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct, size_t count, int size, int in_form, uint64_t *d_plain, void *d_work,
                    void *stream);
/* Decryptor::invariant_noise_budget (SEAL decryptor.cpp:295-403) on the device, for every ciphertext of a tensor at once: d_sk_ntt and d_ct as crc_decrypt_dev
 * takes them ([count][size][k][n], `size` 2 or 3, `in_form` CRC_COEFF or CRC_NTT).  Per ciphertext: v = c0 + c1 s (+ c2 s^2) mod q (decryptor.cpp:333-359, the
 * decryptor's dot product and inverse transforms), per coefficient t v mod q composed from its residues as a multi-word integer and centred against
 * floor(q/2) (:361-384), the largest significant bit count over the n coefficients (:386-399), and d_bits[m] = max(0, bits(q) - that - 1) (:400-403) -- the
 * integer crc_noise_budget and the reference report, bit for bit.  d_min (may be NULL) receives {the smallest budget, the index of its first occurrence}: a
 * caller who only asks whether a tensor still decrypts copies two integers back.  count == 0 is CRC_OK and writes nothing.
 * d_work: crc_noise_budget_dev_work_bytes(count, size, in_form) (0 for a size or form the call refuses).  Asynchronous on `stream`.
 * crc_budget_bits_host runs the same per-coefficient routine on the host (any context, device = -1 included) on coefficient-form residues of v,
 * h_v [count][k][n]: what the device computes behind the inverse transforms, for tests of the multi-word arithmetic that need no GPU. */
size_t crc_noise_budget_dev_work_bytes(const crc_ctx *ctx, size_t count, int size, int in_form);
int crc_noise_budget_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct, size_t count, int size, int in_form, int32_t *d_bits /*[count]*/,
                         int32_t *d_min /*[2]: min, index; may be NULL*/, void *d_work, void *stream);
int crc_budget_bits_host(const crc_ctx *ctx, const uint64_t *h_v /*[count][k][n], coefficient form*/, size_t count, int32_t *h_bits /*[count]*/);
/* -------------------------------------------------------------------------------------------------------------
 * Slot batching (SEAL's PolyCRTBuilder, polycrt.cpp:82-147, 327-370): with a PRIME plain modulus t = 1 (mod 2n) a plaintext is n independent numbers of Z_t,
 * and ciphertext addition, multiplication by a plaintext, square and multiply act on every slot separately -- image j of a batch in slot j makes one
 * ciphertext tensor carry up to n images through the same kernels.  psi = the minimal primitive 2n-th root of unity mod t ("slots_root" of crc_ctx_table),
 * m = 2n, pos_i = 3^i mod m, idx[i] = bitrev((pos_i - 1)/2, log n), idx[n/2 + i] = bitrev((m - pos_i - 1)/2, log n) for i < n/2 ("slots_index_map"):
 *   compose    v[0..slots) -> v[i] mod t at position idx[i] of a row, zeros at idx[i] for i >= slots, inverse negacyclic transform mod t = the coefficients
 *   decompose  forward transform mod t; slot i = position idx[i], returned as the centred representative in [-(t-1)/2, (t-1)/2]
 * i.e. slot i of p is p(psi^(3^i)) and slot n/2 + i is p(psi^(-3^i)).  A constant polynomial w is the number w in every slot.
 * Values are int64; (item c, slot i) sits at values[c item_stride + i slot_stride]: image-major data [slots][count] is (1, count), item-major (slots, 1).
 * ANY int64 is accepted and taken as its residue mod t: SEAL throws for a value outside the plain modulus, a device kernel cannot.  Plaintext words read by
 * decompose are reduced mod t the same way.
 *   crc_slots_supported   1 only if t is prime, t = 1 (mod 2n) and t differs from every modulus the context computes with (the q_i, the Bsk base, gamma, the
 *                         fp64 primes of the square and the key switch)
 *   crc_slots_prime       the largest prime below 2^bits that is 1 (mod 2n), 2 <= bits <= 60 (CRC_ERR_NOT_FOUND if there is none)
 *   crc_slots_compose / crc_slots_decompose            host memory, any context (device = -1 included)
 *   crc_slots_compose_dev / crc_slots_decompose_dev    device memory, asynchronous on `stream`, no work buffer: one kernel, one workgroup per row
 *                         (kernels_slots.hip); d_plain 16-byte aligned; n <= 16384 (CRC_ERR_UNSUPPORTED above)
 * The tables of t are built by the first of these calls (or by crc_ctx_table), not by crc_ctx_create; on a device context that first call uploads them and
 * synchronises once.  Every entry point returns CRC_ERR_PARAMETERS on a context where crc_slots_supported is 0, CRC_ERR_INVALID_ARGUMENT for slots outside
 * [1, n], null pointers or a zero stride.  The caller guarantees that the values buffer covers (count - 1) item_stride + (slots - 1) slot_stride.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_slots_supported(const crc_ctx *ctx);
int crc_slots_prime(int n, int bits, uint64_t *t);
int crc_slots_compose(crc_ctx *ctx, const int64_t *h_values, size_t count, int slots, size_t item_stride, size_t slot_stride, uint64_t *h_plain /*[count][n]*/);
int crc_slots_decompose(crc_ctx *ctx, const uint64_t *h_plain /*[count][n]*/, size_t count, int slots, int64_t *h_values, size_t item_stride, size_t slot_stride);
int crc_slots_compose_dev(crc_ctx *ctx, const int64_t *d_values, size_t count, int slots, size_t item_stride, size_t slot_stride, uint64_t *d_plain, void *stream);
int crc_slots_decompose_dev(crc_ctx *ctx, const uint64_t *d_plain, size_t count, int slots, int64_t *d_values, size_t item_stride, size_t slot_stride,
                            void *stream);
/* rescale: every slot of a plaintext divided by an integer -- the re-encoding a slot-batched network needs where its scale has to come down.  For a row p (n
 * words, each taken mod t) and 1 <= divisor D <= 2^62: v_i = the centred value of slot i (all n slots), v'_i = floor(v_i / D + 1/2) (floor division: ties go
 * towards +infinity), result = the canonical coefficients of compose(v').  D = 1 returns p reduced mod t; zero slots stay zero; no slot count is needed, the
 * operation is the same in every slot.  crc_slots_rescale: host memory, any context.  crc_slots_rescale_dev: device memory, asynchronous on `stream`, one kernel,
 * one workgroup per row, no work buffer; both pointers 16-byte aligned, d_plain_out may be d_plain_in; n <= 16384 (CRC_ERR_UNSUPPORTED above); count = 0 is
 * CRC_OK.  CRC_ERR_PARAMETERS on a context without slots comes first, then CRC_ERR_INVALID_ARGUMENT for D = 0, D > 2^62 or a null pointer.
 *
 * crc_slots_refresh_*: the client-side refresh of a slot-batched tensor -- crc_decrypt_dev (size 2), crc_slots_rescale_dev in place on the plaintexts,
 * crc_encrypt_dev[_key]_forms (public key) / crc_encrypt_sym_dev[_key]_forms (secret key) -- as one call on `stream`; the result is by definition bit for bit
 * what those three calls give with the same seed or key + stream_base.  in_form / out_form: CRC_COEFF or CRC_NTT; d_ct_out may be d_ct_in; d_work of
 * crc_slots_refresh[_sym]_dev_work_bytes(ctx, count, in_form) bytes. */
int crc_slots_rescale(crc_ctx *ctx, const uint64_t *h_plain_in /*[count][n]*/, size_t count, uint64_t divisor, uint64_t *h_plain_out /*[count][n]*/);
int crc_slots_rescale_dev(crc_ctx *ctx, const uint64_t *d_plain_in, size_t count, uint64_t divisor, uint64_t *d_plain_out, void *stream);
size_t crc_slots_refresh_dev_work_bytes(const crc_ctx *ctx, size_t count, int in_form);
int crc_slots_refresh_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor,
                          uint64_t seed, int out_form, uint64_t *d_ct_out, void *d_work, void *stream);
int crc_slots_refresh_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor,
                              const uint8_t *h_key /*[32]*/, uint64_t stream_base, int out_form, uint64_t *d_ct_out, void *d_work, void *stream);
size_t crc_slots_refresh_sym_dev_work_bytes(const crc_ctx *ctx, size_t count, int in_form);
int crc_slots_refresh_sym_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor, uint64_t seed,
                              int out_form, uint64_t *d_ct_out, void *d_work, void *stream);
int crc_slots_refresh_sym_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t divisor,
                                  const uint8_t *h_key /*[32]*/, uint64_t stream_base, int out_form, uint64_t *d_ct_out, void *d_work, void *stream);

/* act: the client-side ReLU and max pooling of a slot-batched network, taken where the rescale is taken -- while the slots are in the clear between decrypt and
 * encrypt.  Input: plaintext rows p[planes][xd][yd][n], every word taken mod t; an xf x yf window of stride (xs, ys) the library's window test admits, outputs
 * xo x yo = ((xd - xf) / xs + 1) x ((yd - yf) / ys + 1); 1 <= divisor D <= 2^62; relu 0 or 1; 0 <= cap <= (t - 1) / 2 (0: no cap).  For every output (pl, i, j)
 * and every one of the n slots s:
 *     m = max over a < xf, b < yf of the centred value of slot s of p[pl][i xs + a][j ys + b]
 *     r = floor(m / D + 1/2) (floor division, ties towards +infinity, as the rescale);  relu: r = max(r, 0);  cap: r = min(r, cap)
 *     out[pl][i][j] = the canonical coefficients of compose(r)
 * Rounding is non-decreasing, so r is also the maximum of the individually rescaled values.  relu = 0, cap = 0 and a 1 x 1 window of stride 1 is
 * crc_slots_rescale, bit for bit.  crc_slots_act: host memory, any context.  crc_slots_act_dev: device memory, asynchronous on `stream`, one kernel, one
 * workgroup per output row, no work buffer; both pointers 16-byte aligned; d_plain_out may equal d_plain_in only for a 1 x 1 window of stride 1, any other overlap
 * of the two tensors is CRC_ERR_INVALID_ARGUMENT and nothing is written; n <= 16384 (CRC_ERR_UNSUPPORTED above).  CRC_ERR_PARAMETERS on a context without slots
 * comes first, then CRC_ERR_INVALID_ARGUMENT for a bad divisor, relu outside {0, 1}, cap > (t - 1) / 2, a refused window, a null or misaligned pointer;
 * planes = 0 is CRC_OK.
 *
 * crc_slots_refresh_act_*: crc_decrypt_dev (size 2) of all planes * xd * yd ciphertexts, crc_slots_act_dev, crc_encrypt_dev[_key]_forms (public key) /
 * crc_encrypt_sym_dev[_key]_forms (secret key) of the planes * xo * yo outputs, as one call on `stream`; by definition bit for bit what those three calls give
 * with the same seed or key + stream_base.  A 2 x 2 window of stride 2 re-encrypts a quarter of the ciphertexts it decrypts.  d_ct_out may be d_ct_in (the whole
 * input is decrypted into the work space before anything is written); d_work of crc_slots_refresh_act[_sym]_dev_work_bytes(...) bytes.
 * Security is the rescale's: the key holder sees the activations at this point, nobody else does. */
int crc_slots_act(crc_ctx *ctx, const uint64_t *h_plain_in /*[planes][xd][yd][n]*/, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, uint64_t divisor,
                  int relu, uint64_t cap, uint64_t *h_plain_out /*[planes][xo][yo][n]*/);
int crc_slots_act_dev(crc_ctx *ctx, const uint64_t *d_plain_in, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, uint64_t divisor, int relu,
                      uint64_t cap, uint64_t *d_plain_out, void *stream);
size_t crc_slots_refresh_act_dev_work_bytes(const crc_ctx *ctx, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, int in_form);
int crc_slots_refresh_act_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys,
                              int xf, int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, uint64_t seed, int out_form, uint64_t *d_ct_out, void *d_work,
                              void *stream);
int crc_slots_refresh_act_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs,
                                  int ys, int xf, int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *h_key /*[32]*/, uint64_t stream_base,
                                  int out_form, uint64_t *d_ct_out, void *d_work, void *stream);
size_t crc_slots_refresh_act_sym_dev_work_bytes(const crc_ctx *ctx, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf, int in_form);
int crc_slots_refresh_act_sym_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys, int xf, int yf,
                                  int in_form, uint64_t divisor, int relu, uint64_t cap, uint64_t seed, int out_form, uint64_t *d_ct_out, void *d_work, void *stream);
int crc_slots_refresh_act_sym_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t planes, int xd, int yd, int xs, int ys, int xf,
                                      int yf, int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *h_key /*[32]*/, uint64_t stream_base,
                                      int out_form, uint64_t *d_ct_out, void *d_work, void *stream);

/* Several plain moduli.  One slot prime t has to hold the largest integer a slot-batched network forms, and every square costs about log2 t + log2 n bits of
 * noise budget.  A residue base runs the same network under r small pairwise coprime plain moduli and recombines the slots by the Chinese remainder theorem
 * into integers mod T = t_0 ... t_{r-1}.  The base is 1 <= r <= CRC_SLOTS_CRT_MAX contexts `ctxs[0 .. r-1]` of the same n and the same device, every one with
 * crc_slots_supported, their t_j pairwise distinct and T < 2^63 (every centred integer mod T is an int64): crc_slots_crt_supported says 1 for exactly these.
 * The keys do not involve t: one key set serves r contexts that share n and q.  Composing a batch is r calls of crc_slots_compose[_dev] on the same int64
 * values.  What cannot be composed from the calls above -- a rescale or an activation does not commute with the reduction mod t_j -- is here:
 *   crc_slots_crt_primes     the r largest primes below 2^bits that are 1 (mod 2n), descending; CRC_ERR_NOT_FOUND if fewer exist or their product is >= 2^63
 *   crc_slots_crt_decompose  plain[j] = plaintext rows [count][n] of ctxs[j]; values (item c, slot i) at values[c item_stride + i slot_stride], i < slots: the
 *                            centred integer mod T whose residue mod t_j is slot i of plain[j][c] for every j
 *   crc_slots_crt_act        per slot, with V that centred integer: rho = floor(V / D + 1/2) (floor division, ties towards +infinity), 1 <= D <= 2^62; relu:
 *                            rho = max(rho, 0); cap: rho = min(rho, cap), 0 <= cap <= (T - 1) / 2, 0 meaning none; out[j] = the canonical coefficients of
 *                            compose(rho mod t_j) under ctxs[j].  out[j] may be in[j]; an output row tensor must not overlap anything else
 *   crc_slots_crt_refresh_*  by definition, bit for bit: crc_decrypt_dev (size 2) on every ctxs[j], crc_slots_crt_act_dev on the r plaintext tensors,
 *                            crc_encrypt_dev_key_forms / crc_encrypt_sym_dev_key_forms on every ctxs[j] with stream base stream_base + j count, on one stream.
 *                            d_ct_out[j] may be d_ct_in[j]; d_work of crc_slots_crt_refresh_dev_work_bytes bytes serves either call
 * The pointer arrays are HOST arrays of r host (crc_slots_crt_decompose / _act) or device (_dev, refresh) pointers, read before the call returns; every device
 * row pointer is 16-byte aligned.  The host calls work on any context.  The _dev calls are one kernel each, one workgroup per item, no work buffer, asynchronous on
 * `stream`.  Refusals, in this order, nothing written: CRC_ERR_INVALID_ARGUMENT for r outside [1, CRC_SLOTS_CRT_MAX] or a null entry of ctxs;
 * CRC_ERR_PARAMETERS where crc_slots_crt_supported is 0; CRC_ERR_INVALID_ARGUMENT for a bad divisor, relu outside {0, 1}, cap > (T - 1) / 2, slots outside [1, n],
 * a zero stride, a null or misaligned pointer, an output row tensor that overlaps any other than its own input; CRC_ERR_UNSUPPORTED for n > 16384 (device).
 * count = 0 is CRC_OK.  At r = 1 the calls are crc_slots_decompose[_dev], crc_slots_act[_dev] on a 1 x 1 window and crc_slots_refresh_act[_sym]_dev_key, to the bit. */
#define CRC_SLOTS_CRT_MAX 4
int crc_slots_crt_supported(crc_ctx *const *ctxs, int r);
int crc_slots_crt_primes(int n, int r, int bits, uint64_t *t /*[r]*/);
int crc_slots_crt_decompose(crc_ctx *const *ctxs, int r, const uint64_t *const *h_plain /*[r] -> [count][n]*/, size_t count, int slots, int64_t *h_values,
                            size_t item_stride, size_t slot_stride);
int crc_slots_crt_decompose_dev(crc_ctx *const *ctxs, int r, const uint64_t *const *d_plain, size_t count, int slots, int64_t *d_values, size_t item_stride,
                                size_t slot_stride, void *stream);
int crc_slots_crt_act(crc_ctx *const *ctxs, int r, const uint64_t *const *h_in /*[r] -> [count][n]*/, size_t count, uint64_t divisor, int relu, uint64_t cap,
                      uint64_t *const *h_out);
int crc_slots_crt_act_dev(crc_ctx *const *ctxs, int r, const uint64_t *const *d_in, size_t count, uint64_t divisor, int relu, uint64_t cap, uint64_t *const *d_out,
                          void *stream);
size_t crc_slots_crt_refresh_dev_work_bytes(crc_ctx *const *ctxs, int r, size_t count, int in_form);
int crc_slots_crt_refresh_dev_key(crc_ctx *const *ctxs, int r, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *const *d_ct_in, size_t count,
                                  int in_form, uint64_t divisor, int relu, uint64_t cap, const uint8_t *h_key /*[32]*/, uint64_t stream_base, int out_form,
                                  uint64_t *const *d_ct_out, void *d_work, void *stream);
int crc_slots_crt_refresh_sym_dev_key(crc_ctx *const *ctxs, int r, const uint64_t *d_sk_ntt, const uint64_t *const *d_ct_in, size_t count, int in_form,
                                      uint64_t divisor, int relu, uint64_t cap, const uint8_t *h_key /*[32]*/, uint64_t stream_base, int out_form,
                                      uint64_t *const *d_ct_out, void *d_work, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Galois automorphisms: Evaluator::apply_galois / rotate_rows / rotate_columns (evaluator.cpp:1587-1834) and KeyGenerator::generate_galois_keys
 * (keygenerator.cpp:325-455) -- the operations that move data between the slots of a batched ciphertext.
 *
 * A Galois element g is valid iff it is odd and 1 <= g < 2n.  sigma_g maps a coefficient row mod q as util::apply_galois does: out[(i g) mod n] = in[i] where bit
 * log2 n of i g is clear, (q - in[i]) mod q where it is set.  apply_galois(ct, g) = (sigma(c0), 0) + KeySwitch_g(sigma(c1)): relinearisation's key switch (the
 * same (q/q_i)^-1 premultiply, dbc-bit digits, lazy inner products, inverse transform) with the key of g.  The result is canonical: the reference's ciphertext
 * bit for bit under the same key blob.  g = 1 is a copy and needs no key.
 *
 * Keys: one blob of crc_evk_words(ctx, dbc) words per element, laid out exactly as an evaluation-key blob with s^2 replaced by sigma_g(s).  A key SET is the
 * host list elts[n_elts] and the blobs [n_elts][crc_evk_words] in the same order (d_gk: the blobs in device memory, 16-byte aligned).  Randomness: a ChaCha20
 * stream per element (a domain of its own, the element in the nonce), so a key does not depend on which other elements the set holds.
 *   crc_galois_elt_valid      1 / 0
 *   crc_galois_elt_rows       the element of rotate_rows(steps): 3^steps mod 2n, a negative step count taken as n/2 - |steps|; 1 for steps = 0; 0 for
 *                             |steps| >= n/2 ("step count too large")
 *   crc_galois_elt_columns    2n - 1
 *   crc_galois_default_elts   the set of generate_galois_keys(dbc): 2n - 1, then 3^(2^i), 3^(-2^i) mod 2n for i < log2 n - 1, in that order, each once (3^(n/4) is its own
 *                             inverse: 2 log2 n - 2 elements).  Returns the count (out = NULL: only that); CRC_ERR_INVALID_ARGUMENT if cap is smaller
 *   crc_gen_galois_keys[_key] host memory, any context; seed / key as crc_gen_evk[_key].  CRC_ERR_INVALID_ARGUMENT for an invalid element or dbc
 *   crc_galois_plan           the steps apply_galois(g) takes with the keys of elts: indices into elts, in order, their count returned.  0 for g = 1; 1 where g
 *                             is in the set; otherwise g = 3^o1 (-1)^o2, o1 replaced by n/2 - o1 over 3^-1 where that has the smaller Hamming weight, one step
 *                             gen^(2^b) per set bit b of o1 from the low end, then 2n - 1 if o2 is set (evaluator.cpp:1623-1661).  CRC_ERR_INVALID_ARGUMENT
 *                             if a step's key is absent ("galois key not present"), g is invalid or cap is too small (log2 n always suffices)
 * Device entry points (asynchronous on `stream`; a host-only context gets CRC_ERR_INVALID_ARGUMENT as from every device entry point):
 *   crc_galois_permute_dev    unit-test access to the kernel (kernels_galois.hip): coefficient-form d_x [count][2][k][n] -> d_x3 [count][3][k][n] =
 *                             (sigma(c0), 0, sigma(c1) (q/q_i)^-1 mod q_i), with accumulate != 0 (sigma(c0) + c0, c1, the same) -- what crc_relinearize's
 *                             key switch takes after its own premultiply
 *   crc_apply_galois_forms    runs the plan's steps in order.  in_form / out_form: CRC_COEFF or CRC_NTT (an NTT-form side is transformed inside the call: the
 *                             same ciphertext transformed).  d_work: crc_apply_galois_work_bytes(ctx, count, dbc) bytes, bounded in count (internal passes of
 *                             whole ciphertexts as crc_relinearize; a step's prepared keys are made once per step, not per pass)
 *   crc_rotate_rows_forms     crc_apply_galois_forms with crc_galois_elt_rows(steps): with the slot order of crc_slots_compose the n slots are a 2 x n/2 matrix
 *                             and new slot i of each row = old slot (i + steps) mod n/2 -- a rotation to the left for positive steps
 *   crc_rotate_columns_forms  crc_apply_galois_forms with 2n - 1: the two rows swap
 *   crc_sum_slots_forms       y = x; y += rotate_rows(y, 2^j) for j < log2(n/2); y += rotate_columns(y): every slot of y holds the sum of all n slots of x mod
 *                             t, in log2 n key switches.  Each y + rotate(y) is formed inside the step (no add pass) and equals crc_add(y, rotate(y)) bit for
 *                             bit.  Every element (all in the default set) must have its own key in elts
 * CRC_ERR_INVALID_ARGUMENT for a null or not 16-byte aligned d_x / d_y / d_gk, a d_y that overlaps d_x, a d_work that overlaps either, an invalid element or step count, a missing key, a
 * form other than CRC_COEFF / CRC_NTT and a dbc outside 1..60 (work bytes: 0) -- nothing is launched then; the rotations and the slot sum give
 * CRC_ERR_PARAMETERS first where crc_slots_supported is 0.  count = 0 is CRC_OK.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_galois_elt_valid(const crc_ctx *ctx, uint64_t g);
uint64_t crc_galois_elt_rows(const crc_ctx *ctx, int steps);
uint64_t crc_galois_elt_columns(const crc_ctx *ctx);
int crc_galois_default_elts(const crc_ctx *ctx, uint64_t *out, int cap);
int crc_gen_galois_keys_key(const crc_ctx *ctx, const uint8_t *h_key, const uint64_t *h_sk_ntt, int dbc, const uint64_t *elts, int n_elts,
                            uint64_t *h_gk /*[n_elts][crc_evk_words]*/);
int crc_gen_galois_keys(const crc_ctx *ctx, uint64_t seed, const uint64_t *h_sk_ntt, int dbc, const uint64_t *elts, int n_elts,
                        uint64_t *h_gk /*[n_elts][crc_evk_words]*/);
int crc_galois_plan(const crc_ctx *ctx, uint64_t g, const uint64_t *elts, int n_elts, int *steps_out, int cap);
int crc_galois_permute_dev(crc_ctx *ctx, const uint64_t *d_x, size_t count, uint64_t g, int accumulate, uint64_t *d_x3, void *stream);
size_t crc_apply_galois_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int crc_apply_galois_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, uint64_t g, const uint64_t *d_gk, const uint64_t *elts, int n_elts,
                           int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream);
int crc_rotate_rows_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, int steps, const uint64_t *d_gk, const uint64_t *elts, int n_elts,
                          int dbc, uint64_t *d_y, int out_form, void *d_work, void *stream);
int crc_rotate_columns_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_gk, const uint64_t *elts, int n_elts, int dbc,
                             uint64_t *d_y, int out_form, void *d_work, void *stream);
size_t crc_sum_slots_work_bytes(const crc_ctx *ctx, size_t count, int dbc);
int crc_sum_slots_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *d_gk, const uint64_t *elts, int n_elts, int dbc,
                        uint64_t *d_y, int out_form, void *d_work, void *stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Hoisted rotations: many automorphisms of ONE ciphertext from one digit decomposition, and the diagonal product over slots that consumes them.
 *
 * For an element g with key K_g (crc_gen_galois_keys: a key from sigma_g(s) to s) the CONJUGATED key is K'_g = sigma_g^-1(K_g): sigma_{g^-1 mod 2n} of every
 * polynomial of the blob, the same layout and size.  The gadget constants are integers, which sigma fixes, so K'_g switches from s to sigma_g^-1(s), and
 *     H_g(ct) := sigma_g( (c0, 0) + KeySwitch(c1; K'_g) )
 * decrypts to sigma_g(m) with the noise law of apply_galois.  KeySwitch is relinearisation's: the (q/q_i)^-1 premultiply, unsigned dbc-bit digits of the canonical
 * residue, the inner product mod q_j.  The digits are those of c1 itself -- independent of g, so they and their transforms are made once for all elements of a
 * call.  H_g is NOT apply_galois(ct, g) bit for bit (the digits of sigma(c1) are not sigma of the digits of c1 wherever sigma negates): it is an operation of its
 * own, and the text above fixes its bits on either key-switch path, every step being an exact function on Z_q.
 *   crc_galois_ntt_table        the automorphism on an NTT-form row is an index gather, the same for every modulus: NTT(sigma_g(p))[i] = NTT(p)[table[i]]
 *   crc_galois_conjugate_keys   host memory, any context: h_out[e] = K'_{elts[e]} from h_gk[e] = K_{elts[e]}.  CRC_ERR_INVALID_ARGUMENT for an invalid element,
 *                               for g = 1 (it has no key) and for a bad dbc, as crc_gen_galois_keys
 *   crc_galois_conjugate_keys_dev   the same on device blobs (16-byte aligned, disjoint)
 *   crc_galois_permute_ntt_dev  unit-test access to galois_permute_ntt_kernel: NTT-form d_in [rows][k][n] -> d_out = NTT(sigma_g(INTT(d_in))); disjoint, aligned
 *   crc_rotate_hoisted_forms    d_y [R][count] size-2 ciphertexts: d_y[r] = H_{gs[r]}(d_x), or d_x itself in out_form where gs[r] = 1.  Every gs[r] != 1 must have
 *                               its own CONJUGATED key in the set (d_cgk, elts): there is no chain of steps for an absent key.  A set of un-conjugated keys
 *                               passed by mistake cannot be told apart and gives ciphertexts that do not decrypt.  d_work: crc_rotate_hoisted_work_bytes(ctx,
 *                               count, R, dbc) -- bounded in count by internal passes, R prepared keys (each made once per call, not per pass)
 *   crc_diag_mac_forms          d_y [count] = Sum_r P_r (*) H_{gs[r]}(d_x) with NTT-form plaintext rows d_p_ntt [R][k][n] (crc_plain_to_ntt): bit for bit
 *                               crc_rotate_hoisted_forms, then crc_multiply_plain_ntt per element, then crc_add -- but the rotated ciphertexts are never
 *                               written (the gather is folded into the product).  With the slots of one image tiled with period M over both rows and the
 *                               diagonals of an M x M matrix as P_r, gs[r] = crc_galois_elt_rows(d_r), this is the matrix-vector product over slots.
 *                               d_work: crc_diag_mac_work_bytes(ctx, count, R, dbc).  d_p_ntt must not overlap d_y or d_work (CRC_ERR_INVALID_ARGUMENT)
 *   crc_diag_mac_bsgs_forms     baby-step / giant-step: d_y [count] = Sum_j H_{gg[j]}( Sum_b P[j][b] (*) H_{gb[b]}(d_x) ) with NTT-form plaintext rows d_p_ntt
 *                               [G][B][k][n].  Bit for bit: crc_diag_mac_forms(d_x, gb, B, P[j]) into NTT form for every j, crc_rotate_hoisted_forms of each result
 *                               by {gg[j]} into NTT form, crc_add over j, one inverse transform for CRC_COEFF -- but neither a rotated input nor a rotated inner
 *                               sum is ever written.  B + G key switches and conjugated keys (fewer where an element is 1) where the flat product of the same
 *                               B G terms takes B G.  With gb[b] = crc_galois_elt_rows(b), gg[j] = crc_galois_elt_rows(B j) and the rows of crc_bsgs_plan
 *                               (crcnn_amd/host/diag_plan.h) this is the M x M matrix-vector product over slots, M = B G.  G = 1 with gg = {1} is
 *                               crc_diag_mac_forms.  d_work: crc_diag_mac_bsgs_work_bytes(ctx, count, B, G, dbc); B, G <= 65536
 *   crc_conv_slots_forms        the packed convolution: d_x [Cin][count] -> d_y [Cout][count],  y[co] = Sum_ci Sum_tau w[.][co][ci][tau] H_{gs[tau]}(x[ci])  with
 *                               SCALAR weights d_w [k][Cout][Cin][T], one canonical residue per modulus (crc_conv_slots_pack_weights).  Bit for bit: for every
 *                               (co, ci) crc_diag_mac_forms(x[ci], gs, T, P[co][ci]) into NTT form, where P[co][ci][tau] is crc_plain_to_ntt of the constant
 *                               polynomial w mod t; crc_add over ci; one inverse transform for CRC_COEFF -- at every tuning setting and however the call groups
 *                               taps, channels and ciphertexts into launches and passes.  One digit decomposition per input ciphertext and one key switch per
 *                               (input ciphertext, tap with gs[tau] != 1) where the composition takes Cout of each; neither a rotated input nor a product is
 *                               written.  With one channel plane per ciphertext and the taps of crc_conv_slots_plan (crcnn_amd/host/diag_plan.h) this is a
 *                               'valid' convolution of a single packed image.  d_work: crc_conv_slots_work_bytes(ctx, count, Cin, Cout, T, dbc) (0 for bad
 *                               arguments); Cin, Cout <= 4096, T <= 1024
 *   crc_conv_slots_pack_weights host memory, any context: h_out [k][count] from count integers h_w (any int64, taken mod t): for c = w mod t in [0, t) the word
 *                               c >= (t + 1) / 2 ? c + q_i - t : c  (mod q_i) -- every position of the NTT-form row of the constant plaintext c
 *   crc_conv_slots_bias_mask_forms  crc_conv_slots_forms with an epilogue in the channel mix: d_bias [k][Cout] (crc_conv_slots_pack_bias) or NULL, d_mask_ntt [k][n]
 *                               (ONE NTT-form plaintext row, crc_plain_to_ntt -- of a 0/1 slot vector for zero padding, but any canonical residues) or NULL.
 *                               Bit for bit, in this order: crc_conv_slots_forms into NTT form; with d_bias, per output channel crc_add_plain (sign +1, group =
 *                               count) of the NTT-form delta row of the constant b[co]; with d_mask_ntt, crc_multiply_plain_ntt of all Cout count ciphertexts by
 *                               the row (group = Cout count); one inverse transform for CRC_COEFF -- at every tuning setting and pass structure.  Both NULL is
 *                               crc_conv_slots_forms itself.  The masked result never leaves the kernel unmasked: no read and write of the Cout count rows, no
 *                               further launch.  A result masked by the 0/1 vector of its valid slots decrypts to exactly 0 elsewhere, which is what a layer
 *                               with zero padding behind it needs (crc_conv_slots_plan_geom, crcnn_amd/host/diag_plan.h).  Work space and caps as
 *                               crc_conv_slots_forms; refused also for d_bias or d_mask_ntt misaligned or overlapping d_y, d_work or d_x
 *   crc_conv_slots_pack_bias    host memory, any context: h_out [k][count] from count integers h_b (any int64, taken mod t): for c = b mod t in [0, t) the word
 *                               floor(q / t) c + (c >= (t + 1) / 2 ? q mod t : 0)  (mod q_i) -- every position of crc_plain_to_delta(form = CRC_NTT) of the
 *                               constant plaintext c
 *   crc_galois_prepare_keys_dev prepared keys that outlive a call: d_pk [n_elts][crc_galois_prepared_key_words(ctx, dbc)] from the CONJUGATED keys d_cgk of elts --
 *                               per key exactly what every entry point above makes of it in pass 0 of every call (the fp64 key switch's form).  d_scratch:
 *                               crc_evk_words(ctx, dbc) words.  CRC_ERR_UNSUPPORTED (and 0 words) where the fp64 key switch does not take (parameters, dbc);
 *                               CRC_ERR_INVALID_ARGUMENT for null, misaligned or overlapping operands, an invalid element or g = 1
 *   crc_dense_planes_forms      the dense layer over channel planes: d_x [Cin][count] -> d_y [count],  y = Sum_j H_{gs[j]}( Sum_c P[j][c] (*) x[c] )  with NTT-form
 *                               plaintext rows d_p_ntt [R][Cin][k][n].  The OUTPUTS are rotated: R key switches (fewer where gs[j] = 1) whatever Cin is, the
 *                               keyed steps of a pass in one batched key switch with one key per step.  Bit for bit: per j crc_multiply_plain_ntt(x[c], P[j][c])
 *                               summed over c with crc_add, crc_rotate_hoisted_forms of the sum by {gs[j]} into NTT form, crc_add over j, one inverse transform
 *                               for CRC_COEFF -- at every tuning setting ("planes_batch": 0 default, 1 one key switch per step, 2 batched) and pass structure.
 *                               d_pk: NULL, or the prepared keys of (d_cgk, elts) from crc_galois_prepare_keys_dev -- then no key is prepared in the call where
 *                               the fp64 key switch runs.  With the rows of crc_dense_planes_fold (crcnn_amd/host/diag_plan.h) this is a dense layer on strided
 *                               slots of Cin planes; Cin = 1 is a dense layer on a vector at arbitrary slots.  d_work: crc_dense_planes_work_bytes(ctx, count,
 *                               Cin, R, dbc, prepared = d_pk != NULL) (0 for bad arguments); Cin <= 4096, R <= 65536.  The size for prepared = 1 is
 *                               SMALLER (one key slot instead of R), and the call derives its layout from d_pk, not from the buffer: a d_work sized with
 *                               prepared = 1 and then passed with d_pk = NULL is written past its end, undetected -- size it with the flag the call will
 *                               see, or with the larger of the two.  Of d_pk only the slots of the call's own elements gs are read, so the others need not
 *                               be prepared.  The key pointers of the batched path are written by a kernel from launch arguments: like its siblings the
 *                               call reads no host memory after it returns
 * Refusals as in the paragraph above (null / misaligned / overlapping operands, forms, dbc, an invalid element), plus R < 1 (B < 1, G < 1) and a missing
 * conjugated key; every entry point with a read-only operand (d_p_ntt, d_w) also where that is null, misaligned or overlaps d_y or d_work -- crc_diag_mac_forms
 * included; crc_conv_slots_forms also for Cin, Cout or T below 1 or above its caps: CRC_ERR_INVALID_ARGUMENT, nothing launched, d_y untouched.  count = 0 is CRC_OK.  crc_dense_planes_forms also for Cin or R outside their caps, d_p_ntt or d_pk
 * misaligned or overlapping d_x, d_y or d_work, and d_pk given with n_elts = 0 while a step is keyed.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_galois_ntt_table(const crc_ctx *ctx, uint64_t g, uint32_t *table /*[n]*/);
int crc_galois_conjugate_keys(const crc_ctx *ctx, const uint64_t *elts, int n_elts, int dbc, const uint64_t *h_gk, uint64_t *h_out);
int crc_galois_conjugate_keys_dev(crc_ctx *ctx, const uint64_t *elts, int n_elts, int dbc, const uint64_t *d_gk, uint64_t *d_out, void *stream);
int crc_galois_permute_ntt_dev(crc_ctx *ctx, const uint64_t *d_in, size_t rows, uint64_t g, uint64_t *d_out, void *stream);
size_t crc_rotate_hoisted_work_bytes(const crc_ctx *ctx, size_t count, int R, int dbc);
int crc_rotate_hoisted_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gs /*[R], host*/, int R, const uint64_t *d_cgk,
                             const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y /*[R][count]*/, int out_form, void *d_work, void *stream);
size_t crc_diag_mac_work_bytes(const crc_ctx *ctx, size_t count, int R, int dbc);
int crc_diag_mac_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gs /*[R], host*/, int R, const uint64_t *d_p_ntt /*[R][k][n]*/,
                       const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_y /*[count]*/, int out_form, void *d_work, void *stream);
size_t crc_diag_mac_bsgs_work_bytes(const crc_ctx *ctx, size_t count, int B, int G, int dbc);
int crc_diag_mac_bsgs_forms(crc_ctx *ctx, const uint64_t *d_x, int in_form, size_t count, const uint64_t *gb /*[B], host*/, int B, const uint64_t *gg /*[G], host*/,
                            int G, const uint64_t *d_p_ntt /*[G][B][k][n]*/, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc,
                            uint64_t *d_y /*[count]*/, int out_form, void *d_work, void *stream);
int crc_conv_slots_pack_weights(const crc_ctx *ctx, const int64_t *h_w, size_t count, uint64_t *h_out /*[k][count]*/);
size_t crc_conv_slots_work_bytes(const crc_ctx *ctx, size_t count, int Cin, int Cout, int T, int dbc);
int crc_conv_slots_forms(crc_ctx *ctx, const uint64_t *d_x /*[Cin][count]*/, int in_form, size_t count, int Cin, const uint64_t *gs /*[T], host*/, int T,
                         const uint64_t *d_w /*[k][Cout][Cin][T]*/, int Cout, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc,
                         uint64_t *d_y /*[Cout][count]*/, int out_form, void *d_work, void *stream);
int crc_conv_slots_pack_bias(const crc_ctx *ctx, const int64_t *h_b, size_t count, uint64_t *h_out /*[k][count]*/);
int crc_conv_slots_bias_mask_forms(crc_ctx *ctx, const uint64_t *d_x /*[Cin][count]*/, int in_form, size_t count, int Cin, const uint64_t *gs /*[T], host*/, int T,
                                   const uint64_t *d_w /*[k][Cout][Cin][T]*/, int Cout, const uint64_t *d_bias /*[k][Cout] or NULL*/,
                                   const uint64_t *d_mask_ntt /*[k][n] or NULL*/, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc,
                                   uint64_t *d_y /*[Cout][count]*/, int out_form, void *d_work, void *stream);
size_t crc_galois_prepared_key_words(const crc_ctx *ctx, int dbc);
int crc_galois_prepare_keys_dev(crc_ctx *ctx, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, int dbc, uint64_t *d_pk /*[n_elts][prepared_key_words]*/,
                                uint64_t *d_scratch /*[crc_evk_words]*/, void *stream);
size_t crc_dense_planes_work_bytes(const crc_ctx *ctx, size_t count, int Cin, int R, int dbc, int prepared);
int crc_dense_planes_forms(crc_ctx *ctx, const uint64_t *d_x /*[Cin][count]*/, int in_form, size_t count, int Cin, const uint64_t *gs /*[R], host*/, int R,
                           const uint64_t *d_p_ntt /*[R][Cin][k][n]*/, const uint64_t *d_cgk, const uint64_t *elts, int n_elts, const uint64_t *d_pk /*or NULL*/,
                           int dbc, uint64_t *d_y /*[count]*/, int out_form, void *d_work, void *stream);
/* FractionalEncoder::decode / encode (encoder.cpp:1226-1270, 1013-1076; 64 integer + 32 fractional coefficients, base 3: CrCNN/src/globals.cpp:52) on the
 * device: the doubles crc_decode returns for d_plain [count][n], and the dense plaintexts [count][n] crc_encode_f32 / _f64 make of the values -- the same IEEE
 * operations in the same order as the host encoder, contraction off. */
int crc_decode_dev(crc_ctx *ctx, const uint64_t *d_plain, size_t count, double *d_out, void *stream);
int crc_encode_dev_f32(crc_ctx *ctx, const float *d_values, size_t count, uint64_t *d_plain, void *stream);
int crc_encode_dev_f64(crc_ctx *ctx, const double *d_values, size_t count, uint64_t *d_plain, void *stream);
/* The client-side refresh of Network::forward (CrCNN/src/network.cpp:30-34: `floatCube image = decryptImage(input); input = encryptImage(image)`,
 * globals.cpp:207-230 and 144-157) for `count` ciphertexts at once, entirely on `stream`: decrypt -> decode -> float (globals.cpp:221 keeps floats) ->
 * encode -> Encryptor::encrypt with fresh randomness (seed / key + stream_base as crc_encrypt_dev[_key]_forms).  in_form / out_form: CRC_COEFF or CRC_NTT.
 * d_values_out (may be NULL): the `count` floats the client saw.  d_ct_out may be d_ct_in.  d_work: crc_refresh_dev_work_bytes(count, in_form). */
size_t crc_refresh_dev_work_bytes(const crc_ctx *ctx, size_t count, int in_form);
int crc_refresh_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t seed,
                    int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream);
int crc_refresh_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_pk, const uint64_t *d_ct_in, size_t count, int in_form,
                        const uint8_t *h_key, uint64_t stream_base, int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Encryption under the SECRET key (BFV "symmetric" encryption; later SEAL releases ship it as encrypt_symmetric, SEAL 2.3.1 and CrCNN do not): for a
 * plaintext m, the secret key s, a uniform in R_q and noise e
 *     c1 = a,    c0 = -(a s) + e + Delta m (+ q mod t on the upper half, as every encryptor here),
 * so that c0 + c1 s = Delta m + e: the fresh noise is e alone (a public-key ciphertext carries e1 + e2 s - e u).  Whoever holds s -- the client that encrypts
 * an image, the refresh of Network::forward -- needs no public key, and since the NTT is a bijection a is sampled directly as NTT-form residues A:
 *     c1_ntt = A,    c0_ntt = NTT(e + Delta m) - A . s_ntt        one forward transform per modulus where Encryptor::encrypt runs three.
 * THE NTT-FORM RESULT IS THE DEFINITION; out_form CRC_COEFF is crc_ntt_inv of it, so the ciphertexts are a function of (key / seed, stream_base) alone,
 * whatever the form.  It is a different ciphertext distribution than Encryptor::encrypt's and OPT-IN everywhere: crc_encrypt*, crc_refresh_dev* and the
 * host classes' defaults are what they were.
 *
 * Sampling: ChaCha20, domain CHACHA_DOM_ENC_SYM = 5 (a public-key and a secret-key encryption under the same (key, stream_base) never share a keystream),
 * one stream per (ciphertext, coefficient pair): nonce = (stream id low, stream id high, 5 << 24 | s), s the even coefficient index, stream id = stream_base +
 * ciphertext index; block counter 0, 1, ... .  With w[16 b + j] = word j of block b:
 *   w[0..1] / w[2..3]   64-bit word (low, high half) of the noise magnitude of coefficient s / s + 1: |e| = the number of the 19 thresholds of
 *                       crc_encrypt_dev_noise_thresholds the word reaches (0..19; the clipped, truncated normal of the reference's encryptor)
 *   w[4]                bit 0 / bit 1 set: e of coefficient s / s + 1 is negative.   w[5..7] unused
 *   w[8 + 8 i + 4 c .. 11 + 8 i + 4 c]   z = w[+0] + 2^32 w[+1] + 2^64 w[+2] + 2^96 w[+3];  A[i][s + c] = z mod q_i   (c = 0, 1; modulus index i)
 * A 128-bit integer reduced modulo q_i < 2^62 is within q_i / 2^128 < 2^-66 statistical distance of uniform on [0, q_i); no rejection, no loop: k / 2 + 1
 * blocks per coefficient pair (one at k = 1, two at k = 2 and 3).  crc_encrypt_sym[_key] (host, any context) and crc_encrypt_sym_dev[_key]_forms follow this
 * layout bit for bit: the same (key / seed, stream_base, plaintexts) give the same ciphertexts on the host and on the device.
 *
 * SECURITY: as for every *_key entry point, NEVER encrypt two different batches under the same (key, stream_base) -- here a reused stream repeats a AND e and
 * the difference of the two c0 is Delta (m - m').  The uint64 seed variants expand a PUBLIC seed: tests, bench and goldens only; anyone who knows the seed
 * recomputes a and e, hence m.  A secret-key ciphertext is decrypted, evaluated on and measured exactly like a public-key one.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_encrypt_sym_key(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_plain /*[count][n]*/, size_t count, const uint8_t *h_key,
                        uint64_t stream_base, int out_form, uint64_t *h_ct /*[count][2][k][n]*/);
int crc_encrypt_sym(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_plain, size_t count, uint64_t seed, int out_form, uint64_t *h_ct);
/* the same on the device: d_sk_ntt [k][n] (the secret key of crc_keygen, NTT form), d_plain [count][n] dense plaintexts, d_ct [count][2][k][n] in out_form.
 * A sampling kernel writes e + Delta m and A; the transform of the c0 rows subtracts A . s in its last loop where the ring has the wave-local row transform
 * (n = 2048 .. 16384 with 45- to 57-bit moduli), else a slot-wise pass follows.  d_work: crc_encrypt_sym_dev_work_bytes(count).  Asynchronous on `stream`. */
size_t crc_encrypt_sym_dev_work_bytes(const crc_ctx *ctx, size_t count);
int crc_encrypt_sym_dev_key_forms(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_plain, size_t count, const uint8_t *h_key, uint64_t stream_base,
                                  int out_form, uint64_t *d_ct, void *d_work, void *stream);
int crc_encrypt_sym_dev_forms(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_plain, size_t count, uint64_t seed, int out_form, uint64_t *d_ct,
                              void *d_work, void *stream);
/* crc_refresh_dev[_key] with the re-encryption under the secret key the refresh holds anyway (no d_pk): the same decrypt -> decode -> float -> encode front end
 * and the same d_values_out, then the encryption above.  d_ct_out may be d_ct_in.  d_work: crc_refresh_sym_dev_work_bytes(count, in_form). */
size_t crc_refresh_sym_dev_work_bytes(const crc_ctx *ctx, size_t count, int in_form);
int crc_refresh_sym_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t count, int in_form, uint64_t seed, int out_form,
                        uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream);
int crc_refresh_sym_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct_in, size_t count, int in_form, const uint8_t *h_key,
                            uint64_t stream_base, int out_form, uint64_t *d_ct_out, float *d_values_out, void *d_work, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * SEEDED secret-key ciphertexts.  c1 = A of the encryption above is a pure function of a keystream and carries no information about the plaintext, so a client
 * may ship the c0 rows and a 32-byte PUBLIC seed and let the server regenerate c1 (later SEAL releases save symmetric ciphertexts this way; SEAL 2.3.1 has no
 * such form): half the bytes per ciphertext.  A seeded batch is `count` ciphertexts held as
 *     c0 [count][k][n] uint64, NTT FORM (the definition of a secret-key ciphertext here),  a PUBLIC 32-byte seed,  a 64-bit stream_base;
 * expansion gives the ordinary [count][2][k][n] ciphertexts, c1[m][i][s] = A(seed, stream_base + m, i, s), in CRC_NTT or (both polynomials inverse-transformed)
 * CRC_COEFF, and from there on nothing knows the difference: they are decrypted, evaluated on, refreshed and budget-measured like any other ciphertext.
 *
 * Two INDEPENDENT keystreams (the encryptor above draws e and A from one key, which therefore can never be published):
 *   mask,  PUBLIC seed,  domain CHACHA_DOM_SEEDED_A = 6: one stream per (ciphertext, coefficient pair), nonce = (stream id low, stream id high, 6 << 24 | s), s the
 *          even slot index, stream id = stream_base + ciphertext index.  Block j (counter j) serves modulus 2j with its words 0..7 and modulus 2j + 1 with its
 *          words 8..15; within a half, words 4c .. 4c + 3 are z = w[+0] + 2^32 w[+1] + 2^64 w[+2] + 2^96 w[+3] and A[i][s + c] = z mod q_i (c = 0, 1):
 *          (k + 1) / 2 blocks per pair, none of whose words depends on anything secret; within q_i / 2^128 < 2^-66 of uniform, as above.
 *   noise, PRIVATE key,  domain CHACHA_DOM_SEEDED_E = 7: one block (counter 0) per (ciphertext, coefficient pair), nonce = (stream id low, stream id high,
 *          7 << 24 | s); words 0..4 as block 0 of domain 5 (w[0..1] / w[2..3] the magnitude words of coefficients s / s + 1 through the thresholds of
 *          crc_encrypt_dev_noise_thresholds, w[4] bit 0 / bit 1 their signs).  A domain of its own ON PURPOSE: were it domain 5, one private key serving
 *          crc_encrypt_sym_key and this encryptor at the same stream_base would give equal e under different, known A, and for equal plaintexts
 *          c0 - c0' = -(A - A') s -- the secret key.  With its own domain, reusing a private key across the two encryptors is harmless.
 *
 * SECURITY: as above, never encrypt two batches under the same (private key, stream_base).  NEVER encrypt two batches under the same (public seed, stream_base)
 * either: equal A, so c0 - c0' = Delta (m - m') + e - e'.  The public seed MUST NOT be the private key: crc_encrypt_sym_seeded_key refuses byte-equal arguments
 * with CRC_ERR_INVALID_ARGUMENT.  crc_encrypt_sym_seeded expands a PUBLIC 64-bit seed (tests, bench; deterministic, NOT secure): private key = the expansion of
 * `seed` that every seed variant uses, public seed = crc_seeded_public_seed(seed) = the same expansion of ~seed, stream_base = 0.
 *
 *   crc_encrypt_sym_seeded[_key]   on the host, any context (device = -1 included), spread over the host threads like crc_encrypt_sym
 *   crc_seeded_expand              the host twin of the kernel (any context): it pins the device's bits
 *   crc_seeded_expand_dev          d_c0 packed [count][k][n] -> d_ct [count][2][k][n]; asynchronous on `stream`, no work buffer (the CRC_COEFF result is the
 *                                  in-place inverse transform of the CRC_NTT one).  count == 0 is CRC_OK and writes nothing; the two ranges must not overlap and
 *                                  must be 16-byte aligned
 *   crc_encrypt_sym_seeded_dev[_key]   the encryptor on the device (a client-side GPU): d_sk_ntt [k][n], d_plain [count][n] dense plaintexts -> d_c0 packed
 *                                  [count][k][n], NTT form, bit for bit what crc_encrypt_sym_seeded[_key] computes for the same (secret key, plaintexts, private
 *                                  key, public seed, stream_base).  Three steps on `stream`, the rows formed in place: a sampling kernel writes e + Delta m into
 *                                  the packed rows, the forward row transform runs over them, a mask kernel regenerates A pair by pair in registers and
 *                                  subtracts A . s.  No c1 row is ever written and there is no work buffer.  The uint64-seed variant derives what
 *                                  crc_encrypt_sym_seeded derives (private key = the expansion of seed, public seed = crc_seeded_public_seed(seed), stream_base
 *                                  0); the _key variant refuses a public seed byte-equal to the private key.  NULL arguments, a source or key that overlaps
 *                                  d_c0 and device pointers that are not 16-byte aligned are refused (CRC_ERR_INVALID_ARGUMENT) and nothing is written;
 *                                  count == 0 is CRC_OK and writes nothing.  Asynchronous on `stream`
 *   crc_encrypt_f32_seeded_dev[_key]   pixels in, packed rows out: d_values [count] floats on the device -> FractionalEncoder::encode (the device encoder that
 *                                  crc_encode_dev_f32 runs, written in the compact 96-word form: the words of crc_encode_f32_compact) -> the encryptor above
 *                                  reading the compact plaintexts: 4 bytes per pixel go up instead of 8 n.  d_work: crc_encrypt_f32_seeded_dev_work_bytes(count)
 *                                  (the compact plaintexts), which must not overlap d_values either.  Refuses a ring with n <= CRC_PLAIN_COMPACT_WORDS (count == 0 is CRC_OK there too); otherwise as above
 *   crc_seeded_ct_bytes / _save / _load   the container: 96 header bytes -- magic "CRCSEED\0", uint32 version 1, uint32 0, crc_params_hash (32), uint64 count,
 *                                  uint64 stream_base, the seed (32) -- then the c0 rows, count * k * n uint64, all little-endian.  _load refuses a wrong magic /
 *                                  version / hash, a short buffer and a count that does not match the byte length, and then writes nothing; with h_c0 = NULL it
 *                                  only validates and reports *count (to size the rows)
 * ------------------------------------------------------------------------------------------------------------- */
int crc_seeded_public_seed(uint64_t seed, uint8_t *h_seed /*[CRC_KEY_BYTES]*/);
int crc_encrypt_sym_seeded_key(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_plain /*[count][n]*/, size_t count, const uint8_t *h_key /*PRIVATE*/,
                               const uint8_t *h_seed /*PUBLIC, CRC_KEY_BYTES*/, uint64_t stream_base, uint64_t *h_c0 /*[count][k][n], NTT form*/);
int crc_encrypt_sym_seeded(const crc_ctx *ctx, const uint64_t *h_sk_ntt, const uint64_t *h_plain, size_t count, uint64_t seed, uint64_t *h_c0);
int crc_seeded_expand(const crc_ctx *ctx, const uint64_t *h_c0, size_t count, const uint8_t *h_seed, uint64_t stream_base, int out_form,
                      uint64_t *h_ct /*[count][2][k][n]*/);
int crc_seeded_expand_dev(crc_ctx *ctx, const uint64_t *d_c0, size_t count, const uint8_t *h_seed, uint64_t stream_base, int out_form, uint64_t *d_ct,
                          void *stream);
int crc_encrypt_sym_seeded_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_plain /*[count][n]*/, size_t count, const uint8_t *h_key /*PRIVATE*/,
                                   const uint8_t *h_seed /*PUBLIC*/, uint64_t stream_base, uint64_t *d_c0 /*[count][k][n], NTT form*/, void *stream);
int crc_encrypt_sym_seeded_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_plain, size_t count, uint64_t seed, uint64_t *d_c0, void *stream);
size_t crc_encrypt_f32_seeded_dev_work_bytes(const crc_ctx *ctx, size_t count);
int crc_encrypt_f32_seeded_dev_key(crc_ctx *ctx, const uint64_t *d_sk_ntt, const float *d_values /*[count]*/, size_t count, const uint8_t *h_key /*PRIVATE*/,
                                   const uint8_t *h_seed /*PUBLIC*/, uint64_t stream_base, uint64_t *d_c0, void *d_work, void *stream);
int crc_encrypt_f32_seeded_dev(crc_ctx *ctx, const uint64_t *d_sk_ntt, const float *d_values, size_t count, uint64_t seed, uint64_t *d_c0, void *d_work,
                               void *stream);
size_t crc_seeded_ct_bytes(const crc_ctx *ctx, size_t count);
int crc_seeded_ct_save(const crc_ctx *ctx, const uint64_t *h_c0, size_t count, const uint8_t *h_seed, uint64_t stream_base, void *buf, size_t cap, size_t *written);
int crc_seeded_ct_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_c0, size_t max_count, size_t *count, uint8_t *h_seed,
                       uint64_t *stream_base);

/* ---------------------------------------------------------------------------------------------------------------
 * SEEDED key-switching keys: evaluation and Galois keys in half the bytes, made on the host or on the device.  A key blob (crc_evk_words) is a list of pairs
 * (first, second) with second = A uniform, so -- as for a seeded ciphertext -- A is a function of a PUBLIC seed and only the first rows travel.
 *
 *   key id     0 for the evaluation key (target w = s^2), or a valid Galois element g (target w = sigma_g(s)); no valid element is even, so 0 is free
 *   pairs      numbered in the blob's own order, p = Sum_{l' < l} L_l' + d for modulus l and digit d; P = Sum_l L_l = crc_evk_words / (2 k n)
 *   one key    its P first polynomials [P][k][n], NTT form: crc_seeded_key_words = P k n words, exactly half the blob
 *   a key set  ids [n_ids], dbc, a 32-byte PUBLIC seed, the rows [n_ids][P][k][n]
 * An EXPANDED seeded key IS an ordinary blob: every consumer (crc_relinearize*, crc_apply_galois_forms, crc_rotate_hoisted_forms, crc_diag_mac*, crc_conv_slots*,
 * crc_dense_planes_forms, crc_galois_prepare_keys_dev) takes it unchanged.  The keys differ from those of crc_gen_evk* / crc_gen_galois_keys* (other
 * keystreams); they decrypt the same.
 *
 * Keystreams, one per (id, pair, even slot s), nonce = (id, p | dbc << 16 | k << 24, domain << 24 | s):
 *   mask,  PUBLIC seed,  domain CHACHA_DOM_KSK_A = 9: blocks and words exactly as domain 6 -- block j serves modulus 2j with its words 0..7 and modulus 2j + 1
 *          with its words 8..15; the 128-bit z of words 4c .. 4c + 3 gives second[i][s + c] = z mod q_i
 *   noise, PRIVATE key,  domain CHACHA_DOM_KSK_E = 10: one block (counter 0), words 0..4 as block 0 of domain 5 (two magnitude words against the 19 thresholds
 *          of crc_encrypt_dev_noise_thresholds, sign bits in w[4]); e is a coefficient-form polynomial, the same integer under every modulus
 * Definition (NTT form, pointwise):  first[j] = -(A[j] s[j] + NTT_j(e)) + [j == l] factor_{l,d} w[j],  factor_{l,d} = (q / q_l) 2^(dbc d) mod q_l,
 * w = s^2 for id 0 and w[j][i] = s[j][pi_g(i)] for an element (pi_g: crc_galois_ntt_table(g); no inverse transform of s is needed).
 *
 * SECURITY.  Two domains and two keys for the reason given for domains 6 / 7.  dbc and k are part of the nonce because the streams are counter-based: without
 * them one private key serving the same id at two digit widths, or on a context and on a prefix of its moduli (crc_mod_switch_*), would give equal A and equal e
 * around DIFFERENT known factors, and first - first' = (factor - factor') sigma_g(s) would reveal the secret key.  Never generate the same id twice under one
 * (private key, dbc, k) with different public seeds or secret keys.  (The host classes keep this by taking the public seed from the private master key itself: bytes 0..31 of
 * block 0 of its stream nonce = (0, 0, CHACHA_DOM_KSK_SEED = 11 << 24), a PRF output that may be published -- an element generated again is the same key.)  The _key variants refuse a public seed byte-equal to the private key.  The uint64-seed
 * variants (tests, bench; deterministic, NOT secure) derive private key = the expansion of `seed`, public seed = crc_seeded_public_seed(seed).
 *
 *   crc_seeded_key_words           P k n; 0 for a bad dbc
 *   crc_gen_keys_seeded[_key]      on the host, any context, spread over the host threads by id: h_first [n_ids][P][k][n]
 *   crc_seeded_keys_expand         on the host: h_first -> h_out [n_ids][crc_evk_words].  conjugate = 0: the blobs K; conjugate = 1: K' =
 *                                  crc_galois_conjugate_keys of them, bit for bit (ids 0 and 1 are refused: they have no conjugated key)
 *   crc_gen_keys_seeded_dev[_key]  d_sk_ntt [k][n] -> d_first, bit for bit the host rows.  Three steps on `stream`, in place, no work buffer: a sample kernel
 *                                  writes e, the forward row transform runs over the n_ids P rows, a finish kernel regenerates A in registers, gathers the target
 *                                  from the secret key's rows and stores first.  `ids` is a HOST array
 *   crc_seeded_keys_expand_dev     d_first -> d_out blobs; one kernel copies the first rows and generates the second rows; with conjugate = 1 the same
 *                                  kernel stores every residue at its conjugated place (equal to crc_seeded_keys_expand_dev + crc_galois_conjugate_keys_dev,
 *                                  without the second buffer)
 *   crc_seeded_keys_bytes / _save / _load   the container: 88 header bytes -- magic "CRCSKEY\0", uint32 version 1, uint32 dbc, crc_params_hash (32), uint64
 *                                  n_ids, the seed (32) -- then the ids (n_ids uint64) and the rows (n_ids P k n uint64), little-endian: half the blobs' bytes
 *                                  plus 88 + 8 n_ids.  _load refuses a wrong magic / version / hash / dbc / id, a short buffer and a count that does not match
 *                                  the byte length, and then writes nothing; with h_first = NULL it only validates and reports *n_ids and *dbc
 * Refusals (CRC_ERR_INVALID_ARGUMENT, nothing written, nothing launched): a host-only context for the _dev calls, NULL or (device) not 16-byte aligned
 * pointers, d_first overlapping d_sk_ntt or d_out, an id that is neither 0 nor a valid element, dbc outside 1..60, a launch grid over 2^31 - 1.  n_ids = 0 is
 * CRC_OK and writes nothing.
 * ------------------------------------------------------------------------------------------------------------- */
size_t crc_seeded_key_words(const crc_ctx *ctx, int dbc);
int crc_gen_keys_seeded_key(const crc_ctx *ctx, const uint8_t *h_key /*PRIVATE*/, const uint8_t *h_seed /*PUBLIC*/, const uint64_t *h_sk_ntt, int dbc,
                            const uint64_t *ids, int n_ids, uint64_t *h_first /*[n_ids][P][k][n]*/);
int crc_gen_keys_seeded(const crc_ctx *ctx, uint64_t seed, const uint64_t *h_sk_ntt, int dbc, const uint64_t *ids, int n_ids, uint64_t *h_first);
int crc_seeded_keys_expand(const crc_ctx *ctx, const uint64_t *h_first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *h_seed, int conjugate,
                           uint64_t *h_out /*[n_ids][crc_evk_words]*/);
int crc_gen_keys_seeded_dev_key(crc_ctx *ctx, const uint8_t *h_key /*PRIVATE*/, const uint8_t *h_seed /*PUBLIC*/, const uint64_t *d_sk_ntt, int dbc,
                                const uint64_t *ids /*host*/, int n_ids, uint64_t *d_first, void *stream);
int crc_gen_keys_seeded_dev(crc_ctx *ctx, uint64_t seed, const uint64_t *d_sk_ntt, int dbc, const uint64_t *ids /*host*/, int n_ids, uint64_t *d_first,
                            void *stream);
int crc_seeded_keys_expand_dev(crc_ctx *ctx, const uint64_t *d_first, const uint64_t *ids /*host*/, int n_ids, int dbc, const uint8_t *h_seed, int conjugate,
                               uint64_t *d_out, void *stream);
size_t crc_seeded_keys_bytes(const crc_ctx *ctx, int dbc, int n_ids);
int crc_seeded_keys_save(const crc_ctx *ctx, const uint64_t *h_first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *h_seed, void *buf, size_t cap,
                         size_t *written);
int crc_seeded_keys_load(const crc_ctx *ctx, const void *buf, size_t bytes, uint64_t *h_first, uint64_t *ids, int max_ids, int *n_ids, int *dbc,
                         uint8_t *h_seed);

/* ---------------------------------------------------------------------------------------------------------------
 * Modulus switching: a ciphertext tensor continues over fewer coefficient moduli (SEAL 2.3.1 has no such operation; later SEALs call it
 * mod_switch_to_next).  `from` has the moduli q_0 .. q_{k-1}, `to` the first k' < k of them (d = k - k' are dropped), the same n and t.
 *
 * Definition.  For every coefficient c in [0, q_from) of every polynomial of a ciphertext (CRT-composed from its residues), in integers:
 *      for p in (q_{k-1}, q_{k-2}, ..., q_{k'}):   h = p >> 1;   c = (c + h) / p   (rounded down)
 *      result = c mod q_to
 * In residues: r_1 = ((c_{k-1} + h) mod p_1) - h is the centred remainder of the last row, every row i below it becomes (c_i - r_1) p_1^-1 mod q_i, r_2 is
 * taken from row k-2 the same way, and so on; a kept row takes c'_i = (c_i - R) (p_1 .. p_d)^-1 mod q_i with R = r_1 + p_1 r_2 + p_1 p_2 r_3 + ...
 *
 * Noise (size-2 ciphertexts, ternary secret key): c' = c / P + delta with |delta| < (1 + 1/p) / 2 per coefficient, so the invariant noise grows by at most
 * t (n + 1) / q_to: a ciphertext with a budget of b bits under `from` has at least floor(-log2(2^-b + t (n + 1) / q_to)) bits under `to` (less up to 2 bits for
 * the two bit-count floors of the budget measurement).  The plaintext does not change.
 *
 * What carries over to `to`: the per-modulus tables are those of `from` (same primes, same minimal roots), so the rows [0, k') of an NTT-form secret key
 * ([k][n]), of each public-key polynomial ([2][k][n]) and of an NTT-form plaintext row are valid there as they stand.  Evaluation keys and Galois keys do NOT
 * carry over (they hold (q / q_i) factors): generate them on `to` with crc_gen_evk* / crc_gen_galois_keys* from the prefix secret-key rows -- or, without the
 * secret key, make `to` with crc_ctx_create_level and restrict the keys of `from` (below: "Key-switching keys for a lower level").
 *
 *   crc_mod_switch_supported   1 if `to` is a proper prefix of `from` (1 <= k' < k, the same moduli in the same order, the same n and t), else 0
 *   crc_mod_switch_forms       d_in [count][size][k][n] of `from` in in_form -> d_out [count][size][k'][n] of `to` in out_form; size 2 or 3; forms CRC_COEFF or
 *                              CRC_NTT on either side.  Asynchronous on `stream`, on `from`'s device.  COEFF -> COEFF is one elementwise kernel; NTT -> NTT
 *                              inverse-transforms only the d dropped rows and forward-transforms R mod q_i per kept row (d + k' transforms per polynomial, the
 *                              kept rows never leave NTT form); COEFF -> NTT costs k' forward, NTT -> COEFF k inverse transforms.  Every form pair gives the
 *                              bits of the definition on coefficient form with crc_ntt_inv in front / crc_ntt_fwd (on `to`) behind.
 *                              d_work: crc_mod_switch_work_bytes(from, to, count, size, in_form, out_form).  n <= 16384 where a side is CRC_NTT
 *                              (CRC_ERR_UNSUPPORTED above).
 *   crc_mod_switch             the host twin: host memory, any contexts (device = -1 included), bit for bit the device call
 * CRC_ERR_INVALID_ARGUMENT, and nothing written, where crc_mod_switch_supported is 0, for a null or (device) not 16-byte aligned pointer, another form or
 * size, and a d_out or d_work that overlaps d_in (or each other); the work-bytes query gives 0 for whatever the call would refuse.  count = 0 is CRC_OK.
 * ------------------------------------------------------------------------------------------------------------- */
int    crc_mod_switch_supported(const crc_ctx *from, const crc_ctx *to);
size_t crc_mod_switch_work_bytes(const crc_ctx *from, const crc_ctx *to, size_t count, int size, int in_form, int out_form);
int    crc_mod_switch_forms(crc_ctx *from, const crc_ctx *to, const uint64_t *d_in, int in_form, size_t count, int size, uint64_t *d_out, int out_form,
                            void *d_work, void *stream);
int    crc_mod_switch(const crc_ctx *from, const crc_ctx *to, const uint64_t *h_in, int in_form, size_t count, int size, uint64_t *h_out, int out_form);

/* ---------------------------------------------------------------------------------------------------------------
 * Noise flooding (smudging): sanitise a response before it leaves the server.  The noise of an evaluated ciphertext is a function of the model's weights, and
 * a client who holds the secret key can read it (crc_noise_budget).  The server therefore adds to every ciphertext of a response a fresh public-key
 * encryption of zero whose first error term is far wider than any noise the evaluation can have left.  Not in SEAL 2.3.1 nor in the reference: the
 * engine's own, like modulus switching.  Opt-in; nothing else changes.  The server's last step is: flood, crc_mod_switch_forms, send.
 *
 * Definition.  For a size-2 ciphertext (c0, c1) under the public key (p0, p1) and flood_bits = B:
 *      c0' = c0 + p0 u + e1,     c1' = c1 + p1 u + e2
 *   u   uniform ternary (the encryptor's law and decoding rule)
 *   e2  the encryptor's clipped normal (sigma 3.19 cut at 6 sigma, truncated: crc_encrypt_dev_noise_thresholds)
 *   e1  UNIFORM on the integers [-2^B, 2^B): x = B + 1 uniform bits, e1 = x - 2^B; its residues are taken from a 128-bit word in exact integer arithmetic
 * The samples are ChaCha20 under a domain of their own, one block per (ciphertext stream id, coefficient pair); csrc/chacha.h (CHACHA_DOM_FLOOD) has the word
 * layout, which is a contract between the device and the host twin.  Ciphertext m of a call has the stream id stream_base + m.
 *
 * Admission.  1 <= B <= 126 and t (2^B + 38 n) < q / 2 (crc_flood_supported): the flood adds w = e1 - e_pk u + e2 s to c0 + c1 s, |w| <= 2^B + 38 n per
 * coefficient under ternary u, s and errors in [-19, 19]; past the bound the flood alone could flip the plaintext.  The plaintext does not change.
 *
 * Noise.  The invariant noise grows by at most t (2^B + 38 n) / q: a ciphertext with b bits of budget keeps at least
 * floor(-log2(2^-b + t (2^B + 38 n) / q)) bits (crc_flood_budget_bound; less up to 2 bits for the bit-count floors of the budget measurement).
 *
 *   crc_flood_supported      1 where B is admitted on this context, else 0
 *   crc_flood_bits           pure arithmetic: the smallest B whose range 2^B exceeds, by lambda_bits, the largest noise |w| a ciphertext with
 *                            budget_bits_in bits of budget can carry: B = lambda_bits + max(0, bits(q) - budget_bits_in - bits(t)).  A negative status
 *                            (CRC_ERR_INVALID_ARGUMENT) where that B is not admitted or an argument is out of range (budget outside [0, bits(q)], lambda
 *                            outside [0, 126]).  A SERVER HAS NO SECRET KEY: it calls this with the budget it knows A PRIORI for its network (the plain-modulus
 *                            search's worst case), never a measured one -- a measured budget is itself a function of the weights and the input.
 *   crc_flood_budget_bound   the lower bound above as an integer (not below 0); a negative status for a B that is not admitted or a budget outside [0, bits(q)]
 *   crc_flood_dev_work_bytes the work space of the device call (0 for a form it refuses): 3 k n words per ciphertext
 *   crc_flood_dev_key        d_ct [count][2][k][n] in `form` CRC_COEFF or CRC_NTT, flooded IN PLACE and in that form; d_pk [2][k][n] (NTT form, as crc_keygen
 *                            makes it).  Asynchronous on `stream`.  An NTT-form tensor is never transformed back: the error rows are transformed forward and
 *                            join the tensor, with p u, in that transform's last loop (three forward transforms per modulus; the tensor is read once and
 *                            written once).  A coefficient-form tensor costs one forward and two inverse transforms per modulus.  n <= 16384
 *                            (CRC_ERR_UNSUPPORTED above).  h_key: 32 bytes of host memory.  A REUSED (key, stream_base + m) IS A BREAK: the same u, e1, e2
 *                            twice, so the difference of two floods is the difference of their inputs.  Callers advance stream_base by count per call.
 *   crc_flood_dev            the same under the expansion of a PUBLIC 64-bit seed, stream_base 0 (tests, benchmarks; deterministic, NOT secure)
 *   crc_flood_key, crc_flood the host twin: host memory, any context (device = -1 included); bit for bit the device call for the same (key, stream_base) / seed
 * Both forms of one tensor under one key give the same ciphertexts (crc_ntt_fwd of the coefficient-form result is the NTT-form result).
 * CRC_ERR_INVALID_ARGUMENT, nothing launched and the tensor untouched: a B that is not admitted, a null or (device) not 16-byte aligned pointer, a d_work or d_pk
 * that overlaps d_ct.  CRC_ERR_UNSUPPORTED for a form other than the two.  count == 0 is CRC_OK on any context the call could serve (a null context, a host-only
 * context for the _dev calls and a null h_key are still CRC_ERR_INVALID_ARGUMENT), whatever the other arguments.  No width is admitted on a context of more than
 * 8 coefficient moduli (the kernels' argument block holds 8): crc_flood_supported is 0 there, for the host twin too.
 * What flooding does not hide: the decrypted values themselves, which are the client's to see; and the bound is statistical in lambda_bits (2^-lambda).
 * ------------------------------------------------------------------------------------------------------------- */
int    crc_flood_supported(const crc_ctx *ctx, int flood_bits);
int    crc_flood_bits(const crc_ctx *ctx, int budget_bits_in, int lambda_bits);
int    crc_flood_budget_bound(const crc_ctx *ctx, int budget_bits_in, int flood_bits);
size_t crc_flood_dev_work_bytes(const crc_ctx *ctx, size_t count, int form);
int    crc_flood_dev_key(crc_ctx *ctx, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, const uint8_t *h_key, uint64_t stream_base,
                         void *d_work, void *stream);
int    crc_flood_dev(crc_ctx *ctx, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, uint64_t seed, void *d_work, void *stream);
int    crc_flood_key(const crc_ctx *ctx, const uint64_t *h_pk, uint64_t *h_ct, size_t count, int form, int flood_bits, const uint8_t *h_key,
                     uint64_t stream_base);
int    crc_flood(const crc_ctx *ctx, const uint64_t *h_pk, uint64_t *h_ct, size_t count, int form, int flood_bits, uint64_t seed);

/* ---------------------------------------------------------------------------------------------------------------
 * Key-switching keys for a lower level WITHOUT the secret key: the upper level's keys, which are public, become the level's keys.
 *
 * Pair p = (l, d) of a key blob over Q = q_0 .. q_{k-1} is  first = -(A s + e) + E w,  second = A,  E = (Q / q_l) 2^(dbc d) mod Q, which is non-zero in
 * residue row l alone.  With q_B = q_0 .. q_{k'-1} dividing Q the identity holds mod q_B as it stands: pairs with l >= k' hold E = 0 and drop out, the others are
 * the first P' = Sum_{l < k'} L_l pairs, and rows [0, k') of their polynomials are a valid key at the lower level -- for the gadget (Q / q_l) 2^(dbc d), not the
 * level's own (q_B / q_l) 2^(dbc d).  The key switch therefore cuts digit l from [c (Q / q_l)^-1]_{q_l}; nothing else in it changes, and the noise term
 * Sum digit e is that of a key generated at the level (same e, same digit width, P' pairs).
 *
 *   crc_ctx_create_level   a context over the first `kept` moduli of `parent` (1 <= kept < k, else CRC_ERR_PARAMETERS; same n and t) whose key-switching gadget is
 *                          the parent's; a level of a level keeps the top one.  Everything else (tables, BEHZ, decryption, budget) is what crc_ctx_create gives
 *                          for the prefix, so crc_mod_switch_supported(parent, level) holds as for a plain prefix context.  Every key switch on it
 *                          (crc_square_relin*, crc_relinearize*, the Galois entry points, hoisted forms included) takes keys RESTRICTED from the parent's
 *   crc_ctx_key_moduli     the modulus count of the context's gadget: k on a context of crc_ctx_create, the top ancestor's k on a level
 *   Key GENERATION is refused on a level with an inherited gadget: crc_gen_evk*, crc_gen_galois_keys* and crc_gen_keys_seeded* (host and device) return
 *   CRC_ERR_PARAMETERS and write nothing.  The stream names of the seeded keys carry k but not the gadget: two levels of equal k' under different parents would
 *   put equal A and equal e around different known factors, and the difference of the two keys is a multiple of the secret key.
 *
 *   crc_keys_restrict_supported   1 if `to` is a level of `from` for key material: the same n, the same gadget moduli, to's moduli a proper prefix of from's
 *   crc_keys_restrict_dev  d_keys [n_keys][crc_evk_words(from, dbc)] -> d_out [n_keys][crc_evk_words(to, dbc)]: word (key, pair p < P', polynomial, row j < k',
 *                          slot) goes to the same coordinates at to's strides.  One copy kernel on from's device, asynchronous on `stream`; evaluation keys,
 *                          Galois keys and conjugated blobs (crc_galois_conjugate_keys: the conjugation acts inside a row) alike
 *   crc_keys_restrict      the host twin (any contexts)
 *   crc_seeded_keys_expand_level[_dev]   from's seeded rows [n_ids][P][k][n] -> to's blobs [n_ids][crc_evk_words(to)], bit for bit crc_keys_restrict of
 *                          crc_seeded_keys_expand(from, ...); from's blobs are never written
 * CRC_ERR_INVALID_ARGUMENT, and nothing written, where crc_keys_restrict_supported is 0, for a bad dbc, a null or (device) not 16-byte aligned pointer and
 * where input and output overlap; n_keys = 0 is CRC_OK.
 * ------------------------------------------------------------------------------------------------------------- */
int crc_ctx_create_level(const crc_ctx *parent, int kept, int device, crc_ctx **out);
int crc_ctx_key_moduli(const crc_ctx *ctx);
int crc_keys_restrict_supported(const crc_ctx *from, const crc_ctx *to);
int crc_keys_restrict(const crc_ctx *from, const crc_ctx *to, const uint64_t *h_keys, int n_keys, int dbc, uint64_t *h_out);
int crc_keys_restrict_dev(crc_ctx *from, const crc_ctx *to, const uint64_t *d_keys, int n_keys, int dbc, uint64_t *d_out, void *stream);
int crc_seeded_keys_expand_level(const crc_ctx *from, const crc_ctx *to, const uint64_t *h_first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *h_seed,
                                 int conjugate, uint64_t *h_out);
int crc_seeded_keys_expand_level_dev(crc_ctx *from, const crc_ctx *to, const uint64_t *d_first, const uint64_t *ids /*host*/, int n_ids, int dbc,
                                     const uint8_t *h_seed, int conjugate, uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * multi-GPU (SURVEY 8e / 8b `crc_broadcast_weights`).  The reference has no analogue: its only parallelism is the
 * std::thread fan-out inside a layer (convolutionalLayer.cpp:177-191).  Here a batch of encrypted images shards over the
 * GPUs of a node with NO data-path collective; the ONE collective is the start-up broadcast of the encoded (NTT-form)
 * weights and evaluation keys from the rank that built them, over RCCL (ncclBroadcast; xGMI inside a node).
 *
 *   crc_comm_unique_id    the root makes the 128-byte rendezvous id and hands it to the other ranks out of band
 *                         (file, socket, MPI, torch.distributed ...)
 *   crc_comm_create       one communicator per (process, GPU): rank `rank` of `world` on the context's device
 *   crc_comm_create_all   single-process alternative: one communicator per context / device (ncclCommInitAll); use the
 *                         *_all broadcast below, or one host thread per communicator
 *   crc_broadcast_weights in-place broadcast of `words` uint64 from `root` in <= 1 GiB pieces on `stream` (asynchronous:
 *                         ordered with the kernels of that stream, no host sync)
 *   crc_comm_allgather_u64  small host-to-host all-gather (per-rank checksums, timings); synchronises `stream`
 *   crc_checksum64        position-sensitive checksum of a device buffer: h_out[0] = xor of all words, h_out[1] =
 *                         sum_i w_i * (2i+1) mod 2^64; synchronises `stream`.  Every rank checks what it received against the
 *                         root's pair.
 * Rehearsal on one GPU: RCCL refuses two ranks on the same device.  With CRC_COMM_TRANSPORT=shm in the environment crc_comm_unique_id makes a POSIX
 * shared-memory segment (an unguessable name, created exclusively, mode 0600) instead of an RCCL rendezvous, names it in the id, and the same calls stage their
 * bytes through it (hipMemcpy, a process-shared barrier): the multi-rank HOST code above this header runs unchanged with several processes on one device.
 * A transport for tests only; never the default.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct crc_comm crc_comm;
#define CRC_COMM_ID_BYTES 128
int  crc_comm_unique_id(uint8_t *h_id /*[CRC_COMM_ID_BYTES]*/);
int  crc_comm_create(crc_ctx *ctx, int world, int rank, const uint8_t *h_id, crc_comm **out);
int  crc_comm_create_all(crc_ctx *const *ctxs, int ndev, crc_comm **out /*[ndev]*/);
void crc_comm_destroy(crc_comm *comm);
int  crc_comm_rank(const crc_comm *comm);
int  crc_comm_world(const crc_comm *comm);
int  crc_last_comm_error(void);                        /* the ncclResult_t of the last failed RCCL call (CRC_ERR_COMM) */
int  crc_broadcast_weights(crc_comm *comm, uint64_t *d_w, size_t words, int root, void *stream);
int  crc_broadcast_weights_all(crc_comm *const *comms, int ndev, uint64_t *const *d_w, size_t words, int root, void *const *streams);
int  crc_comm_allgather_u64(crc_comm *comm, const uint64_t *h_in, size_t words, uint64_t *h_out /*[world][words]*/, void *stream);
int  crc_checksum64(crc_ctx *ctx, const uint64_t *d_words, size_t words, uint64_t *h_out /*[2]*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif
