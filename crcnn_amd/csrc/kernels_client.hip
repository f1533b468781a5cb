// kernels_client.hip -- BFV public-key encryption on gfx950 (the step in front of the evaluation path).
//
// Encryptor::encrypt (SEAL encryptor.cpp:71-134) per plaintext m:   u <- uniform {-1,0,1}^n,  e1, e2 <- clipped normal (sigma 3.19,
// cut at 6 sigma, truncated to an integer: util/globals.cpp:13-15, util/clipnormal.cpp),
//     c0 = pk0 * u + e1 + Delta*m (+ q mod t on the upper half, evaluator.cpp:1168-1191),   c1 = pk1 * u + e2.
// 784 of these per image dominate the client's latency in the reference (2.74 s/image); here the polynomial products are
// the row NTT of kernels.hip and the sampling is ChaCha20 in counter mode (chacha.h), one (ciphertext, coefficient) stream per lane.
// The reference draws from std::random_device, so there are no reference bits to match: the ciphertexts are checked by
// decrypting them (tests/test_gpu_ops.py) and by their noise budget against the CPU encryptor's.
#include "kernels.h"
#include "chacha.h"
#include "enc_sampler.h"
#include <cmath>

// One lane = one (ciphertext, coefficient PAIR): its own ChaCha20 stream, nonce = (ciphertext stream id, domain | even coefficient index), ONE block (round 5;
// one block per coefficient and two Box-Muller draws before -- sampling was 40 % of an encryption).  Per coefficient six words: 64 bits for the ternary sample
// (2-bit fields, rejecting 3: all 32 fields equal to 3 has probability 2^-64 and falls back to 0) and 64 bits for the magnitude of each noise term; the noise
// signs are bits of word 12.  The noise law, cdt_noise and ternary_field: enc_sampler.h.

// U: [count][k][n] ternary polynomial in RNS form (coefficient domain).  ROWS = false: E [count][2][n] signed noise bytes (the coefficient-form pipeline adds
// them after its inverse transforms); ROWS = true: the rows e1 + Delta m (+ q mod t on the upper half, evaluator.cpp:1168-1191) and e2 of every ciphertext, as
// residues in ct [count][2][k][n] -- what the NTT-form pipeline transforms next
// COMPACT: `plain` holds the 96-word compact plaintexts of the fractional encoder (crc_plain_expand's layout) instead of dense rows
template <bool ROWS, bool COMPACT = false>
__global__ void __launch_bounds__(256) enc_sample_kernel(u64 *U, signed char *E, u64 *ct, const u64 *plain, const ModParams *mods, int n, int k, ChaChaKey key,
                                                         u64 stream_base, EncCdt cdt, PlainParams pp)
{
    const int pairs = n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (pr >= pairs) return;
    const int s = 2 * pr;
    const u64 sid = stream_base + m;
    u32 b[16];
    chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), ((u32)CHACHA_DOM_ENC_DEV << 24) | (u32)s, b);
    u32 tv[2]; int e[2][2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const u32 *w = b + 6 * c;
        tv[c] = ternary_field(w[0], w[1]);
        e[c][0] = cdt_noise(w[2], w[3], (b[12] >> (2 * c)) & 1u, cdt);
        e[c][1] = cdt_noise(w[4], w[5], (b[12] >> (2 * c + 1)) & 1u, cdt);
    }
    for (int i = 0; i < k; i++) {
        const u64 qm1 = mods[i].q - 1;
        *reinterpret_cast<ulonglong2 *>(U + (m * k + i) * (size_t)n + s) = ulonglong2{tv[0] == 0 ? 0 : (tv[0] == 1 ? 1 : qm1), tv[1] == 0 ? 0 : (tv[1] == 1 ?
            1 : qm1)};
    }
    if (!ROWS) {
#pragma unroll
        for (int p = 0; p < 2; p++) *reinterpret_cast<char2 *>(E + (m * 2 + p) * (size_t)n + s) = char2{(signed char)e[0][p], (signed char)e[1][p]};
    } else {
        ulonglong2 pl = make_ulonglong2(0, 0);
        if (!COMPACT) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)n + s);
        else if (s < CRC_PLAIN_COMPACT_LOW) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + s);
        else if (s >= n - CRC_PLAIN_COMPACT_HIGH)
            pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + CRC_PLAIN_COMPACT_LOW + (s - (n - CRC_PLAIN_COMPACT_HIGH)));
        const u64 pc[2] = {pl.x, pl.y};
        for (int i = 0; i < k; i++) {
            const ModParams md = mods[i];
            u64 r[2][2];
#pragma unroll
            for (int c = 0; c < 2; c++) {
#pragma unroll
                for (int p = 0; p < 2; p++) r[c][p] = e[c][p] >= 0 ? (u64)e[c][p] : md.q - (u64)(-e[c][p]);
                u64 lo, hi; mul64wide(pp.delta[i], pc[c], lo, hi);
                if (pc[c] >= pp.threshold) { const u64 l2 = lo + pp.uhi[i]; hi += (l2 < lo); lo = l2; }
                r[c][0] = addmod(r[c][0], barrett128(lo, hi, md), md.q);
            }
#pragma unroll
            for (int p = 0; p < 2; p++) *reinterpret_cast<ulonglong2 *>(ct + ((m * 2 + p) * k + i) * (size_t)n + s) = ulonglong2{r[0][p], r[1][p]};
        }
    }
}

// NTT-form pipeline: ct[m][p][i][s] (= the transformed noise rows) += U_ntt[m][i][s] * pk[p][i][s]; two neighbouring slots per thread, both polys
__global__ void __launch_bounds__(256) enc_fma_kernel(const u64 *U, const u64 *pk, u64 *ct, const ModParams *mods, int n, int k)
{
    const size_t row = blockIdx.x;                // m*k + i
    const int i = (int)(row % k);
    const size_t m = row / k;
    const ModParams md = mods[i];
    const u64 *u = U + row * (size_t)n;
    for (int s = 2 * threadIdx.x; s < n; s += 2 * blockDim.x) {
        const ulonglong2 uv = *reinterpret_cast<const ulonglong2 *>(u + s);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(pk + ((size_t)p * k + i) * n + s);
            u64 *dst = ct + ((m * 2 + p) * k + i) * (size_t)n + s;
            const ulonglong2 cv = *reinterpret_cast<const ulonglong2 *>(dst);
            *reinterpret_cast<ulonglong2 *>(dst) = ulonglong2{addmod(cv.x, mulmod(uv.x, kv.x, md), md.q), addmod(cv.y, mulmod(uv.y, kv.y, md), md.q)};
        }
    }
}

// ct[m][p][i][s] = U_ntt[m][i][s] * pk[p][i][s]
__global__ void __launch_bounds__(256) enc_mulpk_kernel(const u64 *U, const u64 *pk, u64 *ct, const ModParams *mods, int n, int k)
{
    const size_t row = blockIdx.x;                // m*2k + p*k + i
    const int i = (int)(row % k), p = (int)((row / k) % 2);
    const size_t m = row / (2 * (size_t)k);
    const ModParams md = mods[i];
    const u64 *u = U + (m * k + i) * (size_t)n, *key = pk + ((size_t)p * k + i) * n;
    u64 *dst = ct + row * (size_t)n;
    for (int s = threadIdx.x; s < n; s += blockDim.x) dst[s] = mulmod(u[s], key[s], md);
}

// ct[m][p][i][s] += e_p[s]  (+ Delta*m[s] on poly 0)
__global__ void __launch_bounds__(256) enc_finish_kernel(u64 *ct, const signed char *E, const u64 *plain, const ModParams *mods, int n, int k, PlainParams pp)
{
    const size_t row = blockIdx.x;
    const int i = (int)(row % k), p = (int)((row / k) % 2);
    const size_t m = row / (2 * (size_t)k);
    const ModParams md = mods[i];
    const signed char *e = E + (m * 2 + p) * (size_t)n;
    const u64 *pl = plain + m * (size_t)n;
    u64 *dst = ct + row * (size_t)n;
    for (int s = threadIdx.x; s < n; s += blockDim.x) {
        const int ev = e[s];
        u64 v = addmod(dst[s], ev >= 0 ? (u64)ev : md.q - (u64)(-ev), md.q);
        if (p == 0) {
            const u64 c = pl[s];
            u64 lo, hi; mul64wide(pp.delta[i], c, lo, hi);
            if (c >= pp.threshold) { const u64 l2 = lo + pp.uhi[i]; hi += (l2 < lo); lo = l2; }
            v = addmod(v, barrett128(lo, hi, md), md.q);
        }
        dst[s] = v;
    }
}

size_t k_encrypt_work_words(const crc_ctx *c, size_t cnt)
{
    return cnt * (size_t)c->n * c->k + (cnt * 2 * (size_t)c->n + 7) / 8;       // U + E
}

// thresholds of the noise magnitude (enc_sample_kernel): P(|e| <= a) for the clipped, truncated normal of the reference, in long double (64-bit mantissa)
static const EncCdt &enc_cdt()
{
    static const EncCdt T = [] {
        EncCdt t{};
        const long double sigma = 3.19L, lim = 6.0L * sigma, r2 = sqrtl(2.0L) * sigma;
        const long double Z = erfl(lim / r2);                                  // P(|g| <= 6 sigma)
        for (int a = 0; a < 19; a++) {
            // P(|e| > a) = P(a + 1 <= |g| <= lim) / Z, from the complementary error function (no cancellation in the tail)
            const long double tail = (erfcl((long double)(a + 1) / r2) - erfcl(lim / r2)) / Z;
            t.t[a] = (u64)floorl((1.0L - tail) * 18446744073709551616.0L);
        }
        return t;
    }();
    return T;
}
void k_encrypt_cdt(u64 *out19) { const EncCdt &T = enc_cdt(); for (int a = 0; a < 19; a++) out19[a] = T.t[a]; }

int k_encrypt(crc_ctx *c, const u64 *pk, const u64 *plain, size_t cnt, const ChaChaKey &key, u64 stream_base, u64 *ct, u64 *work, hipStream_t st, bool out_ntt,
              bool plain_compact)
{
    if (cnt == 0) return CRC_OK;
    if (plain_compact && !out_ntt) return CRC_ERR_INVALID_ARGUMENT;       // (the coefficient-form pipeline adds Delta m from dense rows: expand first)
    const int n = c->n, k = c->k;
    u64 *U = work; signed char *E = reinterpret_cast<signed char *>(U + cnt * (size_t)n * k);
    const int pairs = n / 2, threads = pairs < 256 ? pairs : 256, pblocks = (pairs + threads - 1) / threads;
    if (cnt * (size_t)pblocks > 0x7fffffffULL || cnt * 2 * (size_t)k > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    int rc;
    if (out_ntt) {
        // c_p = NTT(e_p (+ Delta m)) + pk_p . NTT(u): three forward transforms per modulus and no inverse one -- the same residues as transforming the
        // coefficient form
        if (plain_compact)
            hipLaunchKernelGGL((enc_sample_kernel<true, true>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, U, E, ct, plain, c->d_mods, n, k, key,
                               stream_base, enc_cdt(), c->plain);
        else
            hipLaunchKernelGGL((enc_sample_kernel<true, false>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, U, E, ct, plain, c->d_mods, n, k, key,
                               stream_base, enc_cdt(), c->plain);
        HIPCHK(hipGetLastError());
        if ((rc = k_ntt_ct(c, false, U, U, cnt, 1, false, st, nullptr, 0, 0, 0))) return rc;
        // (the product joins in the transform's last loop where the ring has the wave-local kernel; else as a pass of its own)
        rc = k_ntt_ct_fwd_fma(c, ct, cnt, U, pk, st);
        if (rc != CRC_ERR_UNSUPPORTED) return rc;
        if ((rc = k_ntt_ct(c, false, ct, ct, cnt, 2, false, st, nullptr, 0, 0, 0))) return rc;
        hipLaunchKernelGGL(enc_fma_kernel, dim3((unsigned)(cnt * k)), dim3(n / 2 < 256 ? n / 2 : 256), 0, st, U, pk, ct, c->d_mods, n, k);
        HIPCHK(hipGetLastError());
        return CRC_OK;
    }
    hipLaunchKernelGGL((enc_sample_kernel<false, false>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, U, E, ct, plain, c->d_mods, n, k, key, stream_base,
        enc_cdt(),
                       c->plain);
    HIPCHK(hipGetLastError());
    if ((rc = k_ntt_ct(c, false, U, U, cnt, 1, false, st, nullptr, 0, 0, 0))) return rc;
    hipLaunchKernelGGL(enc_mulpk_kernel, dim3((unsigned)(cnt * 2 * k)), dim3(256), 0, st, U, pk, ct, c->d_mods, n, k);
    HIPCHK(hipGetLastError());
    if ((rc = k_ntt_ct(c, true, ct, ct, cnt, 2, false, st, nullptr, 0, 0, 0))) return rc;
    hipLaunchKernelGGL(enc_finish_kernel, dim3((unsigned)(cnt * 2 * k)), dim3(256), 0, st, ct, E, plain, c->d_mods, n, k, c->plain);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}

// ---- encryption under the secret key ---------------------------------------------------------------------------------------------------------------------------
// c1 = a uniform in R_q, c0 = -(a s) + e + Delta m: the client that holds s (the refresh of Network::forward, the encryption of an image) needs no public key,
// no ternary sample and one noise term.  The NTT is a bijection, so a is sampled directly as NTT-form residues A and the NTT-form ciphertext
//     c1 = A,   c0 = NTT(e + Delta m) - A . s
// costs one forward transform per modulus (the public-key encryptor: three).  That NTT form is the definition; the coefficient form is its inverse transform.
// Stream layout: chacha.h (CHACHA_DOM_ENC_SYM); crc_encrypt_sym on the host computes the same bits.

// One lane = one (ciphertext, coefficient pair), as enc_sample_kernel: ct [count][2][k][n] receives the residues of e + Delta m (+ q mod t on the upper half) in
// the c0 rows -- coefficient form, transformed next -- and the uniform residues A in the c1 rows -- NTT form, final.  COMPACT as enc_sample_kernel
template <bool COMPACT>
__global__ void __launch_bounds__(256) enc_sym_sample_kernel(u64 *ct, const u64 *plain, const ModParams *mods, int n, int k, ChaChaKey key, u64 stream_base,
                                                             EncCdt cdt, PlainParams pp)
{
    const int pairs = n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (pr >= pairs) return;
    const int s = 2 * pr;
    const u64 sid = stream_base + m;
    const u32 n2 = ((u32)CHACHA_DOM_ENC_SYM << 24) | (u32)s;
    u32 b[16];
    chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), n2, b);
    const int e[2] = {cdt_noise(b[0], b[1], b[4] & 1u, cdt), cdt_noise(b[2], b[3], (b[4] >> 1) & 1u, cdt)};
    ulonglong2 pl = make_ulonglong2(0, 0);
    if (!COMPACT) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)n + s);
    else if (s < CRC_PLAIN_COMPACT_LOW) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + s);
    else if (s >= n - CRC_PLAIN_COMPACT_HIGH)
        pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + CRC_PLAIN_COMPACT_LOW + (s - (n - CRC_PLAIN_COMPACT_HIGH)));
    const u64 pc[2] = {pl.x, pl.y};
    // one modulus: its two uniform residues from the eight keystream words w, e + Delta m beside them
    auto emit = [&](int i, const u32 *w) {
        const ModParams md = mods[i];
        u64 r[2], a[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            a[c] = mod128_any((u64)w[4 * c] | ((u64)w[4 * c + 1] << 32), (u64)w[4 * c + 2] | ((u64)w[4 * c + 3] << 32), md);
            u64 lo, hi; mul64wide(pp.delta[i], pc[c], lo, hi);
            if (pc[c] >= pp.threshold) { const u64 l2 = lo + pp.uhi[i]; hi += (l2 < lo); lo = l2; }
            r[c] = addmod(e[c] >= 0 ? (u64)e[c] : md.q - (u64)(-e[c]), barrett128(lo, hi, md), md.q);
        }
        *reinterpret_cast<ulonglong2 *>(ct + ((m * 2) * k + i) * (size_t)n + s) = ulonglong2{r[0], r[1]};
        *reinterpret_cast<ulonglong2 *>(ct + ((m * 2 + 1) * k + i) * (size_t)n + s) = ulonglong2{a[0], a[1]};
    };
    // block by block (the halves are picked with constant indices, so the block stays in registers): block j serves modulus 2j - 1 with its lower half and
    // modulus 2j with its upper half; block 0 is the one the noise came from
    emit(0, b + 8);
    for (int j = 1; 2 * j - 1 < k; j++) {
        chacha20_block(key, (u32)j, (u32)sid, (u32)(sid >> 32), n2, b);
        emit(2 * j - 1, b);
        if (2 * j < k) emit(2 * j, b + 8);
    }
}

// rings without the wave-local transform: ct[m][0][i][s] = V[m][i][s] - ct[m][1][i][s] * sk[i][s]   (V = NTT(e + Delta m), dense rows); two slots per thread
__global__ void __launch_bounds__(256) enc_sym_finish_kernel(const u64 *V, const u64 *sk, u64 *ct, const ModParams *mods, int n, int k)
{
    const size_t row = blockIdx.x;                // m*k + i
    const int i = (int)(row % k);
    const size_t m = row / k;
    const ModParams md = mods[i];
    const u64 *v = V + row * (size_t)n, *key = sk + (size_t)i * n, *c1 = ct + ((m * 2 + 1) * k + i) * (size_t)n;
    u64 *c0 = ct + ((m * 2) * k + i) * (size_t)n;
    for (int s = 2 * threadIdx.x; s < n; s += 2 * blockDim.x) {
        const ulonglong2 vv = *reinterpret_cast<const ulonglong2 *>(v + s), av = *reinterpret_cast<const ulonglong2 *>(c1 + s);
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(key + s);
        *reinterpret_cast<ulonglong2 *>(c0 + s) = ulonglong2{submod(vv.x, mulmod(av.x, kv.x, md), md.q), submod(vv.y, mulmod(av.y, kv.y, md), md.q)};
    }
}

size_t k_encrypt_sym_work_words(const crc_ctx *c, size_t cnt) { return cnt * (size_t)c->n * c->k; }      // V of the two-pass form

int k_encrypt_sym(crc_ctx *c, const u64 *sk, const u64 *plain, size_t cnt, const ChaChaKey &key, u64 stream_base, u64 *ct, u64 *work, hipStream_t st, bool out_ntt,
                  bool plain_compact)
{
    if (cnt == 0) return CRC_OK;
    const int n = c->n, k = c->k;
    if (plain_compact && n <= CRC_PLAIN_COMPACT_WORDS) return CRC_ERR_INVALID_ARGUMENT;
    const int pairs = n / 2, threads = pairs < 256 ? pairs : 256, pblocks = (pairs + threads - 1) / threads;
    if (cnt * (size_t)pblocks > 0x7fffffffULL || cnt * (size_t)k > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    if (plain_compact)
        hipLaunchKernelGGL((enc_sym_sample_kernel<true>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, ct, plain, c->d_mods, n, k, key, stream_base,
                           enc_cdt(), c->plain);
    else
        hipLaunchKernelGGL((enc_sym_sample_kernel<false>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, ct, plain, c->d_mods, n, k, key, stream_base,
                           enc_cdt(), c->plain);
    HIPCHK(hipGetLastError());
    // (the product joins in the transform's last loop where the ring has the wave-local kernel; else as a pass of its own)
    int rc = k_ntt_ct_fwd_negmul(c, ct, cnt, sk, st);
    if (rc == CRC_ERR_UNSUPPORTED) {
        if ((rc = k_ntt_ct_poly0(c, ct, work, cnt, st))) return rc;
        hipLaunchKernelGGL(enc_sym_finish_kernel, dim3((unsigned)(cnt * k)), dim3(n / 2 < 256 ? n / 2 : 256), 0, st, work, sk, ct, c->d_mods, n, k);
        HIPCHK(hipGetLastError());
    } else if (rc) return rc;
    return out_ntt ? CRC_OK : k_ntt_ct(c, true, ct, ct, cnt, 2, false, st, nullptr, 0, 0, 0);
}

// ---- seeded secret-key ciphertexts -----------------------------------------------------------------------------------------------------------------------------
// c1 = A of a secret-key ciphertext is a function of a PUBLIC seed alone (chacha.h, CHACHA_DOM_SEEDED_A), so a client ships the c0 rows and 32 bytes and the
// server regenerates c1 here: half the bytes over the link.  One lane = one (ciphertext, coefficient pair), as enc_sym_sample_kernel: per modulus it copies the
// pair's c0 residues from the packed rows [count][k][n] into the ciphertext [count][2][k][n] and stores the two residues of A beside them.  The keystream is
// walked block by block with constant indices into the block (it stays in registers): block j serves modulus 2j with its lower half, modulus 2j + 1 with its
// upper half.  crc_seeded_expand on the host computes the same bits.
__global__ void __launch_bounds__(256) seeded_expand_kernel(u64 *ct, const u64 *c0, const ModParams *mods, int n, int k, ChaChaKey seed, u64 stream_base)
{
    const int pairs = n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (pr >= pairs) return;
    const int s = 2 * pr;
    const u64 sid = stream_base + m;
    const u32 n2 = ((u32)CHACHA_DOM_SEEDED_A << 24) | (u32)s;
    u32 b[16];
    auto emit = [&](int i, const u32 *w) {
        const ModParams md = mods[i];
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(c0 + (m * k + i) * (size_t)n + s);
        u64 a[2];
#pragma unroll
        for (int c = 0; c < 2; c++) a[c] = mod128_any((u64)w[4 * c] | ((u64)w[4 * c + 1] << 32), (u64)w[4 * c + 2] | ((u64)w[4 * c + 3] << 32), md);
        *reinterpret_cast<ulonglong2 *>(ct + ((m * 2) * k + i) * (size_t)n + s) = v;
        *reinterpret_cast<ulonglong2 *>(ct + ((m * 2 + 1) * k + i) * (size_t)n + s) = ulonglong2{a[0], a[1]};
    };
    for (int j = 0; 2 * j < k; j++) {
        chacha20_block(seed, (u32)j, (u32)sid, (u32)(sid >> 32), n2, b);
        emit(2 * j, b);
        if (2 * j + 1 < k) emit(2 * j + 1, b + 8);
    }
}

int k_seeded_expand(crc_ctx *c, const u64 *c0, size_t cnt, const ChaChaKey &seed, u64 stream_base, u64 *ct, hipStream_t st, bool out_ntt)
{
    if (cnt == 0) return CRC_OK;
    const int n = c->n, k = c->k;
    const int pairs = n / 2, threads = pairs < 256 ? pairs : 256, pblocks = (pairs + threads - 1) / threads;
    if (cnt * (size_t)pblocks > 0x7fffffffULL || cnt * (size_t)k > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(seeded_expand_kernel, dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, ct, c0, c->d_mods, n, k, seed, stream_base);
    HIPCHK(hipGetLastError());
    // the NTT form is the definition; the coefficient form is the inverse transform of both polynomials, in place
    return out_ntt ? CRC_OK : k_ntt_ct(c, true, ct, ct, cnt, 2, false, st, nullptr, 0, 0, 0);
}

// ---- the seeded form produced on the device --------------------------------------------------------------------------------------------------------------------
// What crc_encrypt_sym_seeded[_key] computes on the host, bit for bit: the packed rows c0 [count][k][n] = NTT(e + Delta m) - A . s, with e from the PRIVATE key
// (CHACHA_DOM_SEEDED_E) and A from the PUBLIC seed (CHACHA_DOM_SEEDED_A).  Three steps on one stream and in place -- the sampler writes e + Delta m into the
// packed rows, the row transform runs over them as over a size-1 "ciphertext" (what the public-key encryptor does to its U rows), and the mask kernel
// regenerates A pair by pair in registers and subtracts A . s.  No c1 row is ever written: the server regenerates it (seeded_expand_kernel).

// One lane = one (ciphertext, coefficient pair), as enc_sym_sample_kernel: ONE block of the private key's noise stream, words 0..4; per modulus one 16-byte
// store of e + Delta m (+ q mod t on the upper half) into the packed row.  COMPACT as enc_sample_kernel
template <bool COMPACT>
__global__ void __launch_bounds__(256) seeded_enc_sample_kernel(u64 *c0, const u64 *plain, const ModParams *mods, int n, int k, ChaChaKey key, u64 stream_base,
                                                                EncCdt cdt, PlainParams pp)
{
    const int pairs = n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (pr >= pairs) return;
    const int s = 2 * pr;
    const u64 sid = stream_base + m;
    u32 b[16];
    chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), ((u32)CHACHA_DOM_SEEDED_E << 24) | (u32)s, b);
    const int e[2] = {cdt_noise(b[0], b[1], b[4] & 1u, cdt), cdt_noise(b[2], b[3], (b[4] >> 1) & 1u, cdt)};
    ulonglong2 pl = make_ulonglong2(0, 0);
    if (!COMPACT) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)n + s);
    else if (s < CRC_PLAIN_COMPACT_LOW) pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + s);
    else if (s >= n - CRC_PLAIN_COMPACT_HIGH)
        pl = *reinterpret_cast<const ulonglong2 *>(plain + m * (size_t)CRC_PLAIN_COMPACT_WORDS + CRC_PLAIN_COMPACT_LOW + (s - (n - CRC_PLAIN_COMPACT_HIGH)));
    const u64 pc[2] = {pl.x, pl.y};
    for (int i = 0; i < k; i++) {
        const ModParams md = mods[i];
        u64 r[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            u64 lo, hi; mul64wide(pp.delta[i], pc[c], lo, hi);
            if (pc[c] >= pp.threshold) { const u64 l2 = lo + pp.uhi[i]; hi += (l2 < lo); lo = l2; }
            r[c] = addmod(e[c] >= 0 ? (u64)e[c] : md.q - (u64)(-e[c]), barrett128(lo, hi, md), md.q);
        }
        *reinterpret_cast<ulonglong2 *>(c0 + (m * k + i) * (size_t)n + s) = ulonglong2{r[0], r[1]};
    }
}

// The same lanes over the TRANSFORMED packed rows: the public seed's keystream walked as seeded_expand_kernel walks it (block j: modulus 2j from words 0..7,
// modulus 2j + 1 from words 8..15, constant indices so the block stays in registers); per modulus one 16-byte load of the pair's c0 residues, one of the secret
// key's, c0 <- c0 - A . s, one 16-byte store in place.  A lives in registers only
__global__ void __launch_bounds__(256) seeded_enc_mask_kernel(u64 *c0, const u64 *sk, const ModParams *mods, int n, int k, ChaChaKey seed, u64 stream_base)
{
    const int pairs = n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const size_t m = blockIdx.x / pblocks;
    const int pr = (blockIdx.x % pblocks) * blockDim.x + threadIdx.x;
    if (pr >= pairs) return;
    const int s = 2 * pr;
    const u64 sid = stream_base + m;
    const u32 n2 = ((u32)CHACHA_DOM_SEEDED_A << 24) | (u32)s;
    u32 b[16];
    auto emit = [&](int i, const u32 *w) {
        const ModParams md = mods[i];
        u64 *dst = c0 + (m * k + i) * (size_t)n + s;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(dst), kv = *reinterpret_cast<const ulonglong2 *>(sk + (size_t)i * n + s);
        u64 a[2];
#pragma unroll
        for (int c = 0; c < 2; c++) a[c] = mod128_any((u64)w[4 * c] | ((u64)w[4 * c + 1] << 32), (u64)w[4 * c + 2] | ((u64)w[4 * c + 3] << 32), md);
        *reinterpret_cast<ulonglong2 *>(dst) = ulonglong2{submod(v.x, mulmod(a[0], kv.x, md), md.q), submod(v.y, mulmod(a[1], kv.y, md), md.q)};
    };
    for (int j = 0; 2 * j < k; j++) {
        chacha20_block(seed, (u32)j, (u32)sid, (u32)(sid >> 32), n2, b);
        emit(2 * j, b);
        if (2 * j + 1 < k) emit(2 * j + 1, b + 8);
    }
}

int k_encrypt_sym_seeded(crc_ctx *c, const u64 *sk, const u64 *plain, size_t cnt, const ChaChaKey &key, const ChaChaKey &seed, u64 stream_base, u64 *c0,
                         hipStream_t st, bool plain_compact)
{
    if (cnt == 0) return CRC_OK;
    const int n = c->n, k = c->k;
    if (plain_compact && n <= CRC_PLAIN_COMPACT_WORDS) return CRC_ERR_INVALID_ARGUMENT;
    const int pairs = n / 2, threads = pairs < 256 ? pairs : 256, pblocks = (pairs + threads - 1) / threads;
    if (cnt * (size_t)pblocks > 0x7fffffffULL || cnt * (size_t)k > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    if (plain_compact)
        hipLaunchKernelGGL((seeded_enc_sample_kernel<true>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, c0, plain, c->d_mods, n, k, key, stream_base,
                           enc_cdt(), c->plain);
    else
        hipLaunchKernelGGL((seeded_enc_sample_kernel<false>), dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, c0, plain, c->d_mods, n, k, key, stream_base,
                           enc_cdt(), c->plain);
    HIPCHK(hipGetLastError());
    // the packed rows are a size-1 "ciphertext" of k rows: transformed in place
    int rc;
    if ((rc = k_ntt_ct(c, false, c0, c0, cnt, 1, false, st, nullptr, 0, 0, 0))) return rc;
    hipLaunchKernelGGL(seeded_enc_mask_kernel, dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, c0, sk, c->d_mods, n, k, seed, stream_base);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
