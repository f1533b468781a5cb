// client.cpp -- client-side BFV on the host CPU: key generation, encryption, decryption, noise budget.
//
// Outside the accelerated path (needs the secret key) but part of what a CrCNN user calls around it:
// setParameters / encryptImage / decryptImage (CrCNN/src/globals.cpp:25-56,127-157,207-230) over SEAL's KeyGenerator
// (keygenerator.cpp:96-282), Encryptor (encryptor.cpp:71-134) and Decryptor (decryptor.cpp:107-236, BEHZ gamma rounding).
// Randomness: ChaCha20 keystreams (chacha.h) under a 256-bit key -- crc_random_key() draws it from the OS (getrandom(2)); the
// uint64 "seed" entry points expand a public seed and exist for tests / bench / goldens only.  SEAL draws from std::random_device,
// so the reference defines sampling laws, not bits.
#include "ctx.h"
#include "host_parallel.h"
#include "chacha.h"
#include <cmath>
#include <cstring>
#include <vector>
#include <cerrno>
#include <sys/random.h>

typedef unsigned __int128 u128;

namespace {
typedef ChaChaStream Rng;                                 // 64-bit words of a ChaCha20 keystream (chacha.h)
ChaChaKey load_key(const uint8_t *key) { return chacha_load_key(key); }
ChaChaKey seed_key(u64 seed) { return chacha_seed_key(seed); }

void ternary(const crc_ctx *c, Rng &r, u64 *p)            // uniform over {-1,0,1}^n in RNS form
{
    for (int s = 0; s < c->n; s++) {
        u64 v; do { v = r.next() >> 62; } while (v == 3);
        for (int i = 0; i < c->k; i++) p[(size_t)i * c->n + s] = v == 0 ? 0 : (v == 1 ? 1 : c->q[i] - 1);
    }
}
void gauss(const crc_ctx *c, Rng &r, u64 *p)              // sigma = 3.19 clipped at 6 sigma, truncated to integer
{
    const double sigma = 3.19, lim = 6 * sigma;           // util/globals.cpp:13-15
    for (int s = 0; s < c->n; s++) {
        double v;
        do { v = sigma * std::sqrt(-2.0 * std::log(r.unit())) * std::cos(6.283185307179586 * r.unit()); } while (std::fabs(v) > lim);
        const int64_t e = (int64_t)v;
        for (int i = 0; i < c->k; i++) p[(size_t)i * c->n + s] = e >= 0 ? (u64)e : c->q[i] - (u64)(-e);
    }
}
void uniform(const crc_ctx *c, Rng &r, u64 *p)
{
    for (int i = 0; i < c->k; i++) for (int s = 0; s < c->n; s++) { u128 z = ((u128)r.next() << 64) | r.next(); p[(size_t)i * c->n + s] = (u64)(z % c->q[i]); }
}
u64 delta_times(const crc_ctx *c, int i, u64 m)           // Delta*m (+ q mod t for the upper half), evaluator.cpp:1168-1191
{
    u128 z = (u128)c->plain.delta[i] * m;
    if (m >= c->plain.threshold) z += c->plain.uhi[i];
    return (u64)(z % c->q[i]);
}
// v = c0 + c1 s + c2 s^2 ... in coefficient form
void dot_secret(const crc_ctx *c, const u64 *sk, const u64 *ct, int size, u64 *v)
{
    const int n = c->n, k = c->k;
    std::vector<u64> tmp(n), sp(n);
    for (int i = 0; i < k; i++) {
        const u64 q = c->q[i]; u64 *o = v + (size_t)i * n;
        std::memset(o, 0, 8 * (size_t)n);
        std::memcpy(sp.data(), sk + (size_t)i * n, 8 * (size_t)n);
        for (int p = 1; p < size; p++) {
            std::memcpy(tmp.data(), ct + ((size_t)p * k + i) * n, 8 * (size_t)n);
            h_ntt_fwd(c->tabs[i], tmp.data(), n);
            for (int s = 0; s < n; s++) { o[s] = addmod(o[s], h_mulmod(tmp[s], sp[s], q), q); sp[s] = h_mulmod(sp[s], sk[(size_t)i * n + s], q); }
        }
        h_ntt_inv(c->tabs[i], o, n);
        for (int s = 0; s < n; s++) o[s] = addmod(o[s], ct[(size_t)i * n + s], q);
    }
}
}  // namespace

// known-answer access to the generator (RFC 8439 section 2.3.2 test vector; tests/test_client_rng.py)
extern "C" int crc_chacha20_block(const uint8_t *key, uint32_t counter, const uint8_t *nonce, uint8_t *out)
{
    if (!key || !nonce || !out) return CRC_ERR_INVALID_ARGUMENT;
    u32 nw[3], o[16];
    for (int i = 0; i < 3; i++) nw[i] = (u32)nonce[4 * i] | ((u32)nonce[4 * i + 1] << 8) | ((u32)nonce[4 * i + 2] << 16) | ((u32)nonce[4 * i + 3] << 24);
    chacha20_block(load_key(key), counter, nw[0], nw[1], nw[2], o);
    for (int i = 0; i < 16; i++) { out[4 * i] = (uint8_t)o[i]; out[4 * i + 1] = (uint8_t)(o[i] >> 8); out[4 * i + 2] = (uint8_t)(o[i] >> 16); out[4 * i + 3] = (uint8_t)(o[i] >> 24); }
    return CRC_OK;
}

extern "C" int crc_random_key(uint8_t *key)
{
    if (!key) return CRC_ERR_INVALID_ARGUMENT;
    size_t got = 0;
    while (got < CRC_KEY_BYTES) {
        const ssize_t r = getrandom(key + got, CRC_KEY_BYTES - got, 0);
        if (r < 0) { if (errno == EINTR) continue; return CRC_ERR_IO; }
        got += (size_t)r;
    }
    return CRC_OK;
}

static int keygen_impl(const crc_ctx *c, const ChaChaKey &key, uint64_t *sk, uint64_t *pk)
{
    const int n = c->n, k = c->k;
    Rng r(key, 0, 0, (u32)CHACHA_DOM_KEYGEN << 24);
    std::vector<u64> e((size_t)k * n);
    ternary(c, r, sk); uniform(c, r, pk + (size_t)k * n); gauss(c, r, e.data());
    for (int i = 0; i < k; i++) {
        const u64 q = c->q[i];
        h_ntt_fwd(c->tabs[i], sk + (size_t)i * n, n); h_ntt_fwd(c->tabs[i], pk + ((size_t)k + i) * n, n); h_ntt_fwd(c->tabs[i], e.data() + (size_t)i * n, n);
        for (int s = 0; s < n; s++) {             // pk0 = -(a s + e), pk1 = a   (keygenerator.cpp:112-150), NTT form
            const size_t o = (size_t)i * n + s;
            pk[o] = negmod(addmod(h_mulmod(sk[o], pk[(size_t)k * n + o], q), e[o], q), q);
        }
    }
    return CRC_OK;
}
extern "C" int crc_keygen_key(const crc_ctx *c, const uint8_t *key, uint64_t *sk, uint64_t *pk)
{
    if (!c || !key || !sk || !pk) return CRC_ERR_INVALID_ARGUMENT;
    return keygen_impl(c, load_key(key), sk, pk);
}
extern "C" int crc_keygen(const crc_ctx *c, uint64_t seed, uint64_t *sk, uint64_t *pk)
{
    if (!c || !sk || !pk) return CRC_ERR_INVALID_ARGUMENT;
    return keygen_impl(c, seed_key(seed), sk, pk);
}

// A key-switching key towards the secret key s for the target polynomial w (NTT form): for l < k and d < L_l the pair first = -(a s + e) + [j == l] (q/q_l) 2^(dbc d) w,
// second = a, NTT form, [2 L_l][k][n] per l -- the evaluation keys with w = s^2 (keygenerator.cpp:652-698), a Galois key with w = sigma_g(s) (:325-405)
static void switch_key_impl(const crc_ctx *c, Rng &r, const uint64_t *sk, const u64 *target, int dbc, uint64_t *out)
{
    const int n = c->n, k = c->k;
    std::vector<u64> e((size_t)k * n);
    u64 *key = out;
    for (int l = 0; l < k; l++) {
        u64 factor = 1;                            // (q/q_l) mod q_l, then times 2^(dbc*d)   keygenerator.cpp:652-698
        for (int j = 0; j < k; j++) if (j != l) factor = h_mulmod(factor, c->q[j] % c->q[l], c->q[l]);
        const int L = evk_digits(c->q[l], dbc);
        for (int d = 0; d < L; d++) {
            u64 *first = key + (size_t)(2 * d) * k * n, *second = first + (size_t)k * n;
            uniform(c, r, second); gauss(c, r, e.data());
            for (int j = 0; j < k; j++) {
                const u64 q = c->q[j];
                h_ntt_fwd(c->tabs[j], second + (size_t)j * n, n); h_ntt_fwd(c->tabs[j], e.data() + (size_t)j * n, n);
                for (int s = 0; s < n; s++) {
                    const size_t o = (size_t)j * n + s;
                    u64 v = negmod(addmod(h_mulmod(second[o], sk[o], q), e[o], q), q);
                    if (j == l) v = addmod(v, h_mulmod(target[o], factor, q), q);
                    first[o] = v;
                }
            }
            factor = h_mulmod(factor, (1ULL << dbc) % c->q[l], c->q[l]);
        }
        key += (size_t)2 * L * k * n;
    }
}
static int gen_evk_impl(const crc_ctx *c, const ChaChaKey &ckey, const uint64_t *sk, int dbc, uint64_t *evk)
{
    if (!own_gadget(c)) return CRC_ERR_PARAMETERS;             // a level with an inherited gadget takes its keys from above (crc_keys_restrict*)
    if (!dbc_ok(dbc)) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k;
    Rng r(ckey, 0, 0, (u32)CHACHA_DOM_EVK << 24);
    std::vector<u64> s2((size_t)k * n);
    for (int j = 0; j < k; j++) for (int s = 0; s < n; s++) { const size_t o = (size_t)j * n + s; s2[o] = h_mulmod(sk[o], sk[o], c->q[j]); }
    switch_key_impl(c, r, sk, s2.data(), dbc, evk);
    return CRC_OK;
}
extern "C" int crc_gen_evk_key(const crc_ctx *c, const uint8_t *key, const uint64_t *sk, int dbc, uint64_t *evk)
{
    if (!c || !key || !sk || !evk) return CRC_ERR_INVALID_ARGUMENT;
    return gen_evk_impl(c, load_key(key), sk, dbc, evk);
}
extern "C" int crc_gen_evk(const crc_ctx *c, uint64_t seed, const uint64_t *sk, int dbc, uint64_t *evk)
{
    if (!c || !sk || !evk) return CRC_ERR_INVALID_ARGUMENT;
    return gen_evk_impl(c, seed_key(seed), sk, dbc, evk);
}

// ---- Galois elements, keys and the rotation planner (Evaluator::apply_galois / rotate_rows / rotate_columns, KeyGenerator::generate_galois_keys) ----
extern "C" int crc_galois_elt_valid(const crc_ctx *c, uint64_t g) { return c && (g & 1) && g < 2 * (u64)c->n ? 1 : 0; }      // evaluator.cpp:1595
extern "C" uint64_t crc_galois_elt_rows(const crc_ctx *c, int steps)
{
    if (!c || c->n < 2) return 0;
    const long long half = c->n / 2, a = steps < 0 ? -(long long)steps : steps;
    if (a >= half) return 0;                       // "step count too large", evaluator.cpp:1808
    const long long e = steps < 0 ? half - a : a;  // a right rotation by a is a left rotation by n/2 - a
    u64 g = 1;
    for (long long i = 0; i < e; i++) g = g * 3 & (2 * (u64)c->n - 1);
    return g;
}
extern "C" uint64_t crc_galois_elt_columns(const crc_ctx *c) { return c ? 2 * (u64)c->n - 1 : 0; }
extern "C" int crc_galois_default_elts(const crc_ctx *c, uint64_t *out, int cap)
{
    if (!c) return CRC_ERR_INVALID_ARGUMENT;
    const u64 mask = 2 * (u64)c->n - 1;
    u64 p = 3, m = 1, list[2 * 64];               // keygenerator.cpp:436-453: m - 1, then 3^(2^i) and 3^(-2^i) for i < log2 n - 1
    for (u64 x = 3, e = (u64)c->n - 1; e; e >>= 1, x = x * x & mask) if (e & 1) m = m * x & mask;      // 3^-1 = 3^(n - 1) mod 2n
    int cnt = 0;
    // (SEAL keeps the keys in a map: 3^(n/4) is its own inverse and appears once)
    auto put = [&](u64 e) { for (int i = 0; i < cnt; i++) if (list[i] == e) return; list[cnt++] = e; };
    put(mask);
    for (int i = 0; i < c->logn - 1; i++) { put(p); p = p * p & mask; put(m); m = m * m & mask; }
    if (!out) return cnt;
    if (cap < cnt) return CRC_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < cnt; i++) out[i] = list[i];
    return cnt;
}
// The steps of apply_galois(g) with the keys of elts[]: the indices into elts to apply, in order (evaluator.cpp:1623-1661).  Returns their count: 0 for g = 1, one
// where the key of g is in the set, else the bits of the discrete logarithm over 3 or 3^-1, whichever has fewer, then 2n - 1 for the sign
extern "C" int crc_galois_plan(const crc_ctx *c, uint64_t g, const uint64_t *elts, int n_elts, int *steps_out, int cap)
{
    if (!c || !crc_galois_elt_valid(c, g) || n_elts < 0 || (n_elts && !elts) || cap < 0 || (cap && !steps_out)) return CRC_ERR_INVALID_ARGUMENT;
    if (g == 1) return 0;
    auto find = [&](u64 e) { for (int i = 0; i < n_elts; i++) if (elts[i] == e) return i; return -1; };
    int cnt = 0;
    auto put = [&](u64 e) { const int i = find(e); if (i < 0 || cnt >= cap) return false; steps_out[cnt++] = i; return true; };
    if (find(g) >= 0) return put(g) ? 1 : CRC_ERR_INVALID_ARGUMENT;
    const u64 mask = 2 * (u64)c->n - 1, half = (u64)c->n / 2;
    u64 o1 = 0, o2 = 0, p = 1;                     // g = 3^o1 (-1)^o2
    for (; o1 < half; o1++, p = p * 3 & mask) { if (p == g) break; if (((mask + 1) - p) == g) { o2 = 1; break; } }
    if (o1 >= half) return CRC_ERR_INVALID_ARGUMENT;               // (n = 2: every odd residue is +-1)
    u64 gen = 3;
    if (__builtin_popcountll(half - o1) < __builtin_popcountll(o1)) {
        o1 = half - o1; gen = 1;
        for (u64 x = 3, e = (u64)c->n - 1; e; e >>= 1, x = x * x & mask) if (e & 1) gen = gen * x & mask;
    }
    for (; o1; o1 >>= 1, gen = gen * gen & mask) if ((o1 & 1) && !put(gen)) return CRC_ERR_INVALID_ARGUMENT;
    if (o2 && !put(mask)) return CRC_ERR_INVALID_ARGUMENT;
    return cnt;
}
// sigma_g of a coefficient row mod q (util::apply_galois, util/polyarithsmallmod.h:313-360): the host twin of galois_permute_kernel's gather
static void galois_row(const u64 *in, u64 *out, int n, u64 g, u64 q)
{
    for (u64 i = 0; i < (u64)n; i++) {
        const u64 r = i * g;
        out[r & ((u64)n - 1)] = r & (u64)n ? negmod(in[i], q) : in[i];
    }
}
// One key blob (crc_evk_words) per element: the evaluation-key construction with s^2 replaced by NTT(sigma_g(INTT(s))).  A stream of its own per element
// (CHACHA_DOM_GALOIS, the element in the nonce): keys of different elements never share randomness, and a set's keys do not depend on its order
static int gen_galois_impl(const crc_ctx *c, const ChaChaKey &ckey, const uint64_t *sk, int dbc, const uint64_t *elts, int n_elts, uint64_t *gk)
{
    if (!own_gadget(c)) return CRC_ERR_PARAMETERS;
    if (!dbc_ok(dbc) || n_elts < 0) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_elts; e++) if (!crc_galois_elt_valid(c, elts[e])) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k;
    const size_t words = crc_evk_words(c, dbc);
    std::vector<u64> sc((size_t)k * n);            // s in coefficient form
    std::memcpy(sc.data(), sk, 8 * (size_t)k * n);
    for (int j = 0; j < k; j++) h_ntt_inv(c->tabs[j], sc.data() + (size_t)j * n, n);
    crc_host::parallel_for((size_t)n_elts, 1, [&](size_t e0, size_t e1) {
    std::vector<u64> w((size_t)k * n);
    for (size_t e = e0; e < e1; e++) {
        const u64 g = elts[e];
        for (int j = 0; j < k; j++) { galois_row(sc.data() + (size_t)j * n, w.data() + (size_t)j * n, n, g, c->q[j]); h_ntt_fwd(c->tabs[j], w.data() + (size_t)j * n, n); }
        Rng r(ckey, (u32)g, (u32)(g >> 32), (u32)CHACHA_DOM_GALOIS << 24);
        switch_key_impl(c, r, sk, w.data(), dbc, gk + e * words);
    }
    });
    return CRC_OK;
}
extern "C" int crc_gen_galois_keys_key(const crc_ctx *c, const uint8_t *key, const uint64_t *sk, int dbc, const uint64_t *elts, int n_elts, uint64_t *gk)
{
    if (!c || !key || !sk || (n_elts > 0 && (!elts || !gk))) return CRC_ERR_INVALID_ARGUMENT;
    return gen_galois_impl(c, load_key(key), sk, dbc, elts, n_elts, gk);
}
extern "C" int crc_gen_galois_keys(const crc_ctx *c, uint64_t seed, const uint64_t *sk, int dbc, const uint64_t *elts, int n_elts, uint64_t *gk)
{
    if (!c || !sk || (n_elts > 0 && (!elts || !gk))) return CRC_ERR_INVALID_ARGUMENT;
    return gen_galois_impl(c, seed_key(seed), sk, dbc, elts, n_elts, gk);
}

// ---- conjugated Galois keys (the hoisted rotations, abi.hip) ----
// sigma_g on an NTT-form row is a gather by index alone: X[i] = p(psi^(2 brev(i) + 1)), so NTT(sigma_g(p))[i] = X[pi_g(i)] with 2 brev(pi_g(i)) + 1 =
// g (2 brev(i) + 1) mod 2n -- the table galois_permute_ntt_kernel computes on the fly
extern "C" int crc_galois_ntt_table(const crc_ctx *c, uint64_t g, uint32_t *table)
{
    if (!c || !table || !crc_galois_elt_valid(c, g)) return CRC_ERR_INVALID_ARGUMENT;
    const u64 n = (u64)c->n, m2 = 2 * n - 1;
    auto brev = [&](u64 v) { u64 r = 0; for (int b = 0; b < c->logn; b++) r |= ((v >> b) & 1) << (c->logn - 1 - b); return r; };
    for (u64 i = 0; i < n; i++) table[i] = (uint32_t)brev(((g * (2 * brev(i) + 1)) & m2) >> 1);
    return CRC_OK;
}
static u64 galois_inverse(const crc_ctx *c, u64 g)
{
    const u64 mask = 2 * (u64)c->n - 1;
    u64 h = 1;                                     // g^-1 = g^(n - 1) mod 2n (the odd residues have exponent n / 2)
    for (u64 x = g & mask, e = (u64)c->n - 1; e; e >>= 1, x = x * x & mask) if (e & 1) h = h * x & mask;
    return h;
}
// K'_g = sigma_g^-1(K_g): sigma_{g^-1} of every polynomial of the blob of g, the same layout.  K_g switches sigma_g(s) -> s; the gadget constants are integers,
// which sigma fixes, so K'_g switches s -> sigma_g^-1(s), and sigma_g of that key switch's result is a ciphertext under s again.  g = 1 has no key
extern "C" int crc_galois_conjugate_keys(const crc_ctx *c, const uint64_t *elts, int n_elts, int dbc, const uint64_t *gk, uint64_t *out)
{
    if (!c || !dbc_ok(dbc) || n_elts < 0 || (n_elts > 0 && (!elts || !gk || !out || gk == out))) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_elts; e++) if (!crc_galois_elt_valid(c, elts[e]) || elts[e] == 1) return CRC_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)c->n, words = crc_evk_words(c, dbc), rows = words / n;
    crc_host::parallel_for((size_t)n_elts, 1, [&](size_t e0, size_t e1) {
    std::vector<uint32_t> tab(n);
    for (size_t e = e0; e < e1; e++) {
        crc_galois_ntt_table(c, galois_inverse(c, elts[e]), tab.data());
        for (size_t r = 0; r < rows; r++) {
            const u64 *src = gk + e * words + r * n; u64 *dst = out + e * words + r * n;
            for (size_t i = 0; i < n; i++) dst[i] = src[tab[i]];
        }
    }
    });
    return CRC_OK;
}

static int encrypt_impl(const crc_ctx *c, const uint64_t *pk, const uint64_t *plain, size_t count, const ChaChaKey &key, uint64_t stream_base, uint64_t *ct)
{
    const int n = c->n, k = c->k;
    // one keystream per ciphertext: ranges of ciphertexts on the host threads, the same bits however they are split
    crc_host::parallel_for(count, 8, [&](size_t m0, size_t m1) {
    std::vector<u64> u((size_t)k * n), e((size_t)k * n);
    for (size_t m = m0; m < m1; m++) {
        const u64 sid = stream_base + m;
        Rng r(key, (u32)sid, (u32)(sid >> 32), (u32)CHACHA_DOM_ENC_HOST << 24);
        u64 *o = ct + m * 2 * (size_t)k * n; const u64 *pl = plain + m * (size_t)n;
        ternary(c, r, u.data());
        for (int i = 0; i < k; i++) {
            const u64 q = c->q[i];
            h_ntt_fwd(c->tabs[i], u.data() + (size_t)i * n, n);
            for (int s = 0; s < n; s++) { const size_t x = (size_t)i * n + s; o[x] = h_mulmod(u[x], pk[x], q); o[(size_t)k * n + x] = h_mulmod(u[x], pk[(size_t)k * n + x], q); }
            h_ntt_inv(c->tabs[i], o + (size_t)i * n, n); h_ntt_inv(c->tabs[i], o + ((size_t)k + i) * n, n);
        }
        for (int p = 0; p < 2; p++) {
            gauss(c, r, e.data());
            for (int i = 0; i < k; i++) for (int s = 0; s < n; s++) {
                const size_t x = (size_t)i * n + s; u64 v = addmod(o[(size_t)p * k * n + x], e[x], c->q[i]);
                if (p == 0) v = addmod(v, delta_times(c, i, pl[s]), c->q[i]);
                o[(size_t)p * k * n + x] = v;
            }
        }
    }
    });
    return CRC_OK;
}
extern "C" int crc_encrypt_key(const crc_ctx *c, const uint64_t *pk, const uint64_t *plain, size_t count, const uint8_t *key, uint64_t stream_base, uint64_t *ct)
{
    if (!c || !pk || !plain || !ct || !key) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_impl(c, pk, plain, count, load_key(key), stream_base, ct);
}
extern "C" int crc_encrypt(const crc_ctx *c, const uint64_t *pk, const uint64_t *plain, size_t count, uint64_t seed, uint64_t *ct)
{
    if (!c || !pk || !plain || !ct) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_impl(c, pk, plain, count, seed_key(seed), 0, ct);
}

// BFV encryption under the secret key: c1 = a uniform in R_q, sampled directly as NTT-form residues A; c0 = -(a s) + e + Delta m, i.e. in NTT form
// NTT(e + Delta m) - A . s -- one forward transform per modulus, no public key.  The NTT-form result is the definition, the coefficient form its inverse
// transform.  The host twin of enc_sym_sample_kernel (kernels_client.hip): the stream layout of chacha.h, bit for bit
void k_encrypt_cdt(u64 *out19);                            // (kernels_client.hip: the thresholds of the noise magnitudes)
static int encrypt_sym_impl(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, const ChaChaKey &key, uint64_t stream_base, int out_form,
                            uint64_t *ct)
{
    const int n = c->n, k = c->k;
    u64 T[19]; k_encrypt_cdt(T);
    crc_host::parallel_for(count, 8, [&](size_t m0, size_t m1) {
    for (size_t m = m0; m < m1; m++) {
        const u64 sid = stream_base + m;
        u64 *o = ct + m * 2 * (size_t)k * n; const u64 *pl = plain + m * (size_t)n;
        for (int s = 0; s < n; s += 2) {
            const u32 n2 = ((u32)CHACHA_DOM_ENC_SYM << 24) | (u32)s;
            u32 b[16];
            chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), n2, b);
            int e[2];
            for (int x = 0; x < 2; x++) {
                const u64 w = (u64)b[2 * x] | ((u64)b[2 * x + 1] << 32);
                int a = 0; for (int j = 0; j < 19; j++) a += w >= T[j] ? 1 : 0;
                e[x] = (b[4] >> x) & 1u ? -a : a;
            }
            for (int i = 0; i < k; i++) {
                const u64 q = c->q[i];
                if (i & 1) chacha20_block(key, (u32)CHACHA_SYM_BLOCK(i), (u32)sid, (u32)(sid >> 32), n2, b);
                const u32 *w = b + CHACHA_SYM_WORD(i);
                for (int x = 0; x < 2; x++) {
                    const u128 z = (u128)w[4 * x] | ((u128)w[4 * x + 1] << 32) | ((u128)w[4 * x + 2] << 64) | ((u128)w[4 * x + 3] << 96);
                    o[((size_t)k + i) * n + s + x] = (u64)(z % q);
                    const u64 er = e[x] >= 0 ? (u64)e[x] : q - (u64)(-e[x]);
                    o[(size_t)i * n + s + x] = addmod(er, delta_times(c, i, pl[s + x]), q);
                }
            }
        }
        for (int i = 0; i < k; i++) {
            const u64 q = c->q[i]; u64 *c0 = o + (size_t)i * n, *c1 = o + ((size_t)k + i) * n; const u64 *sp = sk + (size_t)i * n;
            h_ntt_fwd(c->tabs[i], c0, n);
            for (int s = 0; s < n; s++) c0[s] = submod(c0[s], h_mulmod(c1[s], sp[s], q), q);
            if (out_form == CRC_COEFF) { h_ntt_inv(c->tabs[i], c0, n); h_ntt_inv(c->tabs[i], c1, n); }
        }
    }
    });
    return CRC_OK;
}
extern "C" int crc_encrypt_sym_key(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, const uint8_t *key, uint64_t stream_base, int out_form,
                                   uint64_t *ct)
{
    if (!c || !sk || !plain || !ct || !key || (out_form != CRC_COEFF && out_form != CRC_NTT)) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_sym_impl(c, sk, plain, count, load_key(key), stream_base, out_form, ct);
}
extern "C" int crc_encrypt_sym(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, uint64_t seed, int out_form, uint64_t *ct)
{
    if (!c || !sk || !plain || !ct || (out_form != CRC_COEFF && out_form != CRC_NTT)) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_sym_impl(c, sk, plain, count, seed_key(seed), 0, out_form, ct);
}

// Seeded secret-key ciphertexts: c1 = A(public seed, stream id) is regenerated by whoever holds the seed, so only the c0 rows travel.  The mask comes from the
// PUBLIC seed (CHACHA_DOM_SEEDED_A), the noise from the PRIVATE key (CHACHA_DOM_SEEDED_E): the layouts of chacha.h, bit for bit what seeded_expand_kernel reads.
// A of one ciphertext, NTT form: a [k][n]
static void seeded_mask(const crc_ctx *c, const ChaChaKey &seed, u64 sid, u64 *a)
{
    const int n = c->n, k = c->k;
    for (int s = 0; s < n; s += 2) {
        const u32 n2 = ((u32)CHACHA_DOM_SEEDED_A << 24) | (u32)s;
        u32 b[16];
        for (int i = 0; i < k; i++) {
            if (!(i & 1)) chacha20_block(seed, (u32)(i >> 1), (u32)sid, (u32)(sid >> 32), n2, b);
            const u32 *w = b + 8 * (i & 1);
            for (int x = 0; x < 2; x++) {
                const u128 z = (u128)w[4 * x] | ((u128)w[4 * x + 1] << 32) | ((u128)w[4 * x + 2] << 64) | ((u128)w[4 * x + 3] << 96);
                a[(size_t)i * n + s + x] = (u64)(z % c->q[i]);
            }
        }
    }
}
static int encrypt_sym_seeded_impl(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, const ChaChaKey &key, const ChaChaKey &seed,
                                   uint64_t stream_base, uint64_t *c0_out)
{
    const int n = c->n, k = c->k;
    u64 T[19]; k_encrypt_cdt(T);
    crc_host::parallel_for(count, 8, [&](size_t m0, size_t m1) {
    std::vector<u64> a((size_t)k * n);
    for (size_t m = m0; m < m1; m++) {
        const u64 sid = stream_base + m;
        u64 *o = c0_out + m * (size_t)k * n; const u64 *pl = plain + m * (size_t)n;
        seeded_mask(c, seed, sid, a.data());
        for (int s = 0; s < n; s += 2) {
            u32 b[16];
            chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), ((u32)CHACHA_DOM_SEEDED_E << 24) | (u32)s, b);
            for (int x = 0; x < 2; x++) {
                const u64 w = (u64)b[2 * x] | ((u64)b[2 * x + 1] << 32);
                int mag = 0; for (int j = 0; j < 19; j++) mag += w >= T[j] ? 1 : 0;
                const int e = (b[4] >> x) & 1u ? -mag : mag;
                for (int i = 0; i < k; i++) {
                    const u64 q = c->q[i], er = e >= 0 ? (u64)e : q - (u64)(-e);
                    o[(size_t)i * n + s + x] = addmod(er, delta_times(c, i, pl[s + x]), q);
                }
            }
        }
        for (int i = 0; i < k; i++) {
            const u64 q = c->q[i]; u64 *c0 = o + (size_t)i * n; const u64 *c1 = a.data() + (size_t)i * n, *sp = sk + (size_t)i * n;
            h_ntt_fwd(c->tabs[i], c0, n);
            for (int s = 0; s < n; s++) c0[s] = submod(c0[s], h_mulmod(c1[s], sp[s], q), q);
        }
    }
    });
    return CRC_OK;
}
extern "C" int crc_seeded_public_seed(uint64_t seed, uint8_t *h_seed)
{
    if (!h_seed) return CRC_ERR_INVALID_ARGUMENT;
    const ChaChaKey k = seed_key(~seed);
    for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) h_seed[4 * i + b] = (uint8_t)(k.w[i] >> (8 * b));
    return CRC_OK;
}
extern "C" int crc_encrypt_sym_seeded_key(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, const uint8_t *key, const uint8_t *seed,
                                          uint64_t stream_base, uint64_t *c0)
{
    if (!c || !sk || !plain || !c0 || !key || !seed || !std::memcmp(key, seed, CRC_KEY_BYTES)) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_sym_seeded_impl(c, sk, plain, count, load_key(key), load_key(seed), stream_base, c0);
}
extern "C" int crc_encrypt_sym_seeded(const crc_ctx *c, const uint64_t *sk, const uint64_t *plain, size_t count, uint64_t seed, uint64_t *c0)
{
    if (!c || !sk || !plain || !c0) return CRC_ERR_INVALID_ARGUMENT;
    return encrypt_sym_seeded_impl(c, sk, plain, count, seed_key(seed), seed_key(~seed), 0, c0);
}
extern "C" int crc_seeded_expand(const crc_ctx *c, const uint64_t *c0, size_t count, const uint8_t *seed, uint64_t stream_base, int out_form, uint64_t *ct)
{
    if (!c || !c0 || !ct || !seed || (out_form != CRC_COEFF && out_form != CRC_NTT)) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k;
    const ChaChaKey sd = load_key(seed);
    crc_host::parallel_for(count, 8, [&](size_t m0, size_t m1) {
    for (size_t m = m0; m < m1; m++) {
        u64 *o = ct + m * 2 * (size_t)k * n;
        std::memcpy(o, c0 + m * (size_t)k * n, 8 * (size_t)k * n);
        seeded_mask(c, sd, stream_base + m, o + (size_t)k * n);
        if (out_form == CRC_COEFF) for (int i = 0; i < 2 * k; i++) h_ntt_inv(c->tabs[i % k], o + (size_t)i * n, n);
    }
    });
    return CRC_OK;
}

extern "C" int crc_decrypt(const crc_ctx *c, const uint64_t *sk, const uint64_t *ct, size_t count, int size, uint64_t *plain)
{
    if (!c || !sk || !ct || !plain || size < 2) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k; const u64 t = c->t, gamma = c->gmod.q;
    std::vector<u64> v((size_t)k * n);
    for (size_t m = 0; m < count; m++) {
        dot_secret(c, sk, ct + m * (size_t)size * k * n, size, v.data());
        u64 *out = plain + m * (size_t)n;
        for (int s = 0; s < n; s++) {
            u128 at = 0, ag = 0;                   // fastbconv_plain_gamma of (t gamma v), baseconverter.cpp:744-797
            for (int i = 0; i < k; i++) {
                const u64 y = h_mulmod(h_mulmod(v[(size_t)i * n + s], c->tgamma_mod_q[i], c->q[i]), c->behz.inv_qhat[i], c->q[i]);
                at += (u128)y * c->qhat_mod_tg[0][i]; ag += (u128)y * c->qhat_mod_tg[1][i];
            }
            const u64 rt = h_mulmod((u64)(at % t), c->neg_inv_q_mod_tg[0], t), rg = h_mulmod((u64)(ag % gamma), c->neg_inv_q_mod_tg[1], gamma);
            const u64 w = rg > (gamma >> 1) ? addmod(rt, (gamma - rg) % t, t) : submod(rt, rg % t, t);     // centred correction, decryptor.cpp:193-215
            out[s] = h_mulmod(w, c->inv_gamma_mod_t, t);
        }
    }
    return CRC_OK;
}

extern "C" int crc_noise_budget(const crc_ctx *c, const uint64_t *sk, const uint64_t *ct, int size)
{
    // invariant noise budget = bits(q) - bits(|| t (c0 + c1 s + ...) mod q ||_inf centred) - 1   (decryptor.cpp:295-403)
    if (!c || !sk || !ct || size < 2) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k;
    std::vector<u64> v((size_t)k * n);
    dot_secret(c, sk, ct, size, v.data());
    auto cmp = [&](const u64 *a, const u64 *b) { for (int l = k - 1; l >= 0; l--) if (a[l] != b[l]) return a[l] < b[l] ? -1 : 1; return 0; };
    auto sub = [&](u64 *a, const u64 *b) { u64 br = 0; for (int l = 0; l < k; l++) { u128 z = (u128)a[l] - b[l] - br; a[l] = (u64)z; br = (u64)(z >> 64) & 1; } };
    std::vector<std::vector<u64>> qhat(k, std::vector<u64>(k, 0));
    for (int i = 0; i < k; i++) { qhat[i][0] = 1; for (int j = 0; j < k; j++) if (j != i) { u64 cy = 0; for (int l = 0; l < k; l++) { u128 z = (u128)qhat[i][l] * c->q[j] + cy; qhat[i][l] = (u64)z; cy = (u64)(z >> 64); } } }
    std::vector<u64> half(c->qbig), norm(k, 0), acc(k), term(k);
    { u64 cy = 0; for (int l = k - 1; l >= 0; l--) { u64 nc = half[l] & 1; half[l] = (half[l] >> 1) | (cy << 63); cy = nc; } }
    for (int s = 0; s < n; s++) {
        std::fill(acc.begin(), acc.end(), 0);
        for (int i = 0; i < k; i++) {
            const u64 x = h_mulmod(h_mulmod(v[(size_t)i * n + s], c->t % c->q[i], c->q[i]), c->behz.inv_qhat[i], c->q[i]);
            u64 cy = 0; for (int l = 0; l < k; l++) { u128 z = (u128)qhat[i][l] * x + cy; term[l] = (u64)z; cy = (u64)(z >> 64); }
            cy = 0; for (int l = 0; l < k; l++) { u128 z = (u128)acc[l] + term[l] + cy; acc[l] = (u64)z; cy = (u64)(z >> 64); }
            if (cmp(acc.data(), c->qbig.data()) >= 0) sub(acc.data(), c->qbig.data());
        }
        if (cmp(acc.data(), half.data()) > 0) { std::vector<u64> tq(c->qbig); sub(tq.data(), acc.data()); acc = tq; }
        if (cmp(acc.data(), norm.data()) > 0) norm = acc;
    }
    int nb = 0; for (int l = k - 1; l >= 0; l--) if (norm[l]) { nb = 64 * l + 64 - __builtin_clzll(norm[l]); break; }
    const int b = c->total_bits - nb - 1;
    return b > 0 ? b : 0;
}

// ---- seeded key-switching keys: the first rows and a public seed (chacha.h: CHACHA_DOM_KSK_A / CHACHA_DOM_KSK_E) ----
// A key id is 0 (the evaluation key, target s^2) or a valid Galois element g (target sigma_g(s)).  The host twin of seeded_keys_device.h, bit for bit.
namespace {
struct KskPair { int l; u64 factor; };                     // pair p of a blob: its modulus l and (q/q_l) 2^(dbc d) mod q_l, as switch_key_impl walks them
std::vector<KskPair> ksk_pairs(const crc_ctx *c, int dbc)
{
    int L[CRC_MAXK]; u64 qhat[CRC_MAXK];
    evk_gadget(c, dbc, L, qhat);
    std::vector<KskPair> v;
    for (int l = 0; l < c->k; l++) {
        u64 factor = qhat[l];
        for (int d = 0; d < L[l]; d++) { v.push_back({l, factor}); factor = h_mulmod(factor, (1ULL << dbc) % c->q[l], c->q[l]); }
    }
    return v;
}
bool ksk_id_ok(const crc_ctx *c, u64 id) { return id == 0 || crc_galois_elt_valid(c, id); }
// A of one pair, NTT form: a [k][n]
void ksk_mask(const crc_ctx *c, const ChaChaKey &seed, u64 id, u32 n1, u64 *a)
{
    const int n = c->n, k = c->k;
    for (int s = 0; s < n; s += 2) {
        const u32 n2 = ((u32)CHACHA_DOM_KSK_A << 24) | (u32)s;
        u32 b[16];
        for (int i = 0; i < k; i++) {
            if (!(i & 1)) chacha20_block(seed, (u32)(i >> 1), (u32)id, n1, n2, b);
            const u32 *w = b + 8 * (i & 1);
            for (int x = 0; x < 2; x++) {
                const u128 z = (u128)w[4 * x] | ((u128)w[4 * x + 1] << 32) | ((u128)w[4 * x + 2] << 64) | ((u128)w[4 * x + 3] << 96);
                a[(size_t)i * n + s + x] = (u64)(z % c->q[i]);
            }
        }
    }
}
int gen_keys_seeded_impl(const crc_ctx *c, const ChaChaKey &key, const ChaChaKey &seed, const uint64_t *sk, int dbc, const uint64_t *ids, int n_ids, uint64_t *first)
{
    if (!own_gadget(c)) return CRC_ERR_PARAMETERS;
    if (!dbc_ok(dbc) || n_ids < 0) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_ids; e++) if (!ksk_id_ok(c, ids[e])) return CRC_ERR_INVALID_ARGUMENT;
    const int n = c->n, k = c->k;
    const std::vector<KskPair> pairs = ksk_pairs(c, dbc);
    const size_t P = pairs.size();
    u64 T[19]; k_encrypt_cdt(T);
    crc_host::parallel_for((size_t)n_ids, 1, [&](size_t e0, size_t e1) {
    std::vector<u64> a((size_t)k * n), w((size_t)k * n);
    std::vector<uint32_t> tab(n);
    for (size_t e = e0; e < e1; e++) {
        const u64 id = ids[e];
        if (id) crc_galois_ntt_table(c, id, tab.data());
        for (int j = 0; j < k; j++) for (int s = 0; s < n; s++) {
            const size_t o = (size_t)j * n + s;
            w[o] = id ? sk[(size_t)j * n + tab[s]] : h_mulmod(sk[o], sk[o], c->q[j]);
        }
        for (size_t p = 0; p < P; p++) {
            u64 *o = first + (e * P + p) * (size_t)k * n;
            const u32 n1 = CHACHA_KSK_NONCE1(p, dbc, k);
            ksk_mask(c, seed, id, n1, a.data());
            for (int s = 0; s < n; s += 2) {
                u32 b[16];
                chacha20_block(key, 0, (u32)id, n1, ((u32)CHACHA_DOM_KSK_E << 24) | (u32)s, b);
                for (int x = 0; x < 2; x++) {
                    const u64 m = (u64)b[2 * x] | ((u64)b[2 * x + 1] << 32);
                    int mag = 0; for (int j = 0; j < 19; j++) mag += m >= T[j] ? 1 : 0;
                    const int ev = (b[4] >> x) & 1u ? -mag : mag;
                    for (int i = 0; i < k; i++) o[(size_t)i * n + s + x] = ev >= 0 ? (u64)ev : c->q[i] - (u64)(-ev);
                }
            }
            for (int j = 0; j < k; j++) {
                const u64 q = c->q[j];
                h_ntt_fwd(c->tabs[j], o + (size_t)j * n, n);
                for (int s = 0; s < n; s++) {
                    const size_t x = (size_t)j * n + s;
                    u64 v = negmod(addmod(h_mulmod(a[x], sk[x], q), o[x], q), q);
                    if (j == pairs[p].l) v = addmod(v, h_mulmod(w[x], pairs[p].factor, q), q);
                    o[x] = v;
                }
            }
        }
    }
    });
    return CRC_OK;
}
}  // namespace

extern "C" size_t crc_seeded_key_words(const crc_ctx *c, int dbc) { return crc_evk_words(c, dbc) / 2; }
extern "C" int crc_gen_keys_seeded_key(const crc_ctx *c, const uint8_t *key, const uint8_t *seed, const uint64_t *sk, int dbc, const uint64_t *ids, int n_ids,
                                       uint64_t *first)
{
    if (!c || !key || !seed || !sk || (n_ids > 0 && (!ids || !first)) || !std::memcmp(key, seed, CRC_KEY_BYTES)) return CRC_ERR_INVALID_ARGUMENT;
    return gen_keys_seeded_impl(c, load_key(key), load_key(seed), sk, dbc, ids, n_ids, first);
}
extern "C" int crc_gen_keys_seeded(const crc_ctx *c, uint64_t seed, const uint64_t *sk, int dbc, const uint64_t *ids, int n_ids, uint64_t *first)
{
    if (!c || !sk || (n_ids > 0 && (!ids || !first))) return CRC_ERR_INVALID_ARGUMENT;
    return gen_keys_seeded_impl(c, seed_key(seed), seed_key(~seed), sk, dbc, ids, n_ids, first);
}
// first [n_ids][P][k][n] -> blobs [n_ids][crc_evk_words]: pair p of a blob is (first row p, A(seed, id, p)).  conjugate: K' = crc_galois_conjugate_keys of that
extern "C" int crc_seeded_keys_expand(const crc_ctx *c, const uint64_t *first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *seed, int conjugate,
                                      uint64_t *out)
{
    if (!c || !seed || !dbc_ok(dbc) || n_ids < 0 || (conjugate != 0 && conjugate != 1) || (n_ids > 0 && (!first || !ids || !out || first == out)))
        return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_ids; e++) if (!ksk_id_ok(c, ids[e]) || (conjugate && ids[e] <= 1)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)c->n, kn = (size_t)c->k * n, words = crc_evk_words(c, dbc), P = words / (2 * kn);
    const ChaChaKey sd = load_key(seed);
    crc_host::parallel_for((size_t)n_ids, 1, [&](size_t e0, size_t e1) {
    std::vector<u64> blob(conjugate ? words : 0);
    std::vector<uint32_t> tab(conjugate ? n : 0);
    for (size_t e = e0; e < e1; e++) {
        u64 *dst = conjugate ? blob.data() : out + e * words;
        for (size_t p = 0; p < P; p++) {
            std::memcpy(dst + p * 2 * kn, first + (e * P + p) * kn, 8 * kn);
            ksk_mask(c, sd, ids[e], CHACHA_KSK_NONCE1(p, dbc, c->k), dst + p * 2 * kn + kn);
        }
        if (!conjugate) continue;
        crc_galois_ntt_table(c, galois_inverse(c, ids[e]), tab.data());
        for (size_t r = 0; r < words / n; r++) {
            const u64 *src = blob.data() + r * n; u64 *o = out + e * words + r * n;
            for (size_t i = 0; i < n; i++) o[i] = src[tab[i]];
        }
    }
    });
    return CRC_OK;
}

// ---- keys of a level from the keys of the context above it (crc_ctx_create_level): the host twins of ksk_restrict_body / ksk_expand_level_body ----
// A pair (l, d) of a key over Q = q_0 .. q_{K-1} holds E = (Q/q_l) 2^(dbc d) in row l alone; mod q_B = q_0 .. q_{k'-1} the pairs with l >= k' hold nothing, and the
// others are the first P' = Sum_{l < k'} L_l pairs, of which rows [0, k') are a key at the level for the SAME gadget -- hence the level's ksk_inv_qhat
static bool host_ranges_overlap(const void *a, size_t ab, const void *b, size_t bb) { const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b; return a0 < b0 + bb && b0 < a0 + ab; }
extern "C" int crc_keys_restrict(const crc_ctx *from, const crc_ctx *to, const uint64_t *keys, int n_keys, int dbc, uint64_t *out)
{
    if (!keys_level_of(from, to) || !dbc_ok(dbc) || n_keys < 0) return CRC_ERR_INVALID_ARGUMENT;
    if (n_keys == 0) return CRC_OK;
    const size_t n = (size_t)from->n, skn = (size_t)from->k * n, kn = (size_t)to->k * n, in_w = crc_evk_words(from, dbc), out_w = crc_evk_words(to, dbc), P = out_w / (2 * kn);
    if (!keys || !out || host_ranges_overlap(keys, 8 * in_w * n_keys, out, 8 * out_w * n_keys)) return CRC_ERR_INVALID_ARGUMENT;
    crc_host::parallel_for((size_t)n_keys, 1, [&](size_t e0, size_t e1) {
    for (size_t e = e0; e < e1; e++) for (size_t p = 0; p < P; p++) for (int poly = 0; poly < 2; poly++)
        std::memcpy(out + e * out_w + (2 * p + poly) * kn, keys + e * in_w + (2 * p + poly) * skn, 8 * kn);
    });
    return CRC_OK;
}
extern "C" int crc_seeded_keys_expand_level(const crc_ctx *from, const crc_ctx *to, const uint64_t *first, const uint64_t *ids, int n_ids, int dbc, const uint8_t *seed,
                                            int conjugate, uint64_t *out)
{
    if (!keys_level_of(from, to) || !seed || !dbc_ok(dbc) || n_ids < 0 || (conjugate != 0 && conjugate != 1)) return CRC_ERR_INVALID_ARGUMENT;
    if (n_ids == 0) return CRC_OK;
    if (!first || !ids || !out) return CRC_ERR_INVALID_ARGUMENT;
    for (int e = 0; e < n_ids; e++) if (!ksk_id_ok(from, ids[e]) || (conjugate && ids[e] <= 1)) return CRC_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)from->n, skn = (size_t)from->k * n, kn = (size_t)to->k * n, words = crc_evk_words(to, dbc), P = words / (2 * kn),
        sP = crc_evk_words(from, dbc) / (2 * skn);
    if (host_ranges_overlap(first, 8 * sP * skn * n_ids, out, 8 * words * n_ids)) return CRC_ERR_INVALID_ARGUMENT;
    const int name_k = (int)from->key_q.size();                // the k of the stream names: the modulus count of the gadget the keys were generated over
    const ChaChaKey sd = load_key(seed);
    crc_host::parallel_for((size_t)n_ids, 1, [&](size_t e0, size_t e1) {
    std::vector<u64> blob(conjugate ? words : 0);
    std::vector<uint32_t> tab(conjugate ? n : 0);
    for (size_t e = e0; e < e1; e++) {
        u64 *dst = conjugate ? blob.data() : out + e * words;
        for (size_t p = 0; p < P; p++) {
            std::memcpy(dst + p * 2 * kn, first + (e * sP + p) * skn, 8 * kn);
            ksk_mask(to, sd, ids[e], CHACHA_KSK_NONCE1(p, dbc, name_k), dst + p * 2 * kn + kn);      // (the first k' residues of a keystream are a prefix of it)
        }
        if (!conjugate) continue;
        crc_galois_ntt_table(to, galois_inverse(to, ids[e]), tab.data());
        for (size_t r = 0; r < words / n; r++) {
            const u64 *src = blob.data() + r * n; u64 *o = out + e * words + r * n;
            for (size_t i = 0; i < n; i++) o[i] = src[tab[i]];
        }
    }
    });
    return CRC_OK;
}
