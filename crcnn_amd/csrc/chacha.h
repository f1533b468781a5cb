// chacha.h -- ChaCha20 block function (RFC 8439 layout) shared by the host client code (client.cpp) and the device encryptor
// (kernels_client.hip): the generator behind every secret the client side draws (secret key s, encryption sample u, noise e).
//
// The reference (SEAL 2.3.1 KeyGenerator / Encryptor) draws from std::random_device; there are no reference bits to match, only
// laws (uniform ternary, clipped normal sigma 3.19 cut at 6 sigma: util/globals.cpp:13-15).  A 256-bit key -- from the OS
// (crc_random_key -> getrandom(2)) in normal use, expanded from a 64-bit seed only in the explicitly deterministic test / bench
// entry points -- plus a 96-bit nonce that names the stream (domain, ciphertext index, coefficient) gives every sample its own
// keystream block(s); the 32-bit block counter extends a stream when rejection sampling runs past one block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHACHA_HD __host__ __device__ __forceinline__
#else
#define CHACHA_HD inline
#endif

struct ChaChaKey { uint32_t w[8]; };

CHACHA_HD uint32_t chacha_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define CHACHA_QR(a, b, c, d) \
    a += b; d ^= a; d = chacha_rotl(d, 16); c += d; b ^= c; b = chacha_rotl(b, 12); \
    a += b; d ^= a; d = chacha_rotl(d, 8);  c += d; b ^= c; b = chacha_rotl(b, 7);

// out[16] = ChaCha20 block(key, counter, nonce[3])
CHACHA_HD void chacha20_block(const ChaChaKey &key, uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t out[16])
{
    uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
    uint32_t x4 = key.w[0], x5 = key.w[1], x6 = key.w[2], x7 = key.w[3], x8 = key.w[4], x9 = key.w[5], x10 = key.w[6], x11 = key.w[7];
    uint32_t x12 = counter, x13 = n0, x14 = n1, x15 = n2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < 10; r++) {
        CHACHA_QR(x0, x4, x8, x12) CHACHA_QR(x1, x5, x9, x13) CHACHA_QR(x2, x6, x10, x14) CHACHA_QR(x3, x7, x11, x15)
        CHACHA_QR(x0, x5, x10, x15) CHACHA_QR(x1, x6, x11, x12) CHACHA_QR(x2, x7, x8, x13) CHACHA_QR(x3, x4, x9, x14)
    }
    out[0] = x0 + 0x61707865u; out[1] = x1 + 0x3320646eu; out[2] = x2 + 0x79622d32u; out[3] = x3 + 0x6b206574u;
    out[4] = x4 + key.w[0]; out[5] = x5 + key.w[1]; out[6] = x6 + key.w[2]; out[7] = x7 + key.w[3];
    out[8] = x8 + key.w[4]; out[9] = x9 + key.w[5]; out[10] = x10 + key.w[6]; out[11] = x11 + key.w[7];
    out[12] = x12 + counter; out[13] = x13 + n0; out[14] = x14 + n1; out[15] = x15 + n2;
}

// keystream reader: 64-bit words of the stream named by (n0, n1, n2) under `key`
struct ChaChaStream {
    ChaChaKey key; uint32_t n0, n1, n2, counter; uint32_t buf[16]; int pos;
    CHACHA_HD ChaChaStream(const ChaChaKey &k, uint32_t a, uint32_t b, uint32_t c) : key(k), n0(a), n1(b), n2(c), counter(0), pos(16) {}
    CHACHA_HD uint64_t next()
    {
        if (pos >= 16) { chacha20_block(key, counter++, n0, n1, n2, buf); pos = 0; }
        const uint64_t v = (uint64_t)buf[pos] | ((uint64_t)buf[pos + 1] << 32);
        pos += 2;
        return v;
    }
    CHACHA_HD double unit() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }   // uniform in (0, 1)
};

// deterministic entry points (tests, bench, goldens): the 64-bit seed in front of a fixed tag.  NOT secure -- the seed is public
inline ChaChaKey chacha_seed_key(uint64_t seed)
{
    ChaChaKey k; k.w[0] = (uint32_t)seed; k.w[1] = (uint32_t)(seed >> 32);
    const char tag[25] = "crcnn-seeded-determinist";
    for (int i = 0; i < 6; i++) k.w[2 + i] = (uint32_t)(uint8_t)tag[4 * i] | ((uint32_t)(uint8_t)tag[4 * i + 1] << 8) | ((uint32_t)(uint8_t)tag[4 * i + 2] << 16) | ((uint32_t)(uint8_t)tag[4 * i + 3] << 24);
    return k;
}
inline ChaChaKey chacha_load_key(const uint8_t *key)
{
    ChaChaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) | ((uint32_t)key[4 * i + 3] << 24);
    return k;
}

// stream domains (nonce word 2 carries the domain in its top byte)
enum { CHACHA_DOM_KEYGEN = 1, CHACHA_DOM_EVK = 2, CHACHA_DOM_ENC_HOST = 3, CHACHA_DOM_ENC_DEV = 4, CHACHA_DOM_ENC_SYM = 5, CHACHA_DOM_SEEDED_A = 6,
       CHACHA_DOM_SEEDED_E = 7, CHACHA_DOM_GALOIS = 8, CHACHA_DOM_KSK_A = 9, CHACHA_DOM_KSK_E = 10, CHACHA_DOM_KSK_SEED = 11,
       CHACHA_DOM_FLOOD = 12 };

// Streams of the secret-key encryptor (crc_encrypt_sym* on the host, enc_sym_sample_kernel on the device: the same bits).  One stream per (ciphertext,
// coefficient pair), nonce = (stream id low, stream id high, CHACHA_DOM_ENC_SYM << 24 | even coefficient index s); its 32-bit words w[0], w[1], ... run
// through blocks 0, 1, ... (word j of block b is w[16 b + j]):
//   w[0..1], w[2..3]      noise magnitude words (low, high half) of coefficients s and s + 1: |e| = the number of the 19 thresholds of the clipped, truncated
//                         normal (crc_encrypt_dev_noise_thresholds) that the 64-bit word reaches
//   w[4]                  bit 0 / bit 1: e of coefficient s / s + 1 is negative;  w[5..7] unused
//   w[8 + 8 i + 4 c .. 11 + 8 i + 4 c]   the 128-bit integer z = w[+0] + 2^32 w[+1] + 2^64 w[+2] + 2^96 w[+3]: the NTT-form residue of c1 under modulus i in
//                         slot s + c (c = 0, 1) is z mod q_i (within q_i / 2^128 < 2^-66 of uniform)
// i.e. k / 2 + 1 blocks: one at k = 1, two at k = 2 or 3; modulus i reads the upper half of block i / 2 (i even) or the lower half of block (i + 1) / 2 (i odd)
#define CHACHA_SYM_BLOCK(i) (((i) + 1) >> 1)
#define CHACHA_SYM_WORD(i) (((i) & 1) ? 0 : 8)

// Streams of a SEEDED secret-key ciphertext (crc_encrypt_sym_seeded* / crc_seeded_expand on the host, seeded_expand_kernel on the device): c1 = A is a function
// of a PUBLIC seed, so the client ships the c0 rows and the seed and the server regenerates c1.  Two independent sources, two keys:
//   mask stream, PUBLIC seed, CHACHA_DOM_SEEDED_A: one stream per (ciphertext, coefficient pair), nonce = (stream id low, stream id high,
//                         CHACHA_DOM_SEEDED_A << 24 | even slot index s).  Block j serves modulus 2j with its words 0..7 and modulus 2j + 1 with its words 8..15;
//                         within a half, words 4c .. 4c + 3 are the 128-bit integer z (little-endian words) and A[i][s + c] = z mod q_i, c = 0, 1:
//                         (k + 1) / 2 blocks per pair, and no word of them depends on anything secret
//   noise stream, PRIVATE key, CHACHA_DOM_SEEDED_E: one block (counter 0) per (ciphertext, coefficient pair), nonce = (stream id low, stream id high,
//                         CHACHA_DOM_SEEDED_E << 24 | s); words 0..4 as block 0 of CHACHA_DOM_ENC_SYM (magnitude words of coefficients s, s + 1, sign bits in w[4])
// The noise has a domain of its own, not CHACHA_DOM_ENC_SYM: one private key serving crc_encrypt_sym_key and the seeded encryptor at the same stream id would
// give equal e under different, known A -- for equal plaintexts c0 - c0' = -(A - A') s, the secret key.
#define CHACHA_SEEDED_BLOCKS(k) (((k) + 1) >> 1)

// Streams of a SEEDED key-switching key (crc_gen_keys_seeded* / crc_seeded_keys_expand on the host, seeded_keys_device.h on the device).  A key-switching key is
// a list of pairs (first, second) with second = A uniform, so, as for a seeded ciphertext, A is a function of a PUBLIC seed and only the first rows travel.
// A key id is 0 for the evaluation key (target w = s^2) or a valid Galois element g (target w = sigma_g(s)); no valid element is even, so 0 is free.  The pairs of
// a blob are numbered in the blob's own order, p = Sum_{l' < l} L_l' + d (modulus l, digit d), P = Sum_l L_l of them; the seeded form of one key is its P first
// polynomials [P][k][n], NTT form: half the blob.  One stream per (id, pair, even slot s), nonce = (id, p | dbc << 16 | k << 24, domain << 24 | s):
//   mask stream, PUBLIC seed, CHACHA_DOM_KSK_A: blocks and words exactly as CHACHA_DOM_SEEDED_A -- block j serves modulus 2j with its words 0..7 and modulus
//                         2j + 1 with its words 8..15, the 128-bit z of words 4c .. 4c + 3 gives second[i][s + c] = z mod q_i
//   noise stream, PRIVATE key, CHACHA_DOM_KSK_E: one block (counter 0), words 0..4 as block 0 of CHACHA_DOM_ENC_SYM (two magnitude words against the 19
//                         thresholds, sign bits in w[4]); e is a coefficient-form polynomial, the same integer under every modulus
// and, in NTT form and pointwise,  first[j] = -(A[j] s[j] + NTT_j(e)) + [j == l] factor_{l,d} w[j],  factor_{l,d} = (q / q_l) 2^(dbc d) mod q_l.
// Two domains and two keys for the reason given above for SEEDED_A / SEEDED_E.  dbc and k are in the nonce because the streams are counter-based: without them one
// private key serving the same id at two digit widths, or on a context and on a prefix of its moduli, would give equal A and equal e around DIFFERENT known
// factors, and first - first' = (factor - factor') sigma_g(s) would reveal the secret key.
// Nothing in these nonces is per call, so whoever holds a private key must pair it with ONE public seed for as long as it lives: the host classes take the seed
// from the private (master) key itself -- bytes 0..31 of block 0 of the stream nonce = (0, 0, CHACHA_DOM_KSK_SEED << 24), a PRF output that can be published --
// so that an element generated twice is the same key twice.
#define CHACHA_KSK_NONCE1(p, dbc, k) ((uint32_t)(p) | ((uint32_t)(dbc) << 16) | ((uint32_t)(k) << 24))

// Streams of the noise flood (crc_flood* on the host, flood_sample_kernel on the device: the same bits).  One stream per (ciphertext, coefficient pair), nonce =
// (stream id low, stream id high, CHACHA_DOM_FLOOD << 24 | even coefficient index s), ONE block (counter 0).  Coefficient s + c (c = 0, 1) owns words
// w[8 c .. 8 c + 7] of it:
//   w[8c + 0 .. 1]        the ternary sample u: the 64-bit word as 2-bit fields from the low end, the first field that is not 3 (0, 1, 2 stand for 0, 1, -1; all
//                         32 fields equal to 3 gives 0) -- the public-key encryptor's rule
//   w[8c + 2 .. 3]        the magnitude word of e2 (low, high half): |e2| = the number of the 19 thresholds (crc_encrypt_dev_noise_thresholds) that it reaches
//   w[8c + 4 .. 7]        the 128-bit integer X = w[+4] + 2^32 w[+5] + 2^64 w[+6] + 2^96 w[+7]:  x = X mod 2^(B + 1) (its low B + 1 bits, B = flood_bits <= 126) and
//                         e1 = x - 2^B, uniform on [-2^B, 2^B);  bit 127 of X (the top bit of w[8c + 7]), which no x reaches, is the sign of e2 (set: negative)
// A reused (key, stream id) gives the same u, e1 and e2 twice: the difference of the two floods is then exactly the difference of the two inputs.
