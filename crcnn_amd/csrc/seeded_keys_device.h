// seeded_keys_device.h -- device side of the seeded key-switching keys (kernels_seeded_keys.hip): the bodies of the four kernels.  A header so that
// tests/cpp/seeded_keys_kernel_check.cpp can run the same text on the CPU, one thread per workgroup, under sanitizers.
//
// Streams, pair numbering and the definition of a first row: chacha.h (CHACHA_DOM_KSK_A / CHACHA_DOM_KSK_E); the host twin is crc_gen_keys_seeded_key /
// crc_seeded_keys_expand (client.cpp).  One lane = one (key id, pair p, slot pair (s, s + 1)), as the seeded encryptor's lanes (kernels_client.hip): every
// access to a row is 16 bytes wide except the gathers and scatters through pi_g, which are 8.  A launch serves up to KSK_IDS_MAX ids, which travel by value.
//
// Levels (crc_ctx_create_level): a key over the gadget of Q = q_0 .. q_{K-1} serves the level q_0 .. q_{k'-1} as its first P' = Sum_{l < k'} L_l pairs, rows
// [0, k') of each polynomial.  ksk_restrict_body selects those words of expanded blobs; ksk_expand_level_body is ksk_expand_body writing them directly.  In both
// KskArgs describes the DESTINATION (k, P, the lanes) and KskLevel the source; KskArgs itself is unchanged, for the callers that fill it field by field.
#pragma once
#include "ntt_device.h"
#include "chacha.h"

#ifndef CRC_MAXK
#define CRC_MAXK 8
#endif
#define KSK_IDS_MAX 32

struct KskCdt { u64 t[19]; };                              // the thresholds of crc_encrypt_dev_noise_thresholds
struct KskArgs {
    u64 *first;                                            // generation: the rows [n_ids][P][k][n] of this launch's ids, formed in place
    const u64 *sk;                                         // generation: the secret key [k][n], NTT form
    const u64 *rows;                                       // expansion: the first rows [n_ids][P][k][n]
    u64 *out;                                              // expansion: the blobs [n_ids][P][2][k][n]
    const ModParams *mods;
    int n, logn, k, dbc, P, n_ids;
    int L[CRC_MAXK];                                       // digits per modulus: pair p = Sum_{l' < l} L[l'] + d
    u64 qhat[CRC_MAXK];                                    // (q / q_l) mod q_l
    u64 id[KSK_IDS_MAX];
    ChaChaKey key;                                         // sample kernel: the PRIVATE key; finish and expansion kernels: the PUBLIC seed
};
// The source of an expansion into a level, or of a restriction: KskArgs.rows then holds src_P pairs of src_k rows per key, and the streams are named with name_k,
// the modulus count of the gadget the keys were generated over.  KskArgs.k and .P are the level's: the rows written and the pairs the lanes cover
struct KskLevel { int name_k, src_k, src_P; };

__device__ __forceinline__ u32 ksk_brev(u32 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    u32 r = 0;
    for (int b = 0; b < 32; b++) r |= ((v >> b) & 1u) << (31 - b);
    return r;
#endif
}
// pi_g(i): NTT(sigma_g(p))[i] = NTT(p)[pi_g(i)]  (what galois_permute_ntt_kernel computes and crc_galois_ntt_table tabulates); below n for every i < n
__device__ __forceinline__ u32 ksk_ntt_src(u32 i, u32 g, u32 m2, int sh)
{
    const u32 e = (g * (2u * (ksk_brev(i) >> sh) + 1u)) & m2;
    return ksk_brev(e >> 1) >> sh;
}
// z = hi 2^64 + lo -> z mod q for ANY 128-bit z (the generic Barrett path wants z < 2^64 q: the high word is reduced first there)
__device__ __forceinline__ u64 ksk_mod128(u64 lo, u64 hi, const ModParams &m)
{
    if (m.fold) return fold128(lo, hi, m);
    return barrett128(lo, barrett128(hi, 0, m), m);
}
// the lane's place: e (index into a.id), pair p, even slot s.  false: a lane past the row
__device__ __forceinline__ bool ksk_lane(const KskArgs &a, int &e, int &p, int &s)
{
    const int pairs = a.n >> 1, pblocks = (pairs + (int)blockDim.x - 1) / (int)blockDim.x;
    const unsigned m = blockIdx.x / (unsigned)pblocks;     // e P + p
    const int pr = (int)(blockIdx.x % (unsigned)pblocks) * (int)blockDim.x + (int)threadIdx.x;
    e = (int)(m / (unsigned)a.P); p = (int)(m % (unsigned)a.P); s = 2 * pr;
    return pr < pairs && e < a.n_ids;
}
// the two residues of A under modulus i from the eight keystream words w
__device__ __forceinline__ ulonglong2 ksk_mask2(const u32 *w, const ModParams &md)
{
    return ulonglong2{ksk_mod128((u64)w[0] | ((u64)w[1] << 32), (u64)w[2] | ((u64)w[3] << 32), md),
                      ksk_mod128((u64)w[4] | ((u64)w[5] << 32), (u64)w[6] | ((u64)w[7] << 32), md)};
}

// ---- generation, step 1: e, reduced per modulus, into the first rows (coefficient form; the row transform runs next) --------------------------------------------
__device__ __forceinline__ void ksk_sample_body(const KskArgs &a, const KskCdt &T)
{
    int e, p, s;
    if (!ksk_lane(a, e, p, s)) return;
    u32 b[16];
    chacha20_block(a.key, 0, (u32)a.id[e], CHACHA_KSK_NONCE1(p, a.dbc, a.k), ((u32)CHACHA_DOM_KSK_E << 24) | (u32)s, b);
    int ev[2];
#pragma unroll
    for (int x = 0; x < 2; x++) {
        const u64 w = (u64)b[2 * x] | ((u64)b[2 * x + 1] << 32);
        int mag = 0;
#pragma unroll
        for (int j = 0; j < 19; j++) mag += w >= T.t[j] ? 1 : 0;
        ev[x] = (b[4] >> x) & 1u ? -mag : mag;
    }
    u64 *dst = a.first + ((size_t)e * a.P + p) * ((size_t)a.k * a.n) + s;
    for (int i = 0; i < a.k; i++) {
        const u64 q = a.mods[i].q;
        st2(dst + (size_t)i * a.n, ev[0] >= 0 ? (u64)ev[0] : q - (u64)(-ev[0]), ev[1] >= 0 ? (u64)ev[1] : q - (u64)(-ev[1]));
    }
}

// ---- generation, step 3: over the TRANSFORMED rows, first <- -(A s + first) + [j == l] factor w, A regenerated in registers ------------------------------------
__device__ __forceinline__ void ksk_finish_body(const KskArgs &a)
{
    int e, p, s;
    if (!ksk_lane(a, e, p, s)) return;
    const u64 id = a.id[e];
    int l = 0, d = p;
    while (d >= a.L[l]) { d -= a.L[l]; l++; }              // p < P = Sum L: l stays below k
    const u32 n1 = CHACHA_KSK_NONCE1(p, a.dbc, a.k), n2 = ((u32)CHACHA_DOM_KSK_A << 24) | (u32)s;
    const u32 m2 = 2u * (u32)a.n - 1u; const int sh = 32 - a.logn;
    u64 *row = a.first + ((size_t)e * a.P + p) * ((size_t)a.k * a.n) + s;
    u32 b[16];
    auto emit = [&](int j, const u32 *w) {
        const ModParams md = a.mods[j];
        const u64 *skj = a.sk + (size_t)j * a.n;
        const ulonglong2 A = ksk_mask2(w, md), v = ld2(row + (size_t)j * a.n), kv = ld2(skj + s);
        u64 r0 = negmod(addmod(mulmod(A.x, kv.x, md), v.x, md.q), md.q), r1 = negmod(addmod(mulmod(A.y, kv.y, md), v.y, md.q), md.q);
        if (j == l) {
            // 2^(dbc d) < 2^bits(q_l) <= 2 q_l: one subtraction reduces it
            u64 pw = (u64)1 << (a.dbc * d); if (pw >= md.q) pw -= md.q;
            const u64 factor = mulmod(a.qhat[l], pw, md);
            u64 w0, w1;
            if (id == 0) { w0 = mulmod(kv.x, kv.x, md); w1 = mulmod(kv.y, kv.y, md); }
            else { w0 = skj[ksk_ntt_src((u32)s, (u32)id, m2, sh)]; w1 = skj[ksk_ntt_src((u32)s + 1u, (u32)id, m2, sh)]; }
            r0 = addmod(r0, mulmod(w0, factor, md), md.q); r1 = addmod(r1, mulmod(w1, factor, md), md.q);
        }
        st2(row + (size_t)j * a.n, r0, r1);
    };
    for (int j = 0; 2 * j < a.k; j++) {
        chacha20_block(a.key, (u32)j, (u32)id, n1, n2, b);
        emit(2 * j, b);
        if (2 * j + 1 < a.k) emit(2 * j + 1, b + 8);
    }
}

// ---- expansion: pair p of a blob = (first row p, A) ----------------------------------------------------------------------------------------------------------
// CONJ = false: the blob K, both rows stored where they were read / generated.  CONJ = true: K' = sigma_g^-1(K), out[i] = K[pi_h(i)] with h = g^-1 -- the lane
// owns the SOURCE pair (s, s + 1), reads and generates it once, and stores each residue at the one index i with pi_h(i) = s, which is pi_g(s): 16-byte loads,
// 8-byte scattered stores into a row that the same few workgroups fill, and one keystream block per modulus pair as in the plain form.
// Into a level (lv.src_k > a.k): the lanes cover the level's P pairs, read rows at the source's strides and stop the block loop at the level's k -- the first k
// residues of a keystream are a prefix of it, so the words are those of the source's blob, restricted
template <bool CONJ>
__device__ __forceinline__ void ksk_expand_core(const KskArgs &a, const KskLevel lv)
{
    int e, p, s;
    if (!ksk_lane(a, e, p, s)) return;
    const u64 id = a.id[e];
    const u32 n1 = CHACHA_KSK_NONCE1(p, a.dbc, lv.name_k), n2 = ((u32)CHACHA_DOM_KSK_A << 24) | (u32)s;
    const size_t kn = (size_t)a.k * a.n;
    const u64 *src = a.rows + ((size_t)e * lv.src_P + p) * ((size_t)lv.src_k * a.n) + s;
    u64 *dst = a.out + ((size_t)e * a.P + p) * 2 * kn;
    u32 d0 = (u32)s, d1 = (u32)s + 1u;
    if (CONJ) { const u32 m2 = 2u * (u32)a.n - 1u; const int sh = 32 - a.logn; d0 = ksk_ntt_src((u32)s, (u32)id, m2, sh); d1 = ksk_ntt_src((u32)s + 1u, (u32)id, m2, sh); }
    u32 b[16];
    auto emit = [&](int i, const u32 *w) {
        const ModParams md = a.mods[i];
        const ulonglong2 v = ld2(src + (size_t)i * a.n), A = ksk_mask2(w, md);
        u64 *f = dst + (size_t)i * a.n, *g = f + kn;
        if (CONJ) { f[d0] = v.x; f[d1] = v.y; g[d0] = A.x; g[d1] = A.y; }
        else { st2(f + s, v.x, v.y); st2(g + s, A.x, A.y); }
    };
    for (int j = 0; 2 * j < a.k; j++) {
        chacha20_block(a.key, (u32)j, (u32)id, n1, n2, b);
        emit(2 * j, b);
        if (2 * j + 1 < a.k) emit(2 * j + 1, b + 8);
    }
}
template <bool CONJ>
__device__ __forceinline__ void ksk_expand_body(const KskArgs &a) { ksk_expand_core<CONJ>(a, KskLevel{a.k, a.k, a.P}); }
template <bool CONJ>
__device__ __forceinline__ void ksk_expand_level_body(const KskArgs &a, const KskLevel &lv) { ksk_expand_core<CONJ>(a, lv); }

// ---- restriction: blobs of a context -> blobs of one of its levels ------------------------------------------------------------------------------------------
// a.rows: the source blobs [n_ids][src_P][2][src_k][n].  Word (key e, pair p < P, polynomial, row j < k, slot) of the source goes to the same coordinates at the destination's strides; nothing is computed, so the same
// kernel serves evaluation keys, Galois keys and conjugated blobs (sigma_g^-1 acts inside a row).  16-byte loads and stores, 2 k of each per lane
__device__ __forceinline__ void ksk_restrict_body(const KskArgs &a, const KskLevel &lv)
{
    int e, p, s;
    if (!ksk_lane(a, e, p, s)) return;
    const size_t skn = (size_t)lv.src_k * a.n, kn = (size_t)a.k * a.n;
    const u64 *src = a.rows + ((size_t)e * lv.src_P + p) * 2 * skn + s;
    u64 *dst = a.out + ((size_t)e * a.P + p) * 2 * kn + s;
    for (int j = 0; j < a.k; j++) {
        const ulonglong2 f = ld2(src + (size_t)j * a.n), g = ld2(src + skn + (size_t)j * a.n);
        st2(dst + (size_t)j * a.n, f.x, f.y); st2(dst + kn + (size_t)j * a.n, g.x, g.y);
    }
}
