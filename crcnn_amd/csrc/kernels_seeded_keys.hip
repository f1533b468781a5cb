// kernels_seeded_keys.hip -- seeded key-switching keys on gfx950: the first rows of evaluation and Galois keys made on the device, and their expansion into
// ordinary key blobs.  The kernel bodies are seeded_keys_device.h (they also run on the CPU under sanitizers); the keystreams are chacha.h's CHACHA_DOM_KSK_*.
//
// Generation is the seeded encryptor's three steps (k_encrypt_sym_seeded) over the n_ids P rows as over size-1 "ciphertexts", in place and without work space:
// a sample kernel writes e, the row transform runs, a finish kernel regenerates A in registers and adds the gadget term from the secret key's own rows -- the
// target sigma_g(s) is a gather of s through pi_g, s^2 a product.  Ids travel by value, KSK_IDS_MAX per launch.
#include "kernels.h"
#include "seeded_keys_device.h"

__global__ void __launch_bounds__(256) ksk_sample_kernel(KskArgs a, KskCdt T) { ksk_sample_body(a, T); }
__global__ void __launch_bounds__(256) ksk_finish_kernel(KskArgs a) { ksk_finish_body(a); }
template <bool CONJ>
__global__ void __launch_bounds__(256) ksk_expand_kernel(KskArgs a) { ksk_expand_body<CONJ>(a); }
template <bool CONJ>
__global__ void __launch_bounds__(256) ksk_expand_level_kernel(KskArgs a, KskLevel lv) { ksk_expand_level_body<CONJ>(a, lv); }
__global__ void __launch_bounds__(256) ksk_restrict_kernel(KskArgs a, KskLevel lv) { ksk_restrict_body(a, lv); }

void k_encrypt_cdt(u64 *out19);                            // (kernels_client.hip)

struct KskGrid { int threads, pblocks; };
static KskGrid ksk_grid(const crc_ctx *c)
{
    const int pairs = c->n / 2, threads = pairs < 256 ? pairs : 256;
    return {threads, (pairs + threads - 1) / threads};
}
static KskArgs ksk_args(const crc_ctx *c, int dbc, const ChaChaKey &key)
{
    KskArgs a{};
    a.mods = c->d_mods; a.n = c->n; a.logn = c->logn; a.k = c->k; a.dbc = dbc; a.key = key;
    a.P = evk_gadget(c, dbc, a.L, a.qhat);
    return a;
}
// every launch's grid fits: the largest is one chunk of ids; the row transform counts n_ids P k rows
bool k_seeded_keys_grid_ok(const crc_ctx *c, int dbc, int n_ids)
{
    const size_t P = crc_evk_words(c, dbc) / (2 * (size_t)c->k * c->n);
    return (size_t)KSK_IDS_MAX * P * ksk_grid(c).pblocks <= 0x7fffffffULL && (size_t)n_ids * P * c->k <= 0x7fffffffULL;
}

// first [n_ids][P][k][n] <- the first rows of the keys `ids` (host array) under (private key, public seed); the caller has checked ids, dbc, pointers, grids
int k_gen_keys_seeded(crc_ctx *c, const u64 *sk, int dbc, const u64 *ids, int n_ids, const ChaChaKey &key, const ChaChaKey &seed, u64 *first, hipStream_t st)
{
    if (n_ids == 0) return CRC_OK;
    const KskGrid g = ksk_grid(c);
    KskArgs a = ksk_args(c, dbc, key);
    a.sk = sk;
    const size_t per_id = (size_t)a.P * c->k * c->n;
    KskCdt T; k_encrypt_cdt(T.t);
    for (int e0 = 0; e0 < n_ids; e0 += KSK_IDS_MAX) {
        a.n_ids = n_ids - e0 < KSK_IDS_MAX ? n_ids - e0 : KSK_IDS_MAX;
        for (int e = 0; e < a.n_ids; e++) a.id[e] = ids[e0 + e];
        a.first = first + (size_t)e0 * per_id;
        hipLaunchKernelGGL(ksk_sample_kernel, dim3((unsigned)((size_t)a.n_ids * a.P * g.pblocks)), dim3(g.threads), 0, st, a, T);
        HIPCHK(hipGetLastError());
    }
    // the rows are n_ids P size-1 "ciphertexts" of k rows: transformed in place
    { const int rc = k_ntt_ct(c, false, first, first, (size_t)n_ids * a.P, 1, false, st, nullptr, 0, 0, 0); if (rc) return rc; }
    a.key = seed;
    for (int e0 = 0; e0 < n_ids; e0 += KSK_IDS_MAX) {
        a.n_ids = n_ids - e0 < KSK_IDS_MAX ? n_ids - e0 : KSK_IDS_MAX;
        for (int e = 0; e < a.n_ids; e++) a.id[e] = ids[e0 + e];
        a.first = first + (size_t)e0 * per_id;
        hipLaunchKernelGGL(ksk_finish_kernel, dim3((unsigned)((size_t)a.n_ids * a.P * g.pblocks)), dim3(g.threads), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// rows [n_ids][P][k][n] -> blobs [n_ids][crc_evk_words]; conjugate: the blobs of crc_galois_conjugate_keys, in the one pass
int k_seeded_keys_expand(crc_ctx *c, const u64 *rows, const u64 *ids, int n_ids, int dbc, const ChaChaKey &seed, bool conjugate, u64 *out, hipStream_t st)
{
    if (n_ids == 0) return CRC_OK;
    const KskGrid g = ksk_grid(c);
    KskArgs a = ksk_args(c, dbc, seed);
    const size_t per_id = (size_t)a.P * c->k * c->n;
    for (int e0 = 0; e0 < n_ids; e0 += KSK_IDS_MAX) {
        a.n_ids = n_ids - e0 < KSK_IDS_MAX ? n_ids - e0 : KSK_IDS_MAX;
        for (int e = 0; e < a.n_ids; e++) a.id[e] = ids[e0 + e];
        a.rows = rows + (size_t)e0 * per_id; a.out = out + (size_t)e0 * 2 * per_id;
        const dim3 grid((unsigned)((size_t)a.n_ids * a.P * g.pblocks));
        if (conjugate) hipLaunchKernelGGL(ksk_expand_kernel<true>, grid, dim3(g.threads), 0, st, a);
        else hipLaunchKernelGGL(ksk_expand_kernel<false>, grid, dim3(g.threads), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// ---- levels: keys of `from` -> keys of `to`, a level of it (keys_level_of: the caller has checked that, the pointers, dbc and the grids of BOTH contexts) ------
// the lanes and the destination strides are `to`'s, the source strides `from`'s; the streams carry the gadget's modulus count
static KskArgs ksk_level_args(const crc_ctx *from, const crc_ctx *to, int dbc, const ChaChaKey &key, KskLevel &lv)
{
    KskArgs a = ksk_args(to, dbc, key);
    lv.name_k = (int)from->key_q.size(); lv.src_k = from->k;
    lv.src_P = (int)(crc_evk_words(from, dbc) / (2 * (size_t)from->k * from->n));
    return a;
}
// blobs [n_keys][crc_evk_words(from)] -> [n_keys][crc_evk_words(to)]: pairs p < P(to), rows j < to->k of both polynomials
int k_keys_restrict(crc_ctx *from, const crc_ctx *to, const u64 *keys, int n_keys, int dbc, u64 *out, hipStream_t st)
{
    if (n_keys == 0) return CRC_OK;
    const KskGrid g = ksk_grid(to);
    KskLevel lv;
    KskArgs a = ksk_level_args(from, to, dbc, ChaChaKey{}, lv);
    a.mods = nullptr;                                                   // (no arithmetic: `to` may be a host-only context)
    const size_t in_w = crc_evk_words(from, dbc), out_w = crc_evk_words(to, dbc);
    for (int e0 = 0; e0 < n_keys; e0 += KSK_IDS_MAX) {
        a.n_ids = n_keys - e0 < KSK_IDS_MAX ? n_keys - e0 : KSK_IDS_MAX;
        a.rows = keys + (size_t)e0 * in_w; a.out = out + (size_t)e0 * out_w;
        hipLaunchKernelGGL(ksk_restrict_kernel, dim3((unsigned)((size_t)a.n_ids * a.P * g.pblocks)), dim3(g.threads), 0, st, a, lv);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}
// from's rows [n_ids][P(from)][from->k][n] -> to's blobs [n_ids][crc_evk_words(to)]: k_keys_restrict of k_seeded_keys_expand, without the blobs of `from`.
// The moduli of the rows written are a prefix of from's, so from's device table serves
int k_seeded_keys_expand_level(crc_ctx *from, const crc_ctx *to, const u64 *rows, const u64 *ids, int n_ids, int dbc, const ChaChaKey &seed, bool conjugate, u64 *out,
                               hipStream_t st)
{
    if (n_ids == 0) return CRC_OK;
    const KskGrid g = ksk_grid(to);
    KskLevel lv;
    KskArgs a = ksk_level_args(from, to, dbc, seed, lv);
    a.mods = from->d_mods;
    const size_t in_w = (size_t)lv.src_P * from->k * from->n, out_w = crc_evk_words(to, dbc);
    for (int e0 = 0; e0 < n_ids; e0 += KSK_IDS_MAX) {
        a.n_ids = n_ids - e0 < KSK_IDS_MAX ? n_ids - e0 : KSK_IDS_MAX;
        for (int e = 0; e < a.n_ids; e++) a.id[e] = ids[e0 + e];
        a.rows = rows + (size_t)e0 * in_w; a.out = out + (size_t)e0 * out_w;
        const dim3 grid((unsigned)((size_t)a.n_ids * a.P * g.pblocks));
        if (conjugate) hipLaunchKernelGGL(ksk_expand_level_kernel<true>, grid, dim3(g.threads), 0, st, a, lv);
        else hipLaunchKernelGGL(ksk_expand_level_kernel<false>, grid, dim3(g.threads), 0, st, a, lv);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}
