// CPU check of the seeded key kernels' own text (crcnn_amd/csrc/seeded_keys_device.h: the bodies of ksk_sample_kernel, ksk_finish_kernel and both forms of
// ksk_expand_kernel, with chacha.h and the device form of the 64-bit products) against the library's host twins crc_gen_keys_seeded_key and
// crc_seeded_keys_expand, bit for bit: one thread per workgroup over each launch's whole grid (and a few blocks past it), the row transform between the two
// generation kernels done with ntt_device.h's passes as the library's row kernel does it.  Built with -fsanitize=address,undefined
// (tests/test_seeded_keys_cpu.py): every buffer has exactly the documented number of words, so an access past a row or a blob is an error the sanitizer reports.
//   seeded_keys_kernel_check <n> <dbc> <q_0> ... <q_{k-1}>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CRC_FORCE_MAD_MUL 1
#include "seeded_keys_device.h"
#include "../../include/crcnn_hip.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
typedef unsigned __int128 u128;
static u64 shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }

static int evk_digits(u64 q, int dbc) { int L = 0; while (q) { L++; q >>= dbc; } return L; }

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int n = atoi(argv[1]), dbc = atoi(argv[2]), k = argc - 3;
    std::vector<u64> q(k);
    for (int i = 0; i < k; i++) q[i] = strtoull(argv[3 + i], 0, 0);
    int logn = 0; while ((1 << logn) < n) logn++;
    crc_ctx *C;
    if (crc_ctx_create(n, q.data(), k, 65537, -1, &C)) { puts("FAILED context"); return 2; }

    std::vector<ModParams> mods(k);
    for (int i = 0; i < k; i++) {
        const u128 all = ~(u128)0; u128 r = all / q[i]; if (all % q[i] == q[i] - 1) r++;       // floor(2^128 / q)
        ModParams &m = mods[i];
        m.q = q[i]; m.r0 = (u64)r; m.r1 = (u64)(r >> 64); m.two_q = 2 * q[i]; m.bits = 64 - __builtin_clzll(q[i]); m.fold = fold_constant(q[i], m.bits);
    }
    std::vector<ulonglong2> fw((size_t)k * n);
    {
        std::vector<u64> tab(n);
        for (int i = 0; i < k; i++) {
            char name[64]; snprintf(name, sizeof name, "root_powers:%d", i);
            if (crc_ctx_table(C, name, tab.data(), n) != n) { puts("FAILED table"); return 2; }
            for (int s = 0; s < n; s++) fw[(size_t)i * n + s] = {tab[s], shoup(tab[s], q[i])};
        }
    }
    const size_t kn = (size_t)k * n;
    std::vector<u64> sk(kn), pk(2 * kn);
    if (crc_keygen(C, 5, sk.data(), pk.data())) { puts("FAILED keygen"); return 2; }

    KskArgs a; memset(&a, 0, sizeof a);
    a.mods = mods.data(); a.n = n; a.logn = logn; a.k = k; a.dbc = dbc;
    for (int l = 0; l < k; l++) {
        a.L[l] = evk_digits(q[l], dbc); a.P += a.L[l];
        u64 f = 1; for (int j = 0; j < k; j++) if (j != l) f = (u64)((u128)f * (q[j] % q[l]) % q[l]);
        a.qhat[l] = f;
    }
    const size_t P = (size_t)a.P;
    if (crc_seeded_key_words(C, dbc) != P * kn || crc_evk_words(C, dbc) != 2 * P * kn) { puts("FAILED sizes"); return 2; }
    uint8_t key[32], seed[32];
    for (int i = 0; i < 32; i++) { key[i] = (uint8_t)(17 * i + 3); seed[i] = (uint8_t)(201 - 5 * i); }
    KskCdt T; crc_encrypt_dev_noise_thresholds(T.t);

    const u64 ids[4] = {0, 1, 3, 2 * (u64)n - 1};
    const int n_ids = 4;
    std::vector<u64> want(n_ids * P * kn), got(n_ids * P * kn, ~0ull), sm(n);
    if (crc_gen_keys_seeded_key(C, key, seed, sk.data(), dbc, ids, n_ids, want.data())) { puts("FAILED host twin"); return 2; }
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1);
    a.n_ids = n_ids; for (int e = 0; e < n_ids; e++) a.id[e] = ids[e];
    a.first = got.data(); a.sk = sk.data();
    const unsigned grid = (unsigned)(n_ids * P * (n / 2));
    a.key = chacha_load_key(key);
    for (unsigned b = 0; b < grid + 3; b++) { blockIdx = dim3(b); ksk_sample_body(a, T); }             // (+ 3: blocks past the rows return at once)
    for (size_t r = 0; r < n_ids * P * k; r++) {                                                    // the row transform, strict butterflies
        const int i = (int)(r % k); u64 *row = got.data() + r * n;
        for (int s = 0; s < n; s += 2) sm_store_pair64(sm.data(), s, row[s], row[s + 1]);
        ntt_row_passes<false, false, 3, false>(sm.data(), fw.data() + (size_t)i * n, n, logn, q[i], 2 * q[i]);
        const u64 one_s = shoup(1, q[i]);
        for (int s = 0; s < n; s += 2) { const ulonglong2 v = sm_load_pair64(sm.data(), s); row[s] = mulmod_shoup(v.x, 1, one_s, q[i]); row[s + 1] = mulmod_shoup(v.y, 1, one_s, q[i]); }
    }
    a.key = chacha_load_key(seed);
    for (unsigned b = 0; b < grid + 3; b++) { blockIdx = dim3(b); ksk_finish_body(a); }
    int bad = 0;
    if (memcmp(want.data(), got.data(), want.size() * 8)) { puts("FAILED generation differs from the host twin"); bad = 1; }

    // expansion of the host twin's rows: every id plain, the elements other than 1 conjugated
    for (int conj = 0; conj < 2; conj++) {
        const int e0 = conj ? 2 : 0, cnt = n_ids - e0;
        std::vector<u64> bw((size_t)cnt * 2 * P * kn), bg((size_t)cnt * 2 * P * kn, ~0ull);
        if (crc_seeded_keys_expand(C, want.data() + e0 * P * kn, ids + e0, cnt, dbc, seed, conj, bw.data())) { puts("FAILED host expand"); return 2; }
        a.n_ids = cnt; for (int e = 0; e < cnt; e++) a.id[e] = ids[e0 + e];
        a.first = nullptr; a.sk = nullptr; a.rows = want.data() + e0 * P * kn; a.out = bg.data();
        const unsigned g2 = (unsigned)(cnt * P * (n / 2));
        for (unsigned b = 0; b < g2 + 3; b++) { blockIdx = dim3(b); if (conj) ksk_expand_body<true>(a); else ksk_expand_body<false>(a); }
        if (memcmp(bw.data(), bg.data(), bw.size() * 8)) { printf("FAILED expansion conjugate=%d differs from the host twin\n", conj); bad = 1; }
    }
    // ids 0 and 1 have no conjugated key
    { std::vector<u64> o(2 * 2 * P * kn); if (crc_seeded_keys_expand(C, want.data(), ids, 2, dbc, seed, 1, o.data()) == 0) { puts("FAILED: conjugate of id 0 / 1 accepted"); bad = 1; } }
    if (bad) return 1;
    printf("ok n=%d k=%d dbc=%d P=%zu\n", n, k, dbc, P);
    crc_ctx_destroy(C);
    return 0;
}
