// CPU check of the level kernels' own text (crcnn_amd/csrc/seeded_keys_device.h: ksk_restrict_body and both forms of ksk_expand_level_body) against the
// library's host twins crc_keys_restrict and crc_seeded_keys_expand_level, bit for bit: one thread per workgroup over each launch's whole grid (and a few blocks
// past it).  Built with -fsanitize=address,undefined (tests/test_level_keys_cpu.py): every buffer has exactly the documented number of words -- the parent's
// blobs and rows at the parent's sizes, the level's blobs at the level's --, so an access past either is an error the sanitizer reports.
//   level_keys_kernel_check <n> <dbc> <kept> <q_0> ... <q_{k-1}>
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

static int evk_digits(u64 q, int dbc) { int L = 0; while (q) { L++; q >>= dbc; } return L; }

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int n = atoi(argv[1]), dbc = atoi(argv[2]), kept = atoi(argv[3]), k = argc - 4;
    std::vector<u64> q(k);
    for (int i = 0; i < k; i++) q[i] = strtoull(argv[4 + i], 0, 0);
    int logn = 0; while ((1 << logn) < n) logn++;
    crc_ctx *A, *B;
    if (crc_ctx_create(n, q.data(), k, 65537, -1, &A) || crc_ctx_create_level(A, kept, -1, &B)) { puts("FAILED context"); return 2; }
    if (!crc_keys_restrict_supported(A, B) || crc_ctx_key_moduli(B) != k || crc_ctx_k(B) != kept) { puts("FAILED level"); return 2; }

    std::vector<ModParams> mods(k);
    for (int i = 0; i < k; i++) {
        const u128 all = ~(u128)0; u128 r = all / q[i]; if (all % q[i] == q[i] - 1) r++;       // floor(2^128 / q)
        ModParams &m = mods[i];
        m.q = q[i]; m.r0 = (u64)r; m.r1 = (u64)(r >> 64); m.two_q = 2 * q[i]; m.bits = 64 - __builtin_clzll(q[i]); m.fold = fold_constant(q[i], m.bits);
    }
    const size_t skn = (size_t)k * n, kn = (size_t)kept * n;
    std::vector<u64> sk(skn), pk(2 * skn);
    if (crc_keygen(A, 5, sk.data(), pk.data())) { puts("FAILED keygen"); return 2; }

    // the lanes and the destination are the level's, the source strides and the stream names the parent's
    KskArgs a; memset(&a, 0, sizeof a);
    a.mods = mods.data(); a.n = n; a.logn = logn; a.k = kept; a.dbc = dbc;
    int sP = 0;
    for (int l = 0; l < k; l++) { const int L = evk_digits(q[l], dbc); sP += L; if (l < kept) { a.L[l] = L; a.P += L; } }
    const KskLevel lv{k, k, sP};
    const size_t P = (size_t)a.P, in_w = 2 * (size_t)sP * skn, out_w = 2 * P * kn;
    if (crc_evk_words(A, dbc) != in_w || crc_evk_words(B, dbc) != out_w) { puts("FAILED sizes"); return 2; }
    uint8_t key[32], seed[32];
    for (int i = 0; i < 32; i++) { key[i] = (uint8_t)(17 * i + 3); seed[i] = (uint8_t)(201 - 5 * i); }

    const u64 ids[4] = {0, 1, 3, 2 * (u64)n - 1};
    const int n_ids = 4;
    std::vector<u64> rows((size_t)n_ids * sP * skn), blobs((size_t)n_ids * in_w);
    if (crc_gen_keys_seeded_key(A, key, seed, sk.data(), dbc, ids, n_ids, rows.data())) { puts("FAILED generation"); return 2; }
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1);
    int bad = 0;
    for (int conj = 0; conj < 2; conj++) {
        const int e0 = conj ? 2 : 0, cnt = n_ids - e0;
        if (crc_seeded_keys_expand(A, rows.data() + (size_t)e0 * sP * skn, ids + e0, cnt, dbc, seed, conj, blobs.data())) { puts("FAILED host expand"); return 2; }
        std::vector<u64> in(blobs.begin(), blobs.begin() + (size_t)cnt * in_w);                      // exactly cnt blobs of the parent
        std::vector<u64> want((size_t)cnt * out_w), got((size_t)cnt * out_w, ~0ull), lw((size_t)cnt * out_w), lg((size_t)cnt * out_w, ~0ull);
        std::vector<u64> rin(rows.begin() + (size_t)e0 * sP * skn, rows.begin() + (size_t)(e0 + cnt) * sP * skn);
        if (crc_keys_restrict(A, B, in.data(), cnt, dbc, want.data())) { puts("FAILED host restrict"); return 2; }
        if (crc_seeded_keys_expand_level(A, B, rin.data(), ids + e0, cnt, dbc, seed, conj, lw.data())) { puts("FAILED host level expand"); return 2; }
        if (memcmp(want.data(), lw.data(), want.size() * 8)) { printf("FAILED host level expand conjugate=%d is not restrict(expand)\n", conj); bad = 1; }
        const unsigned grid = (unsigned)(cnt * P * (n / 2));
        a.n_ids = cnt; for (int e = 0; e < cnt; e++) a.id[e] = ids[e0 + e];
        a.rows = in.data(); a.out = got.data();
        for (unsigned b = 0; b < grid + 3; b++) { blockIdx = dim3(b); ksk_restrict_body(a, lv); }        // (+ 3: blocks past the rows return at once)
        if (memcmp(want.data(), got.data(), want.size() * 8)) { printf("FAILED restriction conjugate=%d differs from the host twin\n", conj); bad = 1; }
        a.rows = rin.data(); a.out = lg.data(); a.key = chacha_load_key(seed);
        for (unsigned b = 0; b < grid + 3; b++) { blockIdx = dim3(b); if (conj) ksk_expand_level_body<true>(a, lv); else ksk_expand_level_body<false>(a, lv); }
        if (memcmp(lw.data(), lg.data(), lw.size() * 8)) { printf("FAILED level expansion conjugate=%d differs from the host twin\n", conj); bad = 1; }
    }
    if (bad) return 1;
    printf("ok n=%d k=%d kept=%d dbc=%d P=%zu of %d\n", n, k, kept, dbc, P, sP);
    crc_ctx_destroy(A); crc_ctx_destroy(B);
    return 0;
}
