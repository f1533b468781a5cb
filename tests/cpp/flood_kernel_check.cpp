// CPU check of the noise-flooding kernels' own text (crcnn_amd/csrc/flood_device.h: the bodies of flood_sample_kernel and flood_join_kernel, with
// ntt_device.h's passes, the samplers of enc_sampler.h and the device form of the 64-bit products) against the library's host twin crc_flood, bit for bit, for
// both forms: one thread per workgroup over each launch's whole grid, the constants and the tables rebuilt here from the moduli and "root_powers:i" /
// "inv_root_powers_div_two:i".  The forward transform of the ternary rows, which the device runs through the library's row transform, is the plain butterfly
// loop on the same table here.  Built with -fsanitize=address,undefined (tests/test_flood_cpu.py): the tensor has exactly its words and the work space
// exactly the bytes crc_flood_dev_work_bytes states, so an access past a row, the work space or the LDS image is an error the sanitizer reports.
//   flood_kernel_check <n> <count> <flood_bits> <seed> <q_0> <q_1> ... <q_{k-1}>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CRC_FORCE_MAD_MUL 1
#include "flood_device.h"
#include "../../include/crcnn_hip.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
typedef unsigned __int128 u128;
static u64 mulm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); } return r; }
static u64 shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static u64 rnd() { return ((u64)rand() << 42) ^ ((u64)rand() << 21) ^ (u64)rand(); }

static ModParams mod_of(u64 q)
{
    ModParams m{};
    m.q = q; m.two_q = 2 * q; m.bits = 64 - __builtin_clzll(q); m.fold = fold_constant(q, m.bits);
    // floor(2^128 / q): the high word is floor(2^64 / q) (q is no power of two), the low word the quotient of the remainder shifted up
    const u128 top = ((u128)1 << 64) / q, rem = ((u128)1 << 64) % q;
    m.r1 = (u64)top; m.r0 = (u64)((rem << 64) / q);
    return m;
}
static void ntt_fwd_ref(u64 *a, const ulonglong2 *W, int n, u64 q)
{
    for (int t = n >> 1, m = 1; m < n; m <<= 1, t >>= 1)
        for (int i = 0; i < m; i++)
            for (int j = 2 * i * t; j < 2 * i * t + t; j++) { const u64 U = a[j], V = mulm(a[j + t], W[m + i].x, q); a[j] = (U + V) % q; a[j + t] = (U + q - V) % q; }
}

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int n = atoi(argv[1]); const size_t count = (size_t)atoi(argv[2]); const int B = atoi(argv[3]); const u64 seed = strtoull(argv[4], 0, 0);
    const int k = argc - 5;
    std::vector<u64> q(k);
    for (int i = 0; i < k; i++) q[i] = strtoull(argv[5 + i], 0, 0);
    int logn = 0; while ((1 << logn) < n) logn++;
    crc_ctx *A;
    if (k > CRC_MAXK || crc_ctx_create(n, q.data(), k, 65537, -1, &A) || !crc_flood_supported(A, B)) { puts("FAILED context"); return 2; }

    FloodArgs base{};
    base.count = count; base.n = n; base.logn = logn; base.k = k; base.flood_bits = B; base.stream_base = 0; base.key = chacha_seed_key(seed);
    crc_encrypt_dev_noise_thresholds(base.cdt.t);
    bool lazy = true;
    for (int i = 0; i < k; i++) { base.mods[i] = mod_of(q[i]); base.one_s[i] = shoup(1, q[i]); base.pow2b[i] = powm(2, (u64)B, q[i]); lazy = lazy && base.mods[i].bits <= 57; }
    std::vector<ulonglong2> fw((size_t)k * n), iv((size_t)k * n);
    {
        std::vector<u64> tab(n);
        for (int i = 0; i < k; i++) {
            char name[64];
            snprintf(name, sizeof name, "root_powers:%d", i);
            if (crc_ctx_table(A, name, tab.data(), n) != n) { puts("FAILED table"); return 2; }
            for (int s = 0; s < n; s++) fw[(size_t)i * n + s] = {tab[s], shoup(tab[s], q[i])};
            snprintf(name, sizeof name, "inv_root_powers_div_two:%d", i);
            if (crc_ctx_table(A, name, tab.data(), n) != n) { puts("FAILED table"); return 2; }
            for (int s = 0; s < n; s++) iv[(size_t)i * n + s] = {tab[s], shoup(tab[s], q[i])};
        }
    }

    // a public key of random canonical residues (the flood is an identity in them) and a tensor whose ciphertext 0 is all zero and ciphertext 1 all q_i - 1
    const size_t ctw = count * 2 * (size_t)k * n;
    std::vector<u64> pk((size_t)2 * k * n), in(ctw), want(ctw), got(ctw), sm(n);
    srand(n * 31 + k * 7 + B);
    for (int p = 0; p < 2; p++) for (int i = 0; i < k; i++) for (int s = 0; s < n; s++) pk[((size_t)p * k + i) * n + s] = rnd() % q[i];
    for (size_t m = 0; m < count; m++) for (int p = 0; p < 2; p++) for (int i = 0; i < k; i++) for (int s = 0; s < n; s++)
        in[((m * 2 + p) * k + i) * n + s] = m == 0 ? 0 : m == 1 ? q[i] - 1 : rnd() % q[i];

    threadIdx = dim3(0, 0, 0); blockDim = dim3(1);
    int bad = 0;
    for (int form = 0; form < 2; form++) {
        want = in;
        if (crc_flood(A, pk.data(), want.data(), count, form, B, seed)) { puts("FAILED host twin"); return 2; }
        got = in;
        // the work space: the stated bytes less the 256 of alignment slack, cut as FloodLayout cuts it (each region a multiple of 256 bytes)
        const size_t wb = crc_flood_dev_work_bytes(A, count, form);
        const size_t uw = (count * (size_t)k * n * 8 + 255) / 256 * 32, ew = (count * 2 * (size_t)k * n * 8 + 255) / 256 * 32;
        if (wb != (uw + ew) * 8 + 256) { printf("FAILED work bytes %zu\n", wb); return 2; }
        std::vector<u64> U(count * (size_t)k * n), E(count * 2 * (size_t)k * n);                  // exactly the words the kernels may touch
        FloodArgs a = base;
        a.ct = got.data(); a.pk = pk.data(); a.U = U.data(); a.E = E.data(); a.W = form == CRC_NTT ? fw.data() : iv.data();
        const unsigned sgrid = (unsigned)(count * (size_t)(n / 2));                               // blockDim 1: a block per coefficient pair
        for (unsigned b = 0; b < sgrid + 3; b++) { blockIdx = dim3(b); flood_sample_body(a); }    // (+ 3: blocks past the tensor return at once)
        for (size_t r = 0; r < count * (size_t)k; r++) ntt_fwd_ref(U.data() + r * n, fw.data() + (r % k) * (size_t)n, n, q[r % k]);
        const unsigned jgrid = (unsigned)((count * (size_t)k + 7) / 8 * 8 * 2);                   // xcd_grid(count k, 2)
        for (unsigned b = 0; b < jgrid; b++) {
            blockIdx = dim3(b);
            if (form == CRC_NTT) { if (lazy) flood_join_body<false, true>(a, sm.data()); else flood_join_body<false, false>(a, sm.data()); }
            else { if (lazy) flood_join_body<true, true>(a, sm.data()); else flood_join_body<true, false>(a, sm.data()); }
        }
        if (memcmp(want.data(), got.data(), ctw * 8)) { printf("FAILED form=%d differs from the host twin\n", form); bad = 1; }
        if (!memcmp(in.data(), got.data(), ctw * 8)) { printf("FAILED form=%d: nothing was added\n", form); bad = 1; }
    }
    if (bad) return 1;
    printf("ok n=%d k=%d count=%zu B=%d lazy=%d\n", n, k, count, B, (int)lazy);
    crc_ctx_destroy(A);
    return 0;
}
