// CPU check of the modulus-switching kernels' own text (crcnn_amd/csrc/modswitch_device.h: the bodies of modswitch_coeff_kernel, modswitch_inverse_kernel and
// modswitch_rows_kernel, with ntt_device.h's passes and the device form of the 64-bit products) against the library's host twin crc_mod_switch, bit for bit, for
// all four form pairs: one thread per workgroup over each launch's whole grid, the constants and the tables rebuilt here from the moduli and "root_powers:i" /
// "inv_root_powers_div_two:i".  Built with -fsanitize=address,undefined (tests/test_mod_switch_cpu.py): every buffer has exactly the stated number of words, so an
// access past a row, the work space or the LDS image is an error the sanitizer reports.
//   mod_switch_kernel_check <n> <kept> <polys> <q_0> <q_1> ... <q_{k-1}>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CRC_FORCE_MAD_MUL 1
#include "modswitch_device.h"
#include "../../include/crcnn_hip.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
typedef unsigned __int128 u128;
static u64 mulm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); } return r; }
static u64 shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static u64 rnd() { return ((u64)rand() << 42) ^ ((u64)rand() << 21) ^ (u64)rand(); }

template <int D> static void run_coeff(const ModSwitchArgs &a)
{
    const unsigned grid = (unsigned)(a.polys * (size_t)(a.n / 2));           // blockDim 1: a block per coefficient pair
    for (unsigned b = 0; b < grid + 3; b++) { blockIdx = dim3(b); modswitch_coeff_body<D>(a); }        // (+ 3: blocks past the tensor return at once)
}
template <int D> static void run_rows(const ModSwitchArgs &a, bool lazy, u64 *sm)
{
    const unsigned grid = (unsigned)((a.polys + 7) / 8 * 8 * (size_t)a.c.kept);                       // xcd_grid(polys, kept)
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) modswitch_rows_body<D, true>(a, sm); else modswitch_rows_body<D, false>(a, sm); }
}
static void run_inverse(const ModSwitchArgs &a, bool lazy, u64 *sm)
{
    const unsigned grid = (unsigned)(a.polys * (size_t)a.rows);
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) modswitch_inverse_body<true>(a, sm); else modswitch_inverse_body<false>(a, sm); }
}
#define BY_D(D, f, ...) switch (D) { case 1: f<1>(__VA_ARGS__); break; case 2: f<2>(__VA_ARGS__); break; case 3: f<3>(__VA_ARGS__); break; case 4: f<4>(__VA_ARGS__); break; \
                                     case 5: f<5>(__VA_ARGS__); break; case 6: f<6>(__VA_ARGS__); break; case 7: f<7>(__VA_ARGS__); break; }

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int n = atoi(argv[1]), kept = atoi(argv[2]); const size_t polys = (size_t)atoi(argv[3]);
    const int k = argc - 4, D = k - kept;
    std::vector<u64> q(k);
    for (int i = 0; i < k; i++) q[i] = strtoull(argv[4 + i], 0, 0);
    int logn = 0; while ((1 << logn) < n) logn++;
    crc_ctx *A, *B;
    if (crc_ctx_create(n, q.data(), k, 65537, -1, &A) || crc_ctx_create(n, q.data(), kept, 65537, -1, &B) || !crc_mod_switch_supported(A, B)) { puts("FAILED context"); return 2; }

    ModSwitchConsts c; memset(&c, 0, sizeof c);
    c.k = k; c.kept = kept;
    bool lazy = true;
    for (int i = 0; i < k; i++) { c.q[i] = q[i]; c.one_s[i] = shoup(1, q[i]); lazy = lazy && (64 - __builtin_clzll(q[i])) <= 57; }
    for (int j = 0; j < D; j++) {
        const u64 p = q[k - 1 - j];
        c.h[j] = p >> 1;
        for (int i = 0; i < k - 1 - j; i++) {
            c.hmod[j][i] = c.h[j] % q[i];
            c.pinv[j][i] = powm(p % q[i], q[i] - 2, q[i]); c.pinv_s[j][i] = shoup(c.pinv[j][i], q[i]);
            u64 prod = 1; for (int l = 0; l < j; l++) prod = mulm(prod, q[k - 1 - l] % q[i], q[i]);
            c.pmod[j][i] = prod; c.pmod_s[j][i] = shoup(prod, q[i]);
        }
    }
    for (int i = 0; i < kept; i++) {
        u64 prod = 1; for (int j = 0; j < D; j++) prod = mulm(prod, q[k - 1 - j] % q[i], q[i]);
        c.Pinv[i] = powm(prod, q[i] - 2, q[i]); c.Pinv_s[i] = shoup(c.Pinv[i], q[i]);
    }
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

    // input: random canonical residues; polynomial 0 all zero, polynomial 1 every residue q_i - 1, polynomial 2 the edges of the last residue
    const size_t inw = polys * k * n, outw = polys * kept * n;
    std::vector<u64> in(inw), want(outw), got(outw), sm(n);
    srand(n * 31 + k * 7 + kept);
    for (size_t p = 0; p < polys; p++) for (int i = 0; i < k; i++) for (int s = 0; s < n; s++) in[(p * k + i) * n + s] = rnd() % q[i];
    for (int i = 0; i < k && polys > 1; i++) for (int s = 0; s < n; s++) { in[(size_t)i * n + s] = 0; in[((size_t)k + i) * n + s] = q[i] - 1; }
    if (polys > 2) {
        const u64 p = q[k - 1], h = p >> 1, edge[5] = {0, h, h + 1, p - 1 - h, p - 1};
        for (int s = 0; s < n; s++) in[((size_t)2 * k + k - 1) * n + s] = edge[s % 5];
    }

    ModSwitchArgs base{};
    base.c = c; base.polys = polys; base.n = n; base.logn = logn;
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1);
    const size_t ps = (size_t)k * n;
    int bad = 0;
    if (polys % 2) { puts("FAILED: polys must be even (the host twin takes ciphertexts of size 2)"); return 2; }
    for (int in_form = 0; in_form < 2; in_form++) for (int out_form = 0; out_form < 2; out_form++) {
        if (crc_mod_switch(A, B, in.data(), in_form, polys / 2, 2, want.data(), out_form)) { puts("FAILED host twin"); return 2; }
        std::fill(got.begin(), got.end(), ~0ull);
        const int row0 = out_form == CRC_NTT ? kept : 0, nrows = in_form == CRC_NTT ? k - row0 : 0;
        std::vector<u64> work(polys * (size_t)nrows * n);                  // exactly what crc_mod_switch_work_bytes counts (less its alignment slack)
        if (in_form == CRC_NTT) {
            ModSwitchArgs v = base;
            v.kept_in = in.data(); v.kept_ps = ps; v.out = work.data(); v.row0 = row0; v.rows = nrows; v.W = iv.data();
            run_inverse(v, lazy, sm.data());
        }
        ModSwitchArgs a = base;
        a.out = got.data(); a.W = fw.data();
        if (in_form == CRC_COEFF) { a.kept_in = in.data(); a.kept_ps = ps; a.drop_in = in.data() + (size_t)kept * n; a.drop_ps = ps; a.kept_ntt = 0; }
        else if (out_form == CRC_NTT) { a.kept_in = in.data(); a.kept_ps = ps; a.drop_in = work.data(); a.drop_ps = (size_t)D * n; a.kept_ntt = 1; }
        else { a.kept_in = work.data(); a.kept_ps = ps; a.drop_in = work.data() + (size_t)kept * n; a.drop_ps = ps; a.kept_ntt = 0; }
        if (out_form == CRC_NTT) { BY_D(D, run_rows, a, lazy, sm.data()) } else { BY_D(D, run_coeff, a) }
        if (memcmp(want.data(), got.data(), outw * 8)) { printf("FAILED in_form=%d out_form=%d differs from the host twin\n", in_form, out_form); bad = 1; }
    }
    if (bad) return 1;
    printf("ok n=%d k=%d kept=%d polys=%zu lazy=%d\n", n, k, kept, polys, (int)lazy);
    crc_ctx_destroy(A); crc_ctx_destroy(B);
    return 0;
}
