// CPU check of the rescale kernel's own text (crcnn_amd/csrc/slots_device.h: the body of slots_rescale_kernel, with ntt_device.h's passes and the device form of
// the 64-bit products) against the library's host twin crc_slots_rescale, bit for bit: one thread per workgroup over the launch's whole grid, the tables of t
// rebuilt here from "slots_root".  Built with -fsanitize=address,undefined (tests/test_slots_rescale_cpu.py): the buffers have exactly count * n words, so an
// access past a row or past the LDS image is an error the sanitizer reports.  Out of place and in place.  Before that, the reciprocal quotient of the pointwise
// step against unsigned __int128 division over edge magnitudes.
//   slots_rescale_kernel_check <n> <t> <divisor>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CRC_FORCE_MAD_MUL 1
#include "slots_device.h"
#include "../../include/crcnn_hip.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
typedef unsigned __int128 u128;
static u64 mulm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); } return r; }
static u32 brev(u32 x, int b) { u32 r = 0; for (int i = 0; i < b; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
static u64 recip_of(u64 D) { return D == 1 ? ~(u64)0 : (u64)(((u128)1 << 64) / D); }

// slot_quotient == floor(x / D) for every x the centring can produce (x = |v| + rounding < 2^63) and beyond, at the edges of each divisor
static int quotient_check()
{
    std::vector<u64> Ds = {1, 2, 3, 5, 6, 7, 255, 256, 257, 1023, 1024, 65537, 0xffffffffULL, 0x100000000ULL, 0x100000001ULL, (u64)1 << 39, ((u64)1 << 39) + 1,
                           ((u64)1 << 61) - 1, (u64)1 << 61, ((u64)1 << 62) - 1, (u64)1 << 62};
    srand(12345);
    for (int i = 0; i < 200; i++) Ds.push_back(((((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand()) >> (rand() % 62)) % ((u64)1 << 62) + 1);
    for (const u64 D : Ds) {
        const u64 R = recip_of(D);
        std::vector<u64> xs = {0, 1, 2, D - 1, D, D + 1, D / 2, D / 2 + 1, 3 * (D / 2), ((u64)1 << 63) - 1, (u64)1 << 63, ~(u64)0, ~(u64)0 - 1, ((u64)1 << 62) + (D >> 1)};
        for (u64 m = 1; m < 40; m++) {                        // multiples of D and their neighbours, small and close to 2^63 / 2^64
            const u128 a = (u128)D * m, b = (u128)D * ((((u128)1 << 63) / D) - m + 1), c2 = (u128)D * ((((u128)1 << 64) - 1) / D - m + 1);
            for (const u128 y : {a, b, c2}) for (int d = -1; d <= 1; d++) { const u128 z = y + d; if (z >> 64) continue; xs.push_back((u64)z); }
        }
        for (int i = 0; i < 2000; i++) xs.push_back((((u64)rand() << 42) ^ ((u64)rand() << 21) ^ (u64)rand()) >> (rand() % 64));
        for (const u64 x : xs)
            if (slot_quotient(x, D, R) != (u64)((u128)x / D)) { printf("FAILED quotient x=%llu D=%llu\n", (unsigned long long)x, (unsigned long long)D); return 1; }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int n = atoi(argv[1]); const u64 t = strtoull(argv[2], 0, 0), D = strtoull(argv[3], 0, 0);
    if (quotient_check()) return 1;
    int logn = 0; while ((1 << logn) < n) logn++;
    u64 q[1] = {0x3fffffff000001ULL};
    crc_ctx *c;
    if (crc_ctx_create(n, q, 1, t, -1, &c) || !crc_slots_supported(c)) { puts("FAILED context"); return 2; }
    u64 root; crc_ctx_table(c, "slots_root", &root, 1);
    std::vector<ulonglong2> fw(n), iv(n);
    const u64 iroot = powm(root, t - 2, t);
    u64 p = 1, ip = 1;
    for (int i = 0; i < n; i++) {
        const u32 j = brev(i, logn);
        const u64 h = (ip & 1) ? (u64)(((u128)ip + t) >> 1) : ip >> 1;
        fw[j] = {p, (u64)(((u128)p << 64) / t)}; iv[j] = {h, (u64)(((u128)h << 64) / t)};
        p = mulm(p, root, t); ip = mulm(ip, iroot, t);
    }
    const size_t count = 19;                                   // two XCD groups, the second one partly filled
    // rows: random words (any 64-bit value: the fill reduces mod t), and rows composed from chosen slot values -- the extremes, 0, every tie that fits
    std::vector<u64> in(count * n), want(count * n), got(count * n, ~0ull), sm(n);
    srand(n + (unsigned)D);
    for (auto &x : in) x = ((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand();
    {
        const long long half = (long long)((t - 1) >> 1);
        std::vector<long long> v(n);
        for (auto &x : v) x = (long long)((((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand()) % t) - half;
        std::vector<long long> edge = {half, -half, 0, 1, -1};
        for (int m = 1; m <= 5; m += 2) if (D % 2 == 0 && (u128)(D / 2) * m <= (u128)half) { edge.push_back((long long)(D / 2 * m)); edge.push_back(-(long long)(D / 2 * m)); }
        for (int m = 1; m <= 3; m++) if ((u128)D * m <= (u128)half) { edge.push_back((long long)(D * m)); edge.push_back(-(long long)(D * m)); edge.push_back((long long)(D * m) - 1); }
        for (size_t i = 0; i < edge.size() && i < (size_t)n; i++) v[(i * 7) % n] = edge[i];
        if (crc_slots_compose(c, (const int64_t *)v.data(), 1, n, n, 1, in.data() + 2 * (size_t)n)) { puts("FAILED host compose"); return 2; }
        for (int i = 0; i < n; i++) in[17 * (size_t)n + i] = in[2 * (size_t)n + i] + (i % 3 ? 0 : t);      // the same row with words >= t
    }
    if (crc_slots_rescale(c, in.data(), count, D, want.data())) { puts("FAILED host rescale"); return 2; }
    SlotRescaleArgs a{};
    a.count = count; a.n = n; a.logn = logn; a.t = t; a.one_s = (u64)(((u128)1 << 64) / t);
    a.Wf = fw.data(); a.Wi = iv.data();
    a.D = D; a.recip = recip_of(D); a.hpos = D >> 1; a.hneg = (D - 1) >> 1;
    const bool lazy = (64 - __builtin_clzll(t)) <= 57;
    const unsigned grid = (unsigned)(((count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP + 7) / 8 * 8 * CRC_SLOT_GROUP);        // xcd_grid(groups, CRC_SLOT_GROUP)
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1); gridDim = dim3(grid);
    a.plain_in = in.data(); a.plain_out = got.data();
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) slots_rescale_body<true>(a, sm.data()); else slots_rescale_body<false>(a, sm.data()); }
    if (memcmp(want.data(), got.data(), want.size() * 8)) { puts("FAILED out of place differs from the host twin"); return 1; }
    std::vector<u64> inplace(in);
    a.plain_in = inplace.data(); a.plain_out = inplace.data();
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) slots_rescale_body<true>(a, sm.data()); else slots_rescale_body<false>(a, sm.data()); }
    if (memcmp(want.data(), inplace.data(), want.size() * 8)) { puts("FAILED in place differs from the host twin"); return 1; }
    printf("ok n=%d t=%llu D=%llu lazy=%d fused=%d\n", n, (unsigned long long)t, (unsigned long long)D, (int)lazy, (int)ntt_fused_stage(logn));
    crc_ctx_destroy(c);
    return 0;
}
