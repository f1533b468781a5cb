// CPU check of the slot kernels' own text (crcnn_amd/csrc/slots_device.h: the bodies of slots_compose_kernel / slots_decompose_kernel, with ntt_device.h's passes
// and the device form of the 64-bit products) against the library's host twins, bit for bit: one thread per workgroup over the launch's whole grid, the tables of
// t rebuilt here from "slots_root".  Built with -fsanitize=address,undefined (tests/test_slots_cpu.py): the buffers have exactly the size a caller must provide,
// so an access past a row, past the values the strides reach or past the LDS image is an error the sanitizer reports.
//   slots_kernel_check <n> <t> <slots> <layout 0 item-major | 1 image-major>
#include <hip/hip_runtime.h>
#include <climits>
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

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int n = atoi(argv[1]); const u64 t = strtoull(argv[2], 0, 0); const int S = atoi(argv[3]); const int layout = atoi(argv[4]);
    int logn = 0; while ((1 << logn) < n) logn++;
    u64 q[1] = {0x3fffffff000001ULL};
    crc_ctx *c;
    if (crc_ctx_create(n, q, 1, t, -1, &c) || !crc_slots_supported(c)) { puts("FAILED context"); return 2; }
    u64 root; crc_ctx_table(c, "slots_root", &root, 1);
    std::vector<u64> idx64(n); crc_ctx_table(c, "slots_index_map", idx64.data(), n);
    std::vector<u32> idx(idx64.begin(), idx64.end());
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
    const size_t is = layout ? 1 : S, ss = layout ? count : 1;
    std::vector<long long> v(count * S), back(count * S, -7), hback(count * S, -7);
    srand(n + S);
    for (auto &x : v) x = ((long long)rand() << 33) ^ ((long long)rand() << 11) ^ rand();
    if (S >= 5) { v[0] = LLONG_MIN; v[1] = LLONG_MAX; v[2] = -1; v[3] = (long long)t; v[4] = -(long long)t - 3; }
    std::vector<u64> want(count * n), got(count * n, ~0ull), sm(n);
    if (crc_slots_compose(c, (const int64_t *)v.data(), count, S, is, ss, want.data())) { puts("FAILED host compose"); return 2; }
    SlotArgs a{};
    a.count = count; a.slots = S; a.item_stride = is; a.slot_stride = ss; a.n = n; a.logn = logn; a.t = t; a.one_s = (u64)(((u128)1 << 64) / t);
    a.idx = idx.data();
    const bool lazy = (64 - __builtin_clzll(t)) <= 57;
    const unsigned grid = (unsigned)(((count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP + 7) / 8 * 8 * CRC_SLOT_GROUP);        // xcd_grid(groups, CRC_SLOT_GROUP)
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1); gridDim = dim3(grid);
    a.vals_in = v.data(); a.plain_out = got.data(); a.W = iv.data();
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) slots_compose_body<true>(a, sm.data()); else slots_compose_body<false>(a, sm.data()); }
    if (memcmp(want.data(), got.data(), want.size() * 8)) { puts("FAILED compose differs from the host twin"); return 1; }
    std::vector<u64> pl(count * n);                            // decompose takes any words
    for (auto &x : pl) x = ((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand();
    if (crc_slots_decompose(c, pl.data(), count, S, (int64_t *)hback.data(), is, ss)) { puts("FAILED host decompose"); return 2; }
    a.plain_in = pl.data(); a.vals_out = back.data(); a.W = fw.data();
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); if (lazy) slots_decompose_body<true>(a, sm.data()); else slots_decompose_body<false>(a, sm.data()); }
    if (hback != back) { puts("FAILED decompose differs from the host twin"); return 1; }
    printf("ok n=%d t=%llu slots=%d layout=%d lazy=%d\n", n, (unsigned long long)t, S, layout, (int)lazy);
    crc_ctx_destroy(c);
    return 0;
}
