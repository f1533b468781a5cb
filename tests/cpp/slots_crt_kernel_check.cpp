// CPU check of the two kernels over several plain moduli (crcnn_amd/csrc/slots_device.h: the bodies of slots_crt_decompose_kernel and slots_crt_act_kernel, with
// ntt_device.h's passes and the device form of the 64-bit products) against the library's host twins crc_slots_crt_decompose and crc_slots_crt_act, bit for bit:
// one thread per workgroup over the launch's whole grid, every modulus' tables rebuilt here from "slots_root", the Garner constants rebuilt here too.  Built with
// -fsanitize=address,undefined (tests/test_slots_crt_cpu.py): every row tensor has exactly count * n words and the value buffer exactly what the strides reach, so
// an access past a row, past the values or past the LDS image is an error the sanitizer reports.  One thread owns all n / 2 pairs of the image, so the bodies are
// instantiated with PAIRS = n / 2 of the largest ring checked (the device passes 4 or 8).  Decompose runs item-major and image-major with slots < n; the
// activation runs for both relu values, without and with the cap given, out of place and in place.
//   slots_crt_kernel_check <n> <divisor> <cap> <t_0> [<t_1> ...]
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
static const int MAXP = 128;                                 // n <= 256
static u64 mulm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); } return r; }
static u32 brev(u32 x, int b) { u32 r = 0; for (int i = 0; i < b; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
static u64 rnd64() { return ((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand(); }

template <class Body>
static void run_grid(const SlotCrtArgs &a, Body body)
{
    const unsigned grid = (unsigned)(((a.count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP + 7) / 8 * 8 * CRC_SLOT_GROUP);          // xcd_grid(groups, CRC_SLOT_GROUP)
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1); gridDim = dim3(grid);
    for (unsigned b = 0; b < grid; b++) { blockIdx = dim3(b); body(a); }
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int n = atoi(argv[1]); const u64 D = strtoull(argv[2], 0, 0), cap_arg = strtoull(argv[3], 0, 0);
    const int r = argc - 4;
    if (n > 2 * MAXP || r > CRC_SLOTS_CRT_MAX) return 2;
    int logn = 0; while ((1 << logn) < n) logn++;
    u64 q[1] = {0x3fffffff000001ULL};
    crc_ctx *ctxs[CRC_SLOTS_CRT_MAX];
    std::vector<ulonglong2> fw[CRC_SLOTS_CRT_MAX], iv[CRC_SLOTS_CRT_MAX];
    std::vector<u64> map64(n); std::vector<u32> idx(n);
    SlotCrtArgs a{};
    a.r = r; a.n = n; a.logn = logn;
    bool lazy = true;
    u128 T = 1;
    for (int j = 0; j < r; j++) {
        const u64 t = strtoull(argv[4 + j], 0, 0);
        if (crc_ctx_create(n, q, 1, t, -1, &ctxs[j])) { puts("FAILED context"); return 2; }
        u64 root; crc_ctx_table(ctxs[j], "slots_root", &root, 1);
        fw[j].resize(n); iv[j].resize(n);
        const u64 iroot = powm(root, t - 2, t);
        u64 p = 1, ip = 1;
        for (int i = 0; i < n; i++) {
            const u32 k = brev(i, logn);
            const u64 h = (ip & 1) ? (u64)(((u128)ip + t) >> 1) : ip >> 1;
            fw[j][k] = {p, (u64)(((u128)p << 64) / t)}; iv[j][k] = {h, (u64)(((u128)h << 64) / t)};
            p = mulm(p, root, t); ip = mulm(ip, iroot, t);
        }
        SlotCrtMod &m = a.m[j];
        m.Wf = fw[j].data(); m.Wi = iv[j].data(); m.t = t; m.one_s = (u64)(((u128)1 << 64) / t);
        m.P = (u64)T; m.Pinv = j ? powm((u64)(T % t), t - 2, t) : 1; m.Pinv_s = (u64)(((u128)m.Pinv << 64) / t);
        T *= t;
        lazy = lazy && (64 - __builtin_clzll(t)) <= 57;
    }
    if (!crc_slots_crt_supported(ctxs, r) || (T >> 63)) { puts("FAILED base"); return 2; }
    a.T = (u64)T; a.half = (a.T - 1) >> 1;
    crc_ctx_table(ctxs[0], "slots_index_map", map64.data(), n);
    for (int i = 0; i < n; i++) idx[i] = (u32)map64[i];
    a.idx = idx.data();
    const size_t count = 19;                                  // more than one XCD group of 16
    a.count = count;
    // rows: composed from chosen integers mod T -- random ones, the extremes, 0, every tie that fits, the values around the cap -- words >= t_j, and any 64-bit words
    std::vector<u64> in[CRC_SLOTS_CRT_MAX];
    srand(n + (unsigned)D + r);
    const long long half = (long long)a.half;
    {
        std::vector<long long> v(count * (size_t)n);
        for (auto &x : v) x = (long long)(rnd64() % a.T) - half;
        std::vector<long long> edge = {half, -half, 0, 1, -1};
        for (int m = 1; m <= 3; m += 2) if (D % 2 == 0 && (u128)(D / 2) * m <= (u128)half) { edge.push_back((long long)(D / 2 * m)); edge.push_back(-(long long)(D / 2 * m)); }
        if ((u128)D <= (u128)half) for (long long e : {(long long)D, -(long long)D, (long long)D - 1, 1 - (long long)D}) edge.push_back(e);
        if (cap_arg && (u128)cap_arg * D + D <= (u128)half) for (int d = -1; d <= 1; d++) edge.push_back((long long)((cap_arg + d) * D));
        for (size_t row = 0; row < count; row++) for (size_t i = 0; i < edge.size() && i < (size_t)n; i++) if ((row + i) % 3 == 0) v[row * n + (i * 7 + row) % n] = edge[i];
        for (int j = 0; j < r; j++) {
            in[j].resize(count * (size_t)n);
            if (crc_slots_compose(ctxs[j], (const int64_t *)v.data(), count, n, n, 1, in[j].data())) { puts("FAILED host compose"); return 2; }
            for (size_t i = j; i < in[j].size(); i += 3) if (a.m[j].t < ((u64)1 << 63)) in[j][i] += a.m[j].t;                      // words >= t_j
            for (int i = 0; i < n; i++) in[j][(count - 1) * n + i] = rnd64() * 2 + (rnd64() & 1);                                   // any 64-bit words
        }
    }
    std::vector<u64> sm(n);
    const u64 *hin[CRC_SLOTS_CRT_MAX];
    for (int j = 0; j < r; j++) { hin[j] = in[j].data(); a.m[j].plain_in = in[j].data(); }
    // ---- decompose: item-major (all n slots) and image-major (slots < n)
    const int part = n - 5;
    for (int layout = 0; layout < 2; layout++) {
        const int slots = layout ? part : n;
        const size_t is = layout ? 1 : (size_t)n, ss = layout ? count : 1;
        const size_t words = (count - 1) * is + (size_t)(slots - 1) * ss + 1;
        std::vector<long long> want(words, -7), got(words, -7);
        if (crc_slots_crt_decompose(ctxs, r, hin, count, slots, (int64_t *)want.data(), is, ss)) { puts("FAILED host decompose"); return 2; }
        a.vals_out = got.data(); a.slots = slots; a.item_stride = is; a.slot_stride = ss;
        if (lazy) run_grid(a, [&](const SlotCrtArgs &x) { slots_crt_decompose_body<true, MAXP>(x, sm.data()); });
        else run_grid(a, [&](const SlotCrtArgs &x) { slots_crt_decompose_body<false, MAXP>(x, sm.data()); });
        if (memcmp(want.data(), got.data(), words * 8)) { printf("FAILED decompose layout=%d differs from the host twin\n", layout); return 1; }
    }
    // ---- the activation
    a.D = D; a.recip = D == 1 ? ~(u64)0 : (u64)(((u128)1 << 64) / D);
    std::vector<u64> want[CRC_SLOTS_CRT_MAX], got[CRC_SLOTS_CRT_MAX];
    u64 *hwant[CRC_SLOTS_CRT_MAX];
    for (int j = 0; j < r; j++) { want[j].resize(count * (size_t)n); got[j].resize(count * (size_t)n); hwant[j] = want[j].data(); }
    for (int relu = 0; relu <= 1; relu++) for (const u64 cap : {(u64)0, cap_arg}) {
        if (crc_slots_crt_act(ctxs, r, hin, count, D, relu, cap, hwant)) { puts("FAILED host act"); return 2; }
        a.relu = relu; a.cap = cap;
        for (int pass = 0; pass < 2; pass++) {              // out of place, then in place
            for (int j = 0; j < r; j++) {
                if (pass) got[j] = in[j]; else std::fill(got[j].begin(), got[j].end(), ~0ull);
                a.m[j].plain_in = pass ? got[j].data() : in[j].data(); a.m[j].plain_out = got[j].data();
            }
            if (lazy) run_grid(a, [&](const SlotCrtArgs &x) { slots_crt_act_body<true, MAXP>(x, sm.data()); });
            else run_grid(a, [&](const SlotCrtArgs &x) { slots_crt_act_body<false, MAXP>(x, sm.data()); });
            for (int j = 0; j < r; j++) if (memcmp(want[j].data(), got[j].data(), want[j].size() * 8)) {
                printf("FAILED act relu=%d cap=%llu modulus %d %s differs from the host twin\n", relu, (unsigned long long)cap, j, pass ? "in place" : "out of place"); return 1;
            }
        }
    }
    printf("ok n=%d r=%d T=%llu D=%llu lazy=%d fused=%d rows=%zu\n", n, r, (unsigned long long)a.T, (unsigned long long)D, (int)lazy, (int)ntt_fused_stage(logn), count);
    for (int j = 0; j < r; j++) crc_ctx_destroy(ctxs[j]);
    return 0;
}
