// CPU check of the client-side activation kernel's own text (crcnn_amd/csrc/slots_device.h: the body of slots_act_kernel, with ntt_device.h's passes and the
// device form of the 64-bit products) against the library's host twin crc_slots_act, bit for bit: one thread per workgroup over the launch's whole grid, the
// tables of t rebuilt here from "slots_root".  Built with -fsanitize=address,undefined (tests/test_slots_act_cpu.py): the input has exactly planes * xd * yd * n
// words and the output exactly planes * xo * yo * n, so an access past a window row, past the output or past the LDS image is an error the sanitizer reports.
// One thread owns all n / 2 pairs of the image, so the window body is instantiated with PAIRS = n / 2 of the largest ring (the device passes 8); a 1 x 1 window
// of stride 1 runs the one-row body (PAIRS = 0) as on the device.  Every combination of
// relu and a cap for the window given; a 1 x 1 window of stride 1 also runs in place.
//   slots_act_kernel_check <n> <t> <divisor> <xd> <yd> <xs> <ys> <xf> <yf> <cap>
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
static u64 rnd64() { return ((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand(); }

static void run_grid(const SlotActArgs &a, bool lazy, u64 *sm)
{
    const unsigned grid = (unsigned)(((a.count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP + 7) / 8 * 8 * CRC_SLOT_GROUP);          // xcd_grid(groups, CRC_SLOT_GROUP)
    threadIdx = dim3(0, 0, 0); blockDim = dim3(1); gridDim = dim3(grid);
    const bool single = a.xf == 1 && a.yf == 1 && a.xs == 1 && a.ys == 1;          // k_slots_act's rule: the kernel of a one-row window keeps no maxima
    for (unsigned b = 0; b < grid; b++) {
        blockIdx = dim3(b);
        if (single) { if (lazy) slots_act_body<true, 0>(a, sm); else slots_act_body<false, 0>(a, sm); }
        else if (lazy) slots_act_body<true, 8192>(a, sm); else slots_act_body<false, 8192>(a, sm);
    }
}

int main(int argc, char **argv)
{
    if (argc < 11) return 2;
    const int n = atoi(argv[1]); const u64 t = strtoull(argv[2], 0, 0), D = strtoull(argv[3], 0, 0);
    const int xd = atoi(argv[4]), yd = atoi(argv[5]), xs = atoi(argv[6]), ys = atoi(argv[7]), xf = atoi(argv[8]), yf = atoi(argv[9]);
    const u64 cap_arg = strtoull(argv[10], 0, 0);
    if (n > 16384) return 2;
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
    const size_t planes = 2;
    const int xo = (xd - xf) / xs + 1, yo = (yd - yf) / ys + 1;
    const size_t in_rows = planes * xd * yd, out_rows = planes * (size_t)xo * yo;
    // rows: composed from chosen slot values -- random ones, the extremes, 0, every tie that fits, one window all negative, one all zero -- and random words >= t
    std::vector<u64> in(in_rows * n), want(out_rows * n), got(out_rows * n), sm(n);
    srand(n + (unsigned)D + xf * 7 + yf);
    const long long half = (long long)((t - 1) >> 1);
    {
        std::vector<long long> v(in_rows * (size_t)n);
        for (auto &x : v) x = (long long)(rnd64() % t) - half;
        std::vector<long long> edge = {half, -half, 0, 1, -1};
        for (int m = 1; m <= 3; m += 2) if (D % 2 == 0 && (u128)(D / 2) * m <= (u128)half) { edge.push_back((long long)(D / 2 * m)); edge.push_back(-(long long)(D / 2 * m)); }
        if (cap_arg && (u128)cap_arg * D + D <= (u128)half) for (int d = -1; d <= 1; d++) edge.push_back((long long)((cap_arg + d) * D));
        for (size_t r = 0; r < in_rows; r++) for (size_t i = 0; i < edge.size() && i < (size_t)n; i++) if ((r + i) % 3 == 0) v[r * n + (i * 7 + r) % n] = edge[i];
        for (size_t r = 0; r < in_rows; r++) { v[r * n + 1 % n] = -(long long)(rnd64() % (u64)half) - 1; v[r * n + 2 % n] = 0; }        // a negative and a zero window
        if (crc_slots_compose(c, (const int64_t *)v.data(), in_rows, n, n, 1, in.data())) { puts("FAILED host compose"); return 2; }
        for (size_t i = 0; i < in.size(); i++) if (i % 3 == 0 && t < ((u64)1 << 63)) in[i] += t;                                   // words >= t
        for (int i = 0; i < n; i++) in[(in_rows - 1) * n + i] = rnd64() * 2 + (rnd64() & 1);                                        // any 64-bit words
    }
    SlotActArgs a{};
    a.count = out_rows; a.n = n; a.logn = logn; a.t = t; a.one_s = (u64)(((u128)1 << 64) / t);
    a.Wf = fw.data(); a.Wi = iv.data();
    a.D = D; a.recip = D == 1 ? ~(u64)0 : (u64)(((u128)1 << 64) / D);
    a.xd = xd; a.yd = yd; a.xs = xs; a.ys = ys; a.xf = xf; a.yf = yf; a.xo = xo; a.yo = yo;
    const bool lazy = (64 - __builtin_clzll(t)) <= 57;
    for (int relu = 0; relu <= 1; relu++) for (const u64 cap : {(u64)0, cap_arg}) {
        if (crc_slots_act(c, in.data(), planes, xd, yd, xs, ys, xf, yf, D, relu, cap, want.data())) { puts("FAILED host act"); return 2; }
        a.relu = relu; a.cap = cap;
        std::fill(got.begin(), got.end(), ~0ull);
        a.plain_in = in.data(); a.plain_out = got.data();
        run_grid(a, lazy, sm.data());
        if (memcmp(want.data(), got.data(), want.size() * 8)) { printf("FAILED relu=%d cap=%llu differs from the host twin\n", relu, (unsigned long long)cap); return 1; }
        if (xf == 1 && yf == 1 && xs == 1 && ys == 1) {
            std::vector<u64> inplace(in);
            a.plain_in = inplace.data(); a.plain_out = inplace.data();
            run_grid(a, lazy, sm.data());
            if (memcmp(want.data(), inplace.data(), want.size() * 8)) { puts("FAILED in place differs from the host twin"); return 1; }
            if (!relu && !cap) {                                  // the rescale itself
                std::vector<u64> rs(in.size());
                if (crc_slots_rescale(c, in.data(), in_rows, D, rs.data()) || memcmp(rs.data(), want.data(), rs.size() * 8)) { puts("FAILED differs from crc_slots_rescale"); return 1; }
            }
        }
    }
    printf("ok n=%d t=%llu D=%llu lazy=%d fused=%d rows=%zu->%zu\n", n, (unsigned long long)t, (unsigned long long)D, (int)lazy, (int)ntt_fused_stage(logn), in_rows, out_rows);
    crc_ctx_destroy(c);
    return 0;
}
