// CPU check of the 64-bit row transform's own text (crcnn_amd/csrc/ntt_device.h: reduce_small, shoup_lazy4, the lazy and strict butterflies, ntt_row_passes,
// the gap-1 pair stages, inv_stages_unscaled) against unsigned __int128 arithmetic and a textbook Cooley-Tukey / Gentleman-Sande transform in SEAL's order.  One
// thread per workgroup (hipstub: threadIdx 0, blockDim 1); the tables are built here from a 2n-th root found by search -- the project library is not linked.
// Built with -fsanitize=address,undefined (tests/test_ntt_rows_cpu.py): the LDS image has exactly n words.
//   ntt_rows_check                 every part over the modulus classes the dispatcher admits to each path
//   ntt_rows_check lazy <prime>    the lazy parts (reduce_small, shoup_lazy4, rows) over ONE prime, whatever its width: the sensitivity check of the test
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CRC_FORCE_MAD_MUL 1
#include "ntt_device.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
typedef unsigned __int128 u128;
typedef unsigned long long ull;

static u64 rng_state = 0x9e3779b97f4a7c15ULL;
static u64 rnd() { u64 z = (rng_state += 0x9e3779b97f4a7c15ULL); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
static u64 mulm(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); } return r; }
static u32 brev(u32 x, int b) { u32 r = 0; for (int i = 0; i < b; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
static int bits_of(u64 q) { return 64 - __builtin_clzll(q); }
static u64 shoup_of(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static float rq_of(u64 q) { return 1.0f / (float)((u32)(q >> 32) + 1); }

// a primitive 2n-th root of unity mod q (q = 1 mod 2n): g^((q-1)/2n) for the first g whose power has order exactly 2n
static u64 find_root(u64 q, int n)
{
    if ((q - 1) % (2 * (u64)n)) return 0;
    for (u64 g = 2; g < 1000; g++) { const u64 r = powm(g, (q - 1) / (2 * (u64)n), q); if (powm(r, n, q) == q - 1) return r; }
    return 0;
}

struct Tables { std::vector<ulonglong2> fw, iv, ivu; u64 psi, inv_n; };      // root powers, inverse powers halved, inverse powers as they are (bit-reversed index)
static Tables make_tables(u64 q, int n, int logn, u64 psi)
{
    Tables T; T.fw.resize(n); T.iv.resize(n); T.ivu.resize(n); T.psi = psi; T.inv_n = powm((u64)n, q - 2, q);
    const u64 ipsi = powm(psi, q - 2, q);
    u64 p = 1, ip = 1;
    for (int i = 0; i < n; i++) {
        const u32 j = brev(i, logn);
        const u64 h = (ip & 1) ? (u64)(((u128)ip + q) >> 1) : ip >> 1;
        T.fw[j] = {p, shoup_of(p, q)}; T.iv[j] = {h, shoup_of(h, q)}; T.ivu[j] = {ip, shoup_of(ip, q)};
        p = mulm(p, psi, q); ip = mulm(ip, ipsi, q);
    }
    return T;
}

// the textbook transforms: SEAL's loop order, canonical values, the tables' w only
static void ref_fwd(std::vector<u64> &x, const Tables &T, int n, u64 q)
{
    int t = n;
    for (int m = 1; m < n; m <<= 1) {
        t >>= 1;
        for (int i = 0; i < m; i++) {
            const u64 w = T.fw[m + i].x;
            for (int j = 2 * i * t; j < 2 * i * t + t; j++) { const u64 U = x[j], V = mulm(x[j + t], w, q); x[j] = (U + V) % q; x[j + t] = (U + q - V) % q; }
        }
    }
}
static void ref_inv(std::vector<u64> &x, const Tables &T, int n, u64 q)
{
    int t = 1;
    for (int m = n; m > 1; m >>= 1) {
        const int h = m >> 1;
        for (int i = 0; i < h; i++) {
            const u64 w = T.ivu[h + i].x;
            for (int j = 2 * i * t; j < 2 * i * t + t; j++) { const u64 U = x[j], V = x[j + t]; x[j] = (U + V) % q; x[j + t] = mulm((U + q - V) % q, w, q); }
        }
        t <<= 1;
    }
    for (auto &v : x) v = mulm(v, T.inv_n, q);
}

static int reduce_small_check(u64 q)
{
    const u64 q2 = q + q; const float rq = rq_of(q);
    const u128 lim = (u128)128 * q < ((u128)1 << 64) ? (u128)128 * q : ((u128)1 << 64);
    auto one = [&](u64 v) { const u64 r = reduce_small(v, q, q2, rq); if (r != v % q) { printf("FAILED reduce_small q=%llx v=%llx got %llx want %llx\n", (ull)q, (ull)v, (ull)r, (ull)(v % q)); return 1; } return 0; };
    for (int m = 0; m <= 128; m++)
        for (int d = -2; d <= 2; d++) {
            const __int128 v = (__int128)m * q + d;
            if (v >= 0 && (u128)v < lim && one((u64)v)) return 1;
        }
    if (one((u64)(lim - 1))) return 1;
    for (int i = 0; i < 2000000; i++) { const u64 v = (u64)(((u128)rnd() * lim) >> 64); if (one(v)) return 1; }
    return 0;
}

static int shoup_lazy4_check(u64 q, int &maxk)
{
    std::vector<u64> as = {0, 1, 2, q - 1, q, q + 1, 2 * q - 1, 2 * q, 4 * q - 1, 4 * q, 16 * q - 1, (u64)1 << 32, ((u64)1 << 32) - 1, ((u64)1 << 63), ~(u64)0, ~(u64)0 - 1,
                           ~(u64)0 - 2, ~(u64)0 - 3};
    std::vector<u64> ws = {0, 1, 2, q - 1, q - 2, q / 2, q / 2 + 1, ((u64)1 << 32) % q, (((u64)1 << 32) - 1) % q};
    auto one = [&](u64 a, u64 w) {
        const u64 r = shoup_lazy4(a, w, shoup_of(w, q), q);
        if (r % q != (u64)((u128)a * w % q) || (u128)r >= (u128)4 * q) { printf("FAILED shoup_lazy4 q=%llx a=%llx w=%llx got %llx\n", (ull)q, (ull)a, (ull)w, (ull)r); return 1; }
        if ((int)(r / q) > maxk) maxk = (int)(r / q);
        return 0;
    };
    for (const u64 a : as) for (const u64 w : ws) if (one(a, w)) return 1;
    for (int i = 0; i < 2000000; i++) {
        u64 a = rnd(); const u64 w = rnd() % q;
        if ((i & 3) == 1) a |= ~(u64)0 << 40;                 // the top of the word, where the three-product estimate is furthest short
        if (one(a, w)) return 1;
    }
    return 0;
}

// one row through ntt_row_passes on the image, the way ntt_rows_body fills and drains it (FUSE1) or element by element (no fused stage), final reduction included
template <bool INV, bool LAZY, bool FUSE1>
static void run_row(const std::vector<u64> &in, std::vector<u64> &out, std::vector<u64> &sm, const Tables &T, int n, int logn, u64 q)
{
    const u64 q2 = q + q; const float rq = rq_of(q);
    const ulonglong2 *W = INV ? T.iv.data() : T.fw.data(), *W1 = W + (n >> 1);
    const bool fuse1 = FUSE1 && ntt_fused_stage(logn);
    auto fin = [&](u64 v) -> u64 { if (LAZY) return reduce_small(v, q, q2, rq); v = v >= q2 ? v - q2 : v; return v >= q ? v - q : v; };
    for (auto &v : sm) v = 0xdeadbeefdeadbeefULL;
    if (FUSE1) {
        for (int s = 0; s < n; s += 2) { ulonglong2 v{in[s], in[s + 1]}; if (INV && fuse1) inv_pair_stage<LAZY>(v, W1[s >> 1], q, q2); sm_store_pair64(sm.data(), s, v.x, v.y); }
    } else for (int s = 0; s < n; s++) sm[lpad(s)] = in[s];
    ntt_row_passes<INV, LAZY, 3, FUSE1>(sm.data(), W, n, logn, q, q2);
    if (FUSE1) {
        for (int s = 0; s < n; s += 2) { ulonglong2 v = sm_load_pair64(sm.data(), s); if (!INV && fuse1) fwd_pair_stage<LAZY>(v, W1[s >> 1], q, q2); out[s] = fin(v.x); out[s + 1] = fin(v.y); }
    } else for (int s = 0; s < n; s++) out[s] = fin(sm[lpad(s)]);
}

template <bool LAZY, bool FUSE1>
static int rows_check_one(u64 q, int n, int logn, const Tables &T)
{
    std::vector<u64> sm(n), got(n), back(n);
    std::vector<std::vector<u64>> rows(3, std::vector<u64>(n));
    for (int i = 0; i < n; i++) { rows[0][i] = q - 1; rows[1][i] = (i & 1) ? q - 1 : 0; rows[2][i] = rnd() % q; }
    for (size_t r = 0; r < rows.size(); r++) {
        std::vector<u64> want(rows[r]);
        ref_fwd(want, T, n, q);
        run_row<false, LAZY, FUSE1>(rows[r], got, sm, T, n, logn, q);
        if (got != want) { printf("FAILED forward rows q=%llx n=%d lazy=%d fuse1=%d row=%zu\n", (ull)q, n, (int)LAZY, (int)FUSE1, r); return 1; }
        // the same row read as an NTT-form row: the inverse against the textbook, then the forward transform back
        want = rows[r];
        ref_inv(want, T, n, q);
        run_row<true, LAZY, FUSE1>(rows[r], got, sm, T, n, logn, q);
        if (got != want) { printf("FAILED inverse rows q=%llx n=%d lazy=%d fuse1=%d row=%zu\n", (ull)q, n, (int)LAZY, (int)FUSE1, r); return 1; }
        run_row<false, LAZY, FUSE1>(got, back, sm, T, n, logn, q);
        if (back != rows[r]) { printf("FAILED round trip q=%llx n=%d lazy=%d fuse1=%d row=%zu\n", (ull)q, n, (int)LAZY, (int)FUSE1, r); return 1; }
    }
    return 0;
}

template <bool LAZY>
static int rows_check(u64 q, int &transforms)
{
    for (const int n : {64, 128, 256, 8192, 16384}) {
        int logn = 0; while ((1 << logn) < n) logn++;
        const u64 psi = find_root(q, n);
        if (!psi || powm(psi, n, q) != q - 1) { printf("FAILED no 2n-th root q=%llx n=%d\n", (ull)q, n); return 1; }
        const Tables T = make_tables(q, n, logn, psi);
        if (rows_check_one<LAZY, false>(q, n, logn, T) || rows_check_one<LAZY, true>(q, n, logn, T)) return 1;
        transforms += 2 * 3 * 3;
    }
    return 0;
}

// inv_stages_unscaled<R> with the constant a kernel passes, every operand at the documented bound (16 q - 1 and its neighbours below, congruent to chosen
// residues): every butterfly recomputed in 128 bits beside the call -- no sum reaches 2^64, no difference operand exceeds kq -- and every result congruent to the
// textbook butterfly's
template <int R>
static int unscaled_check(u64 q, const Tables &T, int h, int blk, u64 kq, int &butterflies)
{
    constexpr int N = 1 << R;
    const ulonglong2 *W = T.ivu.data();
    for (int trial = 0; trial < 64; trial++) {
        u64 res[N], v[N], sh[N];
        for (int c = 0; c < N; c++) {
            res[c] = trial == 0 ? q - 1 : trial == 1 ? ((c & 1) ? 0 : q - 1) : trial == 2 ? ((c & 1) ? q - 1 : 0) : trial == 3 ? (c ? 0 : q - 1) : rnd() % q;
            v[c] = sh[c] = 15 * q + res[c];                                         // 16 q - 1 for the residue q - 1
        }
        inv_stages_unscaled<R>(v, W, h, blk, q, kq);
        for (int st = 0; st < R; st++) {
            const int half = 1 << st;
            for (int c = 0; c < N; c++) {
                if (c & half) continue;
                const int wi = (h >> st) + (blk << (R - 1 - st)) + (c >> (st + 1));
                const u64 w = W[wi].x, wp = W[wi].y;
                const u128 U = sh[c], V = sh[c + half], sum = U + V, T128 = (u128)kq - V + U;
                if (V > (u128)kq || (sum >> 64) || (T128 >> 64)) {
                    printf("FAILED unscaled range R=%d q=%llx stage %d c=%d\n", R, (ull)q, st, c); return 1;
                }
                sh[c] = (u64)sum; sh[c + half] = shoup_lazy4((u64)T128, w, wp, q);
                const u64 ru = res[c], rv = res[c + half];
                res[c] = (ru + rv) % q; res[c + half] = mulm((ru + q - rv) % q, w, q);
                if ((u128)sh[c + half] >= (u128)4 * q) { printf("FAILED unscaled product range R=%d q=%llx\n", R, (ull)q); return 1; }
                butterflies++;
            }
        }
        for (int c = 0; c < N; c++)
            if (v[c] != sh[c] || v[c] % q != res[c]) { printf("FAILED unscaled R=%d q=%llx trial %d c=%d got %llx shadow %llx residue %llx\n", R, (ull)q, trial, c, (ull)v[c], (ull)sh[c], (ull)res[c]); return 1; }
        if ((u128)v[0] >= ((u128)q << (R + 4))) { printf("FAILED unscaled sum bound R=%d\n", R); return 1; }
    }
    return 0;
}

int main(int argc, char **argv)
{
    threadIdx = dim3(0, 0, 0); blockIdx = dim3(0, 0, 0); blockDim = dim3(1); gridDim = dim3(1);
    // the width classes ntt_launch admits to the lazy butterflies (45..57 bits) and to the strict ones (below and above); all = 1 mod 32768
    std::vector<u64> lazy = {0x100000020001ULL, 0x1ffffff18001ULL, 0xffffffff58001ULL, 0x1ffffffff38001ULL, 0x3fffffff000001ULL, 0x7fffffffe90001ULL, 0x80000000068001ULL,
                             0x1fffffffffc0001ULL};
    std::vector<u64> strict = {0xfffffdf8001ULL, 0x200000000208001ULL, 0xffffffffffe8001ULL};
    const bool only_lazy = argc >= 3 && !strcmp(argv[1], "lazy");
    if (only_lazy) { lazy = {strtoull(argv[2], 0, 0)}; strict.clear(); }
    else for (const u64 q : lazy) if (bits_of(q) < 45 || bits_of(q) > 57) { puts("FAILED table"); return 2; }
    int maxk_min = 4, transforms = 0, butterflies = 0;
    for (const u64 q : lazy) {
        int maxk = 0;
        if (reduce_small_check(q) || shoup_lazy4_check(q, maxk) || rows_check<true>(q, transforms)) return 1;
        printf("lazy q=%llx bits=%d max floor(r/q)=%d\n", (ull)q, bits_of(q), maxk);
        if (maxk < maxk_min) maxk_min = maxk;
    }
    for (const u64 q : strict) {
        if (rows_check<false>(q, transforms)) return 1;
        printf("strict q=%llx bits=%d\n", (ull)q, bits_of(q));
    }
    if (!only_lazy) {
        const u64 q = 0x7fffffffe90001ULL;                            // the largest prime below 2^55 the unscaled inverse can meet
        for (const int n : {8192, 16384}) {
            int logn = 0; while ((1 << logn) < n) logn++;
            const Tables T = make_tables(q, n, logn, find_root(q, n));
            // the wave-local passes (u64_local_passes_inv_unscaled: gaps 2, 16, 128; tabidx = n >> (ls + 1), first, a middle and the last block of the row)
            for (const int ls : {1, 4, 7}) {
                const int nblk = n >> (ls + 3);
                for (const int blk : {0, nblk / 2, nblk - 1}) if (unscaled_check<3>(q, T, n >> (ls + 1), blk, q << 6, butterflies)) return 1;
            }
            // the cross stages (ntt_rows_wave_kernel: CS = log2 n - 10, table index n >> 11, block 0, kq = q << (CS + 3))
            if (n == 8192) { if (unscaled_check<3>(q, T, n >> 11, 0, q << 6, butterflies)) return 1; }
            else if (unscaled_check<4>(q, T, n >> 11, 0, q << 7, butterflies)) return 1;
        }
    }
    printf("ok primes %zu strict %zu transforms %d unscaled_butterflies %d min_max_k %d\n", lazy.size(), strict.size(), transforms, butterflies, maxk_min);
    return 0;
}
