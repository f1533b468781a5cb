// kernels_flood.hip -- noise flooding of whole ciphertext tensors on gfx950, its admission arithmetic, and its host twin.
//
// The server's last step before a response leaves: every size-2 ciphertext (c0, c1) takes a fresh public-key encryption of zero whose first error term is
// uniform on [-2^B, 2^B),  c0' = c0 + p0 u + e1,  c1' = c1 + p1 u + e2.  The fresh u re-randomises c1; e1, far wider than any noise the evaluation can have left,
// drowns the weight-dependent noise statistically.  In place, in the tensor's own form (flood_device.h has the kernels' bodies):
//   CRC_NTT     flood_sample_kernel, the row transform on U, flood_join_kernel<forward>: 3 forward transforms per modulus, none back, the tensor read once
//   CRC_COEFF   flood_sample_kernel, the row transform on U, flood_join_kernel<inverse>: 1 forward and 2 inverse transforms per modulus
// Exact integers throughout; the host twin below computes the same bits from the same keystream in 128-bit integer arithmetic.
#include <algorithm>
#include <cstring>
#include <vector>
#include "kernels.h"
#include "host_parallel.h"
#include "work_arena.h"
#include "flood_device.h"

typedef unsigned __int128 u128;

__global__ void __launch_bounds__(256) flood_sample_kernel(FloodArgs a) { flood_sample_body(a); }
template <bool INV, bool LAZY>
__global__ void __launch_bounds__(1024) flood_join_kernel(FloodArgs a)
{
    extern __shared__ u64 sm[];
    flood_join_body<INV, LAZY>(a, sm);
}

// ---- admission and the two pure functions of (context, budget, B): little-endian multi-word integers, a handful of words -----------------------------------
namespace {
typedef std::vector<u64> Big;
void big_trim(Big &a) { while (a.size() > 1 && !a.back()) a.pop_back(); }
Big big_of(u128 v) { Big a{(u64)v, (u64)(v >> 64)}; big_trim(a); return a; }
Big big_mul(const Big &a, u64 m)
{
    Big r(a.size() + 1); u64 carry = 0;
    for (size_t l = 0; l < a.size(); l++) { const u128 p = (u128)a[l] * m + carry; r[l] = (u64)p; carry = (u64)(p >> 64); }
    r[a.size()] = carry; big_trim(r); return r;
}
Big big_add(const Big &a, const Big &b)
{
    Big r(std::max(a.size(), b.size()) + 1); u64 carry = 0;
    for (size_t l = 0; l + 1 < r.size(); l++) { const u128 s = (u128)(l < a.size() ? a[l] : 0) + (l < b.size() ? b[l] : 0) + carry; r[l] = (u64)s; carry = (u64)(s >> 64); }
    r.back() = carry; big_trim(r); return r;
}
Big big_shl(const Big &a, int bits)
{
    const int words = bits / 64, sh = bits % 64;
    Big r(a.size() + words + 1, 0);
    for (size_t l = 0; l < a.size(); l++) { r[l + words] |= a[l] << sh; if (sh) r[l + words + 1] |= a[l] >> (64 - sh); }
    big_trim(r); return r;
}
int big_cmp(const Big &a, const Big &b)
{
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t l = a.size(); l-- > 0;) if (a[l] != b[l]) return a[l] < b[l] ? -1 : 1;
    return 0;
}
int sig_bits(u64 v) { return v ? 64 - __builtin_clzll(v) : 0; }
// t (2^B + 38 n): the largest |t w| the flood itself can add (|w| <= 2^B + 38 n per coefficient: e1 in [-2^B, 2^B), e_pk u and e2 s each at most 19 n)
Big flood_term(const crc_ctx *c, int B) { return big_mul(big_of(((u128)1 << B) + (u128)38 * (u128)c->n), c->t); }
Big big_q(const crc_ctx *c) { Big q(c->qbig); big_trim(q); return q; }
}

// 1 <= B <= 126 and t (2^B + 38 n) < q / 2: past that the flood alone could flip a plaintext coefficient
bool k_flood_supported(const crc_ctx *c, int B)
{
    if (!c || B < 1 || B > 126 || c->k > CRC_MAXK) return false;
    return big_cmp(big_shl(flood_term(c, B), 1), big_q(c)) < 0;
}
// A ciphertext with b bits of budget has |t w| of total_bits - b - 1 bits, so |w| <= W = floor((2^(total_bits - b - 1) - 1) / t), an integer of
// max(0, total_bits - b - bits(t)) bits; the smallest B with 2^B > 2^lambda W is lambda plus that bit count
int k_flood_bits(const crc_ctx *c, int budget_in, int lambda)
{
    if (!c || budget_in < 0 || budget_in > c->total_bits || lambda < 0 || lambda > 126) return CRC_ERR_INVALID_ARGUMENT;
    const int nb = c->total_bits - budget_in - sig_bits(c->t), B = (nb > 0 ? nb : 0) + lambda;
    return k_flood_supported(c, B) ? B : CRC_ERR_INVALID_ARGUMENT;
}
// floor(-log2(2^-b + t (2^B + 38 n) / q)), not below 0: the largest j with (q + 2^b T) 2^j <= 2^b q, T = t (2^B + 38 n)
int k_flood_budget_bound(const crc_ctx *c, int budget_in, int B)
{
    if (!c || budget_in < 0 || budget_in > c->total_bits || !k_flood_supported(c, B)) return CRC_ERR_INVALID_ARGUMENT;
    const Big q = big_q(c), lhs = big_add(q, big_shl(flood_term(c, B), budget_in)), rhs = big_shl(q, budget_in);
    int j = 0;
    while (big_cmp(big_shl(lhs, j + 1), rhs) <= 0) j++;
    return j;
}

// The work space of one call: the ternary rows and the residues of both error terms
struct FloodLayout {
    u64 *U, *E;
    FloodLayout(WorkArena &w, const crc_ctx *c, size_t cnt)
    {
        U = w.take<u64>(cnt * (size_t)c->k * c->n);
        E = w.take<u64>(cnt * 2 * (size_t)c->k * c->n);
    }
};
size_t k_flood_work_bytes(const crc_ctx *c, size_t cnt)
{
    WorkArena w; FloodLayout L(w, c, cnt); (void)L;
    return w.bytes();
}

static u64 shoup_of(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }

// d_ct [cnt][2][k][n] in CRC_NTT (ntt_form) or CRC_COEFF, in place; the caller has checked B, the pointers and their alignment
int k_flood(crc_ctx *c, const u64 *d_pk, u64 *d_ct, size_t cnt, bool ntt_form, int B, const ChaChaKey &key, u64 stream_base, void *d_work, hipStream_t st)
{
    if (cnt == 0) return CRC_OK;
    const int n = c->n, k = c->k;
    const size_t lds = (size_t)n * 8;
    if (lds > 128 * 1024) return CRC_ERR_UNSUPPORTED;                               // (n = 32768: a row does not fit the LDS; the host twin serves it)
    const int pairs = n / 2, threads = pairs < 256 ? pairs : 256, pblocks = (pairs + threads - 1) / threads;
    if (cnt * (size_t)pblocks > 0x7fffffffULL || (cnt * (size_t)k + 7) / 8 * 16 > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena w(d_work);
    const FloodLayout L(w, c, cnt);
    FloodArgs a{};
    a.ct = d_ct; a.pk = d_pk; a.U = L.U; a.E = L.E; a.count = cnt; a.n = n; a.logn = c->logn; a.k = k; a.flood_bits = B; a.stream_base = stream_base; a.key = key;
    k_encrypt_cdt(a.cdt.t);
    bool lazy = true;
    for (int i = 0; i < k; i++) {
        const u64 q = c->q[i];
        a.mods[i] = c->tabs[i].m; a.one_s[i] = shoup_of(1, q); a.pow2b[i] = h_powmod(2, (u64)B, q);
        lazy = lazy && c->tabs[i].m.bits <= 57;
    }
    a.W = (const ulonglong2 *)(ntt_form ? c->d_rp : c->d_irp2);
    hipLaunchKernelGGL(flood_sample_kernel, dim3((unsigned)(cnt * pblocks)), dim3(threads), 0, st, a);
    HIPCHK(hipGetLastError());
    { const int rc = k_ntt_ct(c, false, L.U, L.U, cnt, 1, false, st, nullptr, 0, 0, 0); if (rc) return rc; }
    int nt = n / 8; if (nt < 64) nt = 64; if (nt > 1024) nt = 1024;
    auto kern = ntt_form ? (lazy ? flood_join_kernel<false, true> : flood_join_kernel<false, false>) : (lazy ? flood_join_kernel<true, true> : flood_join_kernel<true, false>);
    { const int rc = crc_ctx_ensure_lds(c, (const void *)kern, lds); if (rc) return rc; }
    hipLaunchKernelGGL(kern, dim3(xcd_grid(cnt * (size_t)k, 2)), dim3(nt), lds, st, a);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}

// ---- host twin (any context, device = -1 included): the same keystream, decoded by the layout of chacha.h, 128-bit integer arithmetic, the reference
// transforms of ctx.cpp
int k_flood_host(const crc_ctx *c, const u64 *pk, u64 *ct, size_t cnt, bool ntt_form, int B, const ChaChaKey &key, u64 stream_base)
{
    const int n = c->n, k = c->k;
    u64 T[19]; k_encrypt_cdt(T);
    const u128 xmask = (((u128)1 << B) << 1) - 1, half = (u128)1 << B;
    crc_host::parallel_for(cnt, 1, [&](size_t m0, size_t m1) {
        std::vector<int> u(n), e2(n);
        std::vector<u128> x(n);
        std::vector<u64> ur(n), er(n);
        for (size_t m = m0; m < m1; m++) {
            const u64 sid = stream_base + m;
            for (int s = 0; s < n; s += 2) {
                u32 b[16];
                chacha20_block(key, 0, (u32)sid, (u32)(sid >> 32), ((u32)CHACHA_DOM_FLOOD << 24) | (u32)s, b);
                for (int c2 = 0; c2 < 2; c2++) {
                    const u32 *w = b + 8 * c2;
                    const u64 tw = (u64)w[0] | ((u64)w[1] << 32), mw = (u64)w[2] | ((u64)w[3] << 32);
                    int tv = 0;
                    for (int j = 0; j < 32; j++) { const int f = (int)((tw >> (2 * j)) & 3); if (f != 3) { tv = f; break; } }
                    u[s + c2] = tv == 2 ? -1 : tv;
                    int mag = 0; for (int j = 0; j < 19; j++) mag += mw >= T[j] ? 1 : 0;
                    e2[s + c2] = (w[7] >> 31) ? -mag : mag;
                    x[s + c2] = ((u128)w[4] | ((u128)w[5] << 32) | ((u128)w[6] << 64) | ((u128)w[7] << 96)) & xmask;
                }
            }
            for (int i = 0; i < k; i++) {
                const u64 q = c->q[i];
                for (int s = 0; s < n; s++) ur[s] = u[s] == 0 ? 0 : (u[s] == 1 ? 1 : q - 1);
                h_ntt_fwd(c->tabs[i], ur.data(), n);
                for (int p = 0; p < 2; p++) {
                    u64 *row = ct + ((m * 2 + p) * (size_t)k + i) * n; const u64 *kr = pk + ((size_t)p * k + i) * n;
                    // e_p mod q_i: e1 = x - 2^B from the 128-bit integers, e2 a small signed integer
                    for (int s = 0; s < n; s++) {
                        if (p == 0) er[s] = (u64)((x[s] % q + q - (u64)(half % q)) % q);
                        else er[s] = e2[s] >= 0 ? (u64)e2[s] : q - (u64)(-e2[s]);
                    }
                    if (ntt_form) {
                        h_ntt_fwd(c->tabs[i], er.data(), n);
                        for (int s = 0; s < n; s++) row[s] = (u64)(((u128)row[s] + er[s] + h_mulmod(ur[s], kr[s], q)) % q);
                    } else {
                        std::vector<u64> pr(n);
                        for (int s = 0; s < n; s++) pr[s] = h_mulmod(ur[s], kr[s], q);
                        h_ntt_inv(c->tabs[i], pr.data(), n);
                        for (int s = 0; s < n; s++) row[s] = (u64)(((u128)row[s] + er[s] + pr[s]) % q);
                    }
                }
            }
        }
    });
    return CRC_OK;
}
