// kernels_budget.hip -- Decryptor::invariant_noise_budget (SEAL decryptor.cpp:295-403) for whole tensors of ciphertexts on gfx950.
//
// Per ciphertext:  v = c0 + c1 s (+ c2 s^2) mod q in coefficient form (k_decrypt_rows, the decryptor's own dot product and inverse transforms), then per
// coefficient the CRT composition of t v mod q as a K-word integer, centred against floor(q/2) (budget_bits.h), the infinity norm over the n coefficients and
//     budget = max(0, bits(q) - bits(norm) - 1).
// Exact integer arithmetic: the number SEAL and crc_noise_budget report, bit for bit.  Only BIT LENGTHS leave a lane -- the maximum of the bit lengths is the
// bit length of the maximum -- so the reduction over a ciphertext is a 32-bit integer maximum (wave shuffles, then LDS) and no multi-word compare crosses lanes.
#include "kernels.h"
#include "budget_bits.h"

// one workgroup per ciphertext: bits[m] = budget of V[m] ([k][n] coefficient-form residues of c0 + c1 s)
template <int K>
__global__ void __launch_bounds__(256) budget_norm_kernel(const u64 *V, int32_t *bits, int n, BudgetParams bp)
{
    __shared__ int wave_max[4];
    const u64 *v = V + (size_t)blockIdx.x * K * n;
    int mx = 0;
    for (int s = threadIdx.x; s < n; s += 256) {
        const int b = budget_coeff_bits<K>(v + s, (size_t)n, bp);
        mx = b > mx ? b : mx;
    }
    for (int o = 32; o; o >>= 1) { const int other = __shfl_xor(mx, o); mx = other > mx ? other : mx; }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) mx = wave_max[w] > mx ? wave_max[w] : mx;
        const int b = bp.total_bits - mx - 1;
        bits[blockIdx.x] = b > 0 ? b : 0;
    }
}

// one workgroup (16 waves: enough loads in flight for a tensor of a million ciphertexts): out = {min of bits[count], index of its first occurrence}.  A launch of
// its own rather than atomics in budget_norm_kernel: the pair does not depend on the order the ciphertexts' workgroups finish in
__global__ void __launch_bounds__(1024) budget_min_kernel(const int32_t *bits, size_t count, int32_t *out)
{
    __shared__ int wave_v[16], wave_i[16];
    int bv = 0x7fffffff, bi = 0x7fffffff;
    for (size_t m = threadIdx.x; m < count; m += 1024) {    // ascending m per lane: a strict compare keeps the first
        const int v = bits[m];
        if (v < bv) { bv = v; bi = (int)m; }
    }
    for (int o = 32; o; o >>= 1) {
        const int ov = __shfl_xor(bv, o), oi = __shfl_xor(bi, o);
        if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { wave_v[threadIdx.x >> 6] = bv; wave_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) if (wave_v[w] < bv || (wave_v[w] == bv && wave_i[w] < bi)) { bv = wave_v[w]; bi = wave_i[w]; }
        out[0] = bv; out[1] = bi;
    }
}

static BudgetParams budget_params(const crc_ctx *c)
{
    BudgetParams bp{};
    const int k = c->k;
    bp.k = k; bp.total_bits = c->total_bits;
    for (int i = 0; i < k; i++) {
        bp.qi[i] = c->q[i]; bp.xc[i] = c->behz.t_inv_qhat[i]; bp.xc_s[i] = c->behz.t_inv_qhat_s[i];
        bp.q[i] = c->qbig[i];
        u64 *h = bp.qhat[i]; h[0] = 1;                      // q/q_i = prod_{j != i} q_j
        for (int j = 0; j < k; j++) if (j != i) {
            u64 cy = 0;
            for (int l = 0; l < k; l++) { const unsigned __int128 z = (unsigned __int128)h[l] * c->q[j] + cy; h[l] = (u64)z; cy = (u64)(z >> 64); }
        }
    }
    for (int l = 0; l < k; l++) bp.half[l] = (bp.q[l] >> 1) | (l + 1 < k ? bp.q[l + 1] << 63 : 0);
    return bp;
}

// bits [cnt] (and min_out {min, first index} when not NULL) of the ciphertexts ct [cnt][size][k][n]; work: k_decrypt_work_words
int k_noise_budget(crc_ctx *c, const u64 *sk, const u64 *ct, size_t cnt, int size, bool in_ntt, int32_t *bits, int32_t *min_out, u64 *work, hipStream_t st)
{
    if (cnt == 0) return CRC_OK;
    int rc;
    if ((rc = k_decrypt_rows(c, sk, ct, cnt, size, in_ntt, work, st))) return rc;       // checks size and cnt k < 2^31
    const BudgetParams bp = budget_params(c);
    const dim3 g((unsigned)cnt), b(256);
    switch (c->k) {
#define CRC_BUDGET_CASE(K) case K: hipLaunchKernelGGL(budget_norm_kernel<K>, g, b, 0, st, work, bits, c->n, bp); break;
        CRC_BUDGET_CASE(1) CRC_BUDGET_CASE(2) CRC_BUDGET_CASE(3) CRC_BUDGET_CASE(4) CRC_BUDGET_CASE(5) CRC_BUDGET_CASE(6) CRC_BUDGET_CASE(7) CRC_BUDGET_CASE(8)
#undef CRC_BUDGET_CASE
        default: return CRC_ERR_INVALID_ARGUMENT;
    }
    HIPCHK(hipGetLastError());
    if (min_out) {
        hipLaunchKernelGGL(budget_min_kernel, dim3(1), dim3(1024), 0, st, bits, cnt, min_out);
        HIPCHK(hipGetLastError());
    }
    return CRC_OK;
}

// the same per-coefficient routine on the host: h_v [cnt][k][n] coefficient-form residues -> h_bits [cnt]
int k_budget_bits_host(const crc_ctx *c, const u64 *h_v, size_t cnt, int32_t *h_bits)
{
    const BudgetParams bp = budget_params(c);
    const int n = c->n, k = c->k;
    for (size_t m = 0; m < cnt; m++) {
        const u64 *v = h_v + m * (size_t)k * n;
        int mx = 0;
        for (int s = 0; s < n; s++) {
            int b;
            switch (k) {
#define CRC_BUDGET_CASE(K) case K: b = budget_coeff_bits<K>(v + s, (size_t)n, bp); break;
                CRC_BUDGET_CASE(1) CRC_BUDGET_CASE(2) CRC_BUDGET_CASE(3) CRC_BUDGET_CASE(4) CRC_BUDGET_CASE(5) CRC_BUDGET_CASE(6) CRC_BUDGET_CASE(7) CRC_BUDGET_CASE(8)
#undef CRC_BUDGET_CASE
                default: return CRC_ERR_INVALID_ARGUMENT;
            }
            mx = b > mx ? b : mx;
        }
        const int b = c->total_bits - mx - 1;
        h_bits[m] = b > 0 ? b : 0;
    }
    return CRC_OK;
}
