// kernels_slots.hip -- slot batching (SEAL's PolyCRTBuilder, polycrt.cpp:82-147, 327-370) for whole tensors of plaintexts on gfx950, and its host twins.
//
// For a prime plain modulus t = 1 mod 2n a plaintext polynomial p is n independent numbers of Z_t: slot i is p(psi^(3^i)), slot n/2 + i is p(psi^(-3^i)), psi
// the minimal primitive 2n-th root of unity mod t.  compose: values -> the row positions idx[i] -> inverse negacyclic transform mod t -> coefficients;
// decompose: coefficients -> forward transform -> positions idx[i] -> centred values.  One workgroup per row, the row in LDS, ntt_device.h's passes with t's
// tables; the permutation, the reduction of the int64 inputs mod t, the zero fill and the centring sit in the loops that fill / drain the image, so a row costs
// one read and one write of 8 n bytes and nothing else touches memory.
//
// A device kernel cannot throw: where SEAL refuses a value outside the plain modulus, every int64 is accepted here and taken as its residue mod t.
#include "kernels.h"
#include "host_parallel.h"
#include "slots_device.h"      // SlotArgs, the block -> item order, the two kernel bodies

template <bool LAZY>
__global__ void __launch_bounds__(1024) slots_compose_kernel(SlotArgs a)
{
    extern __shared__ u64 sm[];
    slots_compose_body<LAZY>(a, sm);
}
template <bool LAZY>
__global__ void __launch_bounds__(1024) slots_decompose_kernel(SlotArgs a)
{
    extern __shared__ u64 sm[];
    slots_decompose_body<LAZY>(a, sm);
}
template <bool LAZY>
__global__ void __launch_bounds__(1024) slots_rescale_kernel(SlotRescaleArgs a)
{
    extern __shared__ u64 sm[];
    slots_rescale_body<LAZY>(a, sm);
}
template <bool LAZY, int PAIRS>                             // PAIRS = 4: a lane's share up to n = 8192; 8: of n = 16384 at 1024 threads; 0: the window is one row
__global__ void __launch_bounds__(1024) slots_act_kernel(SlotActArgs a)
{
    extern __shared__ u64 sm[];
    slots_act_body<LAZY, PAIRS>(a, sm);
}

template <bool LAZY, int PAIRS>                             // PAIRS: the pairs a lane keeps running values for -- 4 up to n = 4096, 8 above (k_slots_crt_decompose)
__global__ void __launch_bounds__(1024) slots_crt_decompose_kernel(SlotCrtArgs a)
{
    extern __shared__ u64 sm[];
    slots_crt_decompose_body<LAZY, PAIRS>(a, sm);
}
template <bool LAZY, int PAIRS>
__global__ void __launch_bounds__(1024) slots_crt_act_kernel(SlotCrtArgs a)
{
    extern __shared__ u64 sm[];
    slots_crt_act_body<LAZY, PAIRS>(a, sm);
}

// The launch rules of the slot kernels in one place: the tables of every plain modulus the kernel visits (one context, or the r contexts of a residue base), one
// workgroup of max(64, n / 8) threads per row with the row as its LDS image, the rows in XCD groups.  `tables(a, j, T)` puts what the kernel reads of modulus j
// into the argument block; the ring's fields and the kernel's variant -- lazy where every modulus is below 2^57 -- are chosen here.  `threads` (0: the rule
// above) is for the kernels that keep a lane's running values in registers and want fewer, wider lanes.
template <class Args, class Tables>
static int slots_launch(crc_ctx *const *ctxs, int r, void (*lazy)(Args), void (*strict)(Args), Args &a, Tables tables, hipStream_t st, int threads = 0)
{
    const SlotTables *T[CRC_SLOTS_CRT_MAX];
    for (int j = 0; j < r; j++) { const int rc = crc_slots_tables(ctxs[j], &T[j]); if (rc) return rc; }
    if (a.count == 0) return CRC_OK;
    crc_ctx *c = ctxs[0];
    const size_t lds = (size_t)c->n * 8;
    if (lds > 128 * 1024) return CRC_ERR_UNSUPPORTED;                 // (n = 32768: the row does not fit the LDS; the host twins serve it)
    const size_t groups = (a.count + CRC_SLOT_GROUP - 1) / CRC_SLOT_GROUP;
    if ((groups + 7) / 8 * 8 * CRC_SLOT_GROUP > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    bool all_lazy = true;
    for (int j = 0; j < r; j++) { tables(a, j, *T[j]); all_lazy = all_lazy && T[j]->lazy; }
    a.n = c->n; a.logn = c->logn;
    int nt = threads ? threads : c->n / 8; if (nt < 64) nt = 64; if (nt > 1024) nt = 1024;
    auto kern = all_lazy ? lazy : strict;
    { const int rc = crc_ctx_ensure_lds(c, (const void *)kern, lds); if (rc) return rc; }
    hipLaunchKernelGGL(kern, dim3(xcd_grid(groups, CRC_SLOT_GROUP)), dim3(nt), lds, st, a);
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
// the kernels of one plain modulus: the context's t and its Shoup companion of 1 go into the argument block with the tables
template <class Args, class Tables>
static int slots_launch(crc_ctx *c, void (*lazy)(Args), void (*strict)(Args), Args &a, Tables tables, hipStream_t st)
{
    return slots_launch(&c, 1, lazy, strict, a, [&](Args &a, int, const SlotTables &T) { tables(a, T); a.t = c->t; a.one_s = T.one_s; }, st);
}

int k_slots_compose(crc_ctx *c, const long long *d_values, size_t count, int slots, size_t item_stride, size_t slot_stride, u64 *d_plain, hipStream_t st)
{
    SlotArgs a{};
    a.vals_in = d_values; a.plain_out = d_plain; a.count = count; a.slots = slots; a.item_stride = item_stride; a.slot_stride = slot_stride;
    return slots_launch(c, slots_compose_kernel<true>, slots_compose_kernel<false>, a, [](SlotArgs &a, const SlotTables &T) { a.W = T.d_inv; a.idx = T.d_idx; }, st);
}
int k_slots_decompose(crc_ctx *c, const u64 *d_plain, size_t count, int slots, long long *d_values, size_t item_stride, size_t slot_stride, hipStream_t st)
{
    SlotArgs a{};
    a.plain_in = d_plain; a.vals_out = d_values; a.count = count; a.slots = slots; a.item_stride = item_stride; a.slot_stride = slot_stride;
    return slots_launch(c, slots_decompose_kernel<true>, slots_decompose_kernel<false>, a, [](SlotArgs &a, const SlotTables &T) { a.W = T.d_fwd; a.idx = T.d_idx; }, st);
}

// every slot of count plaintexts divided by `divisor`, rounded to nearest (slots_device.h); d_in == d_out allowed
int k_slots_rescale(crc_ctx *c, const u64 *d_in, size_t count, u64 divisor, u64 *d_out, hipStream_t st)
{
    SlotRescaleArgs a{};
    a.plain_in = d_in; a.plain_out = d_out; a.count = count;
    a.D = divisor; a.recip = divisor == 1 ? ~(u64)0 : (u64)(((unsigned __int128)1 << 64) / divisor);
    a.hpos = divisor >> 1; a.hneg = (divisor - 1) >> 1;
    return slots_launch(c, slots_rescale_kernel<true>, slots_rescale_kernel<false>, a, [](SlotRescaleArgs &a, const SlotTables &T) { a.Wf = T.d_fwd; a.Wi = T.d_inv; }, st);
}

// the maximum over a window of plaintext rows, slot by slot, divided, ReLU, cap (slots_device.h): one workgroup per OUTPUT row, no work buffer.  The caller has
// checked the window (Window::ok) and that the two tensors do not overlap, or coincide for a 1 x 1 window of stride 1
int k_slots_act(crc_ctx *c, const u64 *d_in, size_t planes, const Window &w, u64 divisor, int relu, u64 cap, u64 *d_out, hipStream_t st)
{
    SlotActArgs a{};
    a.plain_in = d_in; a.plain_out = d_out; a.count = planes * (size_t)w.P64();
    a.D = divisor; a.recip = divisor == 1 ? ~(u64)0 : (u64)(((unsigned __int128)1 << 64) / divisor);
    a.xd = w.xd; a.yd = w.yd; a.xs = w.xs; a.ys = w.ys; a.xf = w.xf; a.yf = w.yf; a.xo = w.xo(); a.yo = w.yo();
    a.relu = relu; a.cap = cap;
    auto tables = [](SlotActArgs &a, const SlotTables &T) { a.Wf = T.d_fwd; a.Wi = T.d_inv; };
    // a window of one row at stride 1 (outputs and inputs have the same row index) needs no running maximum
    if (w.xf == 1 && w.yf == 1 && w.xs == 1 && w.ys == 1) return slots_launch(c, slots_act_kernel<true, 0>, slots_act_kernel<false, 0>, a, tables, st);
    // pairs a lane owns: n / (2 max(64, n / 8)), i.e. at most 4 up to n = 8192; 8 at n = 16384, where the workgroup stops at 1024 threads
    if (c->n <= 8192) return slots_launch(c, slots_act_kernel<true, 4>, slots_act_kernel<false, 4>, a, tables, st);
    return slots_launch(c, slots_act_kernel<true, 8>, slots_act_kernel<false, 8>, a, tables, st);
}

// ---- host twins (any context, device = -1 included): the reference transforms of ctx.cpp on the same tables ----------------------------------------------
int k_slots_compose_host(crc_ctx *c, const long long *values, size_t count, int slots, size_t item_stride, size_t slot_stride, u64 *plain)
{
    const SlotTables *T;
    { const int rc = crc_slots_tables(c, &T); if (rc) return rc; }
    const int n = c->n; const long long t = (long long)c->t;
    crc_host::parallel_for(count, 4, [&](size_t b, size_t e) {
        for (size_t m = b; m < e; m++) {
            u64 *row = plain + m * (size_t)n;
            for (int i = 0; i < n; i++) row[i] = 0;
            for (int i = 0; i < slots; i++) { long long r = values[m * item_stride + (size_t)i * slot_stride] % t; if (r < 0) r += t; row[T->idx[i]] = (u64)r; }
            h_ntt_inv(T->T, row, n);
        }
    });
    return CRC_OK;
}
int k_slots_decompose_host(crc_ctx *c, const u64 *plain, size_t count, int slots, long long *values, size_t item_stride, size_t slot_stride)
{
    const SlotTables *T;
    { const int rc = crc_slots_tables(c, &T); if (rc) return rc; }
    const int n = c->n; const u64 t = c->t, half = (t - 1) >> 1;
    crc_host::parallel_for(count, 4, [&](size_t b, size_t e) {
        std::vector<u64> row((size_t)n);
        for (size_t m = b; m < e; m++) {
            for (int i = 0; i < n; i++) row[i] = plain[m * (size_t)n + i] % t;
            h_ntt_fwd(T->T, row.data(), n);
            for (int i = 0; i < slots; i++) { const u64 r = row[T->idx[i]]; values[m * item_stride + (size_t)i * slot_stride] = r > half ? (long long)r - (long long)t : (long long)r; }
        }
    });
    return CRC_OK;
}
int k_slots_rescale_host(crc_ctx *c, const u64 *plain_in, size_t count, u64 divisor, u64 *plain_out)
{
    const SlotTables *T;
    { const int rc = crc_slots_tables(c, &T); if (rc) return rc; }
    const int n = c->n; const u64 t = c->t, half = (t - 1) >> 1;
    const __int128 D = (__int128)divisor, h = (__int128)(divisor >> 1);
    crc_host::parallel_for(count, 4, [&](size_t b, size_t e) {
        std::vector<u64> row((size_t)n);
        for (size_t m = b; m < e; m++) {
            for (int i = 0; i < n; i++) row[i] = plain_in[m * (size_t)n + i] % t;
            h_ntt_fwd(T->T, row.data(), n);
            for (int i = 0; i < n; i++) {
                const __int128 num = (row[i] > half ? (__int128)row[i] - (__int128)t : (__int128)row[i]) + h;
                __int128 q = num / D; if (num % D < 0) q--;                    // floor division
                row[i] = (u64)(q < 0 ? q + (__int128)t : q);                   // |q| <= (t - 1) / 2
            }
            h_ntt_inv(T->T, row.data(), n);
            for (int i = 0; i < n; i++) plain_out[m * (size_t)n + i] = row[i];
        }
    });
    return CRC_OK;
}
int k_slots_act_host(crc_ctx *c, const u64 *plain_in, size_t planes, const Window &w, u64 divisor, int relu, u64 cap, u64 *plain_out)
{
    const SlotTables *T;
    { const int rc = crc_slots_tables(c, &T); if (rc) return rc; }
    const int n = c->n, xo = w.xo(), yo = w.yo(); const u64 t = c->t, half = (t - 1) >> 1;
    const __int128 D = (__int128)divisor, h = (__int128)(divisor >> 1);
    crc_host::parallel_for(planes * (size_t)w.P64(), 4, [&](size_t b, size_t e) {
        std::vector<u64> row((size_t)n);
        std::vector<long long> mx((size_t)n);
        for (size_t m = b; m < e; m++) {
            const size_t pl = m / ((size_t)xo * yo), ij = m % ((size_t)xo * yo);
            const int i = (int)(ij / yo), j = (int)(ij % yo);
            for (int wa = 0; wa < w.xf; wa++) for (int wb = 0; wb < w.yf; wb++) {
                const u64 *src = plain_in + ((pl * w.xd + (size_t)(i * w.xs + wa)) * w.yd + (size_t)(j * w.ys + wb)) * (size_t)n;
                for (int k = 0; k < n; k++) row[k] = src[k] % t;
                h_ntt_fwd(T->T, row.data(), n);
                for (int k = 0; k < n; k++) {
                    const long long v = row[k] > half ? (long long)row[k] - (long long)t : (long long)row[k];
                    if ((wa == 0 && wb == 0) || v > mx[k]) mx[k] = v;
                }
            }
            for (int k = 0; k < n; k++) {
                const __int128 num = (__int128)mx[k] + h;
                __int128 q = num / D; if (num % D < 0) q--;                    // floor division
                if (relu && q < 0) q = 0;
                if (cap && q > (__int128)cap) q = (__int128)cap;
                row[k] = (u64)(q < 0 ? q + (__int128)t : q);                   // |q| <= (t - 1) / 2
            }
            h_ntt_inv(T->T, row.data(), n);
            for (int k = 0; k < n; k++) plain_out[m * (size_t)n + k] = row[k];
        }
    });
    return CRC_OK;
}

// ---- several plain moduli (slots_device.h: slots_crt_*) ------------------------------------------------------------------------------------------------------
// The constants of a residue base: P_j = t_0 ... t_{j-1} and its inverse mod t_j.  false unless the t_j are pairwise distinct (primes: pairwise coprime) and
// their product stays below 2^63; the caller has checked the contexts themselves (crc_slots_crt_supported)
bool k_slots_crt_base(crc_ctx *const *ctxs, int r, SlotsCrtBase *B)
{
    if (r < 1 || r > CRC_SLOTS_CRT_MAX) return false;
    B->r = r;
    unsigned __int128 T = 1;
    for (int j = 0; j < r; j++) {
        const u64 t = ctxs[j]->t;
        for (int i = 0; i < j; i++) if (B->t[i] == t) return false;
        B->t[j] = t; B->P[j] = (u64)T;
        T *= t;
        if (T >> 63) return false;
        B->Pinv[j] = j ? h_invmod(B->P[j] % t, t) : 1;
        B->Pinv_s[j] = (u64)(((unsigned __int128)B->Pinv[j] << 64) / t);
    }
    B->T = (u64)T;
    return true;
}
static void slots_crt_args(const SlotsCrtBase &B, SlotCrtArgs &a)
{
    a.r = B.r; a.T = B.T; a.half = (B.T - 1) >> 1;
    for (int j = 0; j < B.r; j++) { a.m[j].P = B.P[j]; a.m[j].Pinv = B.Pinv[j]; a.m[j].Pinv_s = B.Pinv_s[j]; }
}
static const auto slots_crt_tables = [](SlotCrtArgs &a, int j, const SlotTables &T) {
    a.m[j].Wf = T.d_fwd; a.m[j].Wi = T.d_inv; a.m[j].one_s = T.one_s; a.m[j].t = T.T.m.q;
    if (j == 0) a.idx = T.d_idx;
};
// pairs a lane owns: at most 4 up to n = 4096; above that 8 -- at n = 8192 on 512 threads, so that two workgroups of 8 waves share a CU where one of 16 waves
// would need 64 VGPRs or fewer to let a second one in; at n = 16384 the workgroup stops at 1024 threads anyway
int k_slots_crt_decompose(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *d_plain, size_t count, int slots, long long *d_values, size_t item_stride,
                          size_t slot_stride, hipStream_t st)
{
    SlotCrtArgs a{};
    slots_crt_args(B, a);
    for (int j = 0; j < B.r; j++) a.m[j].plain_in = d_plain[j];
    a.vals_out = d_values; a.count = count; a.slots = slots; a.item_stride = item_stride; a.slot_stride = slot_stride;
    if (ctxs[0]->n <= 4096) return slots_launch(ctxs, B.r, slots_crt_decompose_kernel<true, 4>, slots_crt_decompose_kernel<false, 4>, a, slots_crt_tables, st);
    return slots_launch(ctxs, B.r, slots_crt_decompose_kernel<true, 8>, slots_crt_decompose_kernel<false, 8>, a, slots_crt_tables, st, ctxs[0]->n / 16);
}
int k_slots_crt_act(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *d_in, size_t count, u64 divisor, int relu, u64 cap, u64 *const *d_out, hipStream_t st)
{
    SlotCrtArgs a{};
    slots_crt_args(B, a);
    for (int j = 0; j < B.r; j++) { a.m[j].plain_in = d_in[j]; a.m[j].plain_out = d_out[j]; }
    a.count = count; a.D = divisor; a.recip = divisor == 1 ? ~(u64)0 : (u64)(((unsigned __int128)1 << 64) / divisor);
    a.relu = relu; a.cap = cap;
    if (ctxs[0]->n <= 4096) return slots_launch(ctxs, B.r, slots_crt_act_kernel<true, 4>, slots_crt_act_kernel<false, 4>, a, slots_crt_tables, st);
    return slots_launch(ctxs, B.r, slots_crt_act_kernel<true, 8>, slots_crt_act_kernel<false, 8>, a, slots_crt_tables, st, ctxs[0]->n / 16);
}

// host twins: the reference transforms per modulus, the same Garner steps in 128-bit arithmetic
static void slots_crt_lift_host(const SlotsCrtBase &B, const SlotTables *const *T, const u64 *const *plain, size_t m, int n, std::vector<u64> &row, std::vector<u64> &x)
{
    for (int j = 0; j < B.r; j++) {
        const u64 t = B.t[j];
        for (int i = 0; i < n; i++) row[i] = plain[j][m * (size_t)n + i] % t;
        h_ntt_fwd(T[j]->T, row.data(), n);
        for (int i = 0; i < n; i++) {
            if (!j) { x[i] = row[i]; continue; }
            const u64 xr = x[i] % t, d = row[i] >= xr ? row[i] - xr : row[i] + t - xr;
            x[i] += B.P[j] * (u64)((unsigned __int128)d * B.Pinv[j] % t);
        }
    }
}
int k_slots_crt_decompose_host(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *plain, size_t count, int slots, long long *values, size_t item_stride,
                               size_t slot_stride)
{
    const SlotTables *T[CRC_SLOTS_CRT_MAX];
    for (int j = 0; j < B.r; j++) { const int rc = crc_slots_tables(ctxs[j], &T[j]); if (rc) return rc; }
    const int n = ctxs[0]->n; const u64 half = (B.T - 1) >> 1;
    crc_host::parallel_for(count, 4, [&](size_t b, size_t e) {
        std::vector<u64> row((size_t)n), x((size_t)n);
        for (size_t m = b; m < e; m++) {
            slots_crt_lift_host(B, T, plain, m, n, row, x);
            for (int i = 0; i < slots; i++) { const u64 v = x[T[0]->idx[i]]; values[m * item_stride + (size_t)i * slot_stride] = (long long)(v > half ? v - B.T : v); }
        }
    });
    return CRC_OK;
}
int k_slots_crt_act_host(crc_ctx *const *ctxs, const SlotsCrtBase &B, const u64 *const *plain_in, size_t count, u64 divisor, int relu, u64 cap, u64 *const *plain_out)
{
    const SlotTables *T[CRC_SLOTS_CRT_MAX];
    for (int j = 0; j < B.r; j++) { const int rc = crc_slots_tables(ctxs[j], &T[j]); if (rc) return rc; }
    const int n = ctxs[0]->n; const u64 half = (B.T - 1) >> 1;
    const __int128 D = (__int128)divisor, h = (__int128)(divisor >> 1);
    crc_host::parallel_for(count, 4, [&](size_t b, size_t e) {
        std::vector<u64> row((size_t)n), x((size_t)n);
        std::vector<__int128> rho((size_t)n);
        for (size_t m = b; m < e; m++) {
            slots_crt_lift_host(B, T, plain_in, m, n, row, x);          // all r input rows are read before an output row is written
            for (int i = 0; i < n; i++) {
                const __int128 num = (x[i] > half ? (__int128)x[i] - (__int128)B.T : (__int128)x[i]) + h;
                __int128 q = num / D; if (num % D < 0) q--;                    // floor division
                if (relu && q < 0) q = 0;
                if (cap && q > (__int128)cap) q = (__int128)cap;
                rho[i] = q;
            }
            for (int j = 0; j < B.r; j++) {
                const __int128 t = (__int128)B.t[j];
                for (int i = 0; i < n; i++) { __int128 v = rho[i] % t; if (v < 0) v += t; row[i] = (u64)v; }
                h_ntt_inv(T[j]->T, row.data(), n);
                for (int i = 0; i < n; i++) plain_out[j][m * (size_t)n + i] = row[i];
            }
        }
    });
    return CRC_OK;
}
