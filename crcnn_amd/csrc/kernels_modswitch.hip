// kernels_modswitch.hip -- modulus switching for whole ciphertext tensors on gfx950, and its host twin.
//
// A ciphertext [size][k][n] over q_0 .. q_{k-1} becomes one over the first k' moduli: every coefficient c in [0, q) goes to floor((c + h) / p), p the last
// modulus and h = p >> 1, once per dropped modulus, last to first (modswitch_device.h has the residue form).  Four form pairs, all from this file's kernels:
//   COEFF -> COEFF   modswitch_coeff_kernel: elementwise, k rows read once, k' written
//   NTT   -> NTT     modswitch_inverse_kernel on the D dropped rows (into work space), then modswitch_rows_kernel: a workgroup per kept row transforms R mod q_i and
//                    corrects the kept NTT row in its drain loop -- D inverse + k' forward transforms per polynomial, the kept rows never leave NTT form
//   COEFF -> NTT     modswitch_rows_kernel with the switched row itself as the image (k' forward transforms, no work space)
//   NTT   -> COEFF   modswitch_inverse_kernel on all k rows, then modswitch_coeff_kernel on the work space (k inverse transforms)
// The per-modulus tables of the prefix context are those of the full one (same primes, same minimal roots), so only `from`'s tables are read.
#include <cstring>
#include "kernels.h"
#include "host_parallel.h"
#include "work_arena.h"
#include "modswitch_device.h"

typedef unsigned __int128 u128;

template <int D>
__global__ void __launch_bounds__(256) modswitch_coeff_kernel(ModSwitchArgs a) { modswitch_coeff_body<D>(a); }
template <bool LAZY>
__global__ void __launch_bounds__(1024) modswitch_inverse_kernel(ModSwitchArgs a)
{
    extern __shared__ u64 sm[];
    modswitch_inverse_body<LAZY>(a, sm);
}
template <int D, bool LAZY>
__global__ void __launch_bounds__(1024) modswitch_rows_kernel(ModSwitchArgs a)
{
    extern __shared__ u64 sm[];
    modswitch_rows_body<D, LAZY>(a, sm);
}

// `to` is a proper prefix of `from`: fewer moduli, the same ones in the same order, the same ring and plain modulus
bool k_mod_switch_supported(const crc_ctx *from, const crc_ctx *to)
{
    if (!from || !to || to->k < 1 || to->k >= from->k || from->k > CRC_MAXK || to->n != from->n || to->t != from->t) return false;
    for (int i = 0; i < to->k; i++) if (to->q[i] != from->q[i]) return false;
    for (int i = 0; i < from->k; i++) if (from->q[i] >> 62) return false;          // the kernels add three residues in one word
    return true;
}

static u64 shoup_of(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
void k_mod_switch_consts(const crc_ctx *from, int kept, ModSwitchConsts &c)
{
    memset(&c, 0, sizeof c);
    const int k = from->k, D = k - kept;
    c.k = k; c.kept = kept;
    for (int i = 0; i < k; i++) { c.q[i] = from->q[i]; c.one_s[i] = shoup_of(1, from->q[i]); }
    for (int j = 0; j < D; j++) {
        const u64 p = from->q[k - 1 - j];
        c.h[j] = p >> 1;
        for (int i = 0; i < k - 1 - j; i++) {
            const u64 q = from->q[i];
            c.hmod[j][i] = c.h[j] % q;
            c.pinv[j][i] = h_invmod(p % q, q); c.pinv_s[j][i] = shoup_of(c.pinv[j][i], q);
            u64 prod = 1;
            for (int l = 0; l < j; l++) prod = h_mulmod(prod, from->q[k - 1 - l] % q, q);
            c.pmod[j][i] = prod; c.pmod_s[j][i] = shoup_of(prod, q);
        }
    }
    for (int i = 0; i < kept; i++) {
        const u64 q = from->q[i];
        u64 prod = 1;
        for (int j = 0; j < D; j++) prod = h_mulmod(prod, from->q[k - 1 - j] % q, q);
        c.Pinv[i] = h_invmod(prod, q); c.Pinv_s[i] = shoup_of(c.Pinv[i], q);
    }
}

// The work space of one call, by form pair: the coefficient form of the rows the inverse pass makes (none for a coefficient-form input)
struct ModSwitchLayout {
    u64 *rows;
    int row0, nrows;
    ModSwitchLayout(WorkArena &w, const crc_ctx *from, const crc_ctx *to, size_t polys, int in_form, int out_form)
    {
        row0 = out_form == CRC_NTT ? to->k : 0;
        nrows = in_form == CRC_NTT ? from->k - row0 : 0;
        rows = w.take<u64>(polys * (size_t)nrows * from->n);
    }
};
size_t k_mod_switch_work_bytes(const crc_ctx *from, const crc_ctx *to, size_t polys, int in_form, int out_form)
{
    WorkArena w; ModSwitchLayout L(w, from, to, polys, in_form, out_form); (void)L;
    return w.bytes();
}

template <int D>
static int launch_d(crc_ctx *c, bool rows, bool lazy, const ModSwitchArgs &a, int nt, size_t lds, hipStream_t st)
{
    if (!rows) {
        const size_t pairs = a.polys * (size_t)(a.n / 2);
        hipLaunchKernelGGL(modswitch_coeff_kernel<D>, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, a);
    } else {
        auto kern = lazy ? modswitch_rows_kernel<D, true> : modswitch_rows_kernel<D, false>;
        { const int rc = crc_ctx_ensure_lds(c, (const void *)kern, lds); if (rc) return rc; }
        hipLaunchKernelGGL(kern, dim3(xcd_grid(a.polys, (unsigned)a.c.kept)), dim3(nt), lds, st, a);
    }
    HIPCHK(hipGetLastError());
    return CRC_OK;
}
static int launch(crc_ctx *c, int D, bool rows, bool lazy, const ModSwitchArgs &a, int nt, size_t lds, hipStream_t st)
{
    switch (D) {
    case 1: return launch_d<1>(c, rows, lazy, a, nt, lds, st);
    case 2: return launch_d<2>(c, rows, lazy, a, nt, lds, st);
    case 3: return launch_d<3>(c, rows, lazy, a, nt, lds, st);
    case 4: return launch_d<4>(c, rows, lazy, a, nt, lds, st);
    case 5: return launch_d<5>(c, rows, lazy, a, nt, lds, st);
    case 6: return launch_d<6>(c, rows, lazy, a, nt, lds, st);
    case 7: return launch_d<7>(c, rows, lazy, a, nt, lds, st);
    }
    return CRC_ERR_INVALID_ARGUMENT;
}

// d_in [polys][k][n] in in_form -> d_out [polys][k'][n] in out_form; the caller has checked the contexts, the forms, the pointers and their alignment
int k_mod_switch(crc_ctx *from, const crc_ctx *to, const u64 *d_in, int in_form, size_t polys, u64 *d_out, int out_form, void *d_work, hipStream_t st)
{
    if (polys == 0) return CRC_OK;
    const int n = from->n, k = from->k, kept = to->k, D = k - kept;
    const size_t lds = (size_t)n * 8;
    const bool transforms = in_form == CRC_NTT || out_form == CRC_NTT;
    if (transforms && lds > 128 * 1024) return CRC_ERR_UNSUPPORTED;                 // (n = 32768: a row does not fit the LDS; the host twin serves it)
    if (polys > 0x7fffffffULL / ((size_t)k * 8) || polys * (size_t)(n / 2) / 256 > 0x7fffffffULL) return CRC_ERR_INVALID_ARGUMENT;
    WorkArena w(d_work);
    const ModSwitchLayout L(w, from, to, polys, in_form, out_form);
    bool lazy = true;
    for (int i = 0; i < k; i++) lazy = lazy && from->tabs[i].m.bits <= 57;
    int nt = n / 8; if (nt < 64) nt = 64; if (nt > 1024) nt = 1024;
    ModSwitchArgs a{};
    k_mod_switch_consts(from, kept, a.c);
    a.polys = polys; a.n = n; a.logn = from->logn;
    const size_t ps = (size_t)k * n;
    if (in_form == CRC_NTT) {                                                       // the rows that are needed in coefficient form, into work space
        ModSwitchArgs v = a;
        v.kept_in = d_in; v.kept_ps = ps; v.out = L.rows; v.row0 = L.row0; v.rows = L.nrows; v.W = (const ulonglong2 *)from->d_irp2;
        auto kern = lazy ? modswitch_inverse_kernel<true> : modswitch_inverse_kernel<false>;
        { const int rc = crc_ctx_ensure_lds(from, (const void *)kern, lds); if (rc) return rc; }
        hipLaunchKernelGGL(kern, dim3((unsigned)(polys * (size_t)L.nrows)), dim3(nt), lds, st, v);
        HIPCHK(hipGetLastError());
    }
    a.out = d_out; a.W = (const ulonglong2 *)from->d_rp;
    if (in_form == CRC_COEFF) { a.kept_in = d_in; a.kept_ps = ps; a.drop_in = d_in + (size_t)kept * n; a.drop_ps = ps; a.kept_ntt = 0; }
    else if (out_form == CRC_NTT) { a.kept_in = d_in; a.kept_ps = ps; a.drop_in = L.rows; a.drop_ps = (size_t)D * n; a.kept_ntt = 1; }
    else { a.kept_in = L.rows; a.kept_ps = ps; a.drop_in = L.rows + (size_t)kept * n; a.drop_ps = ps; a.kept_ntt = 0; }
    return launch(from, D, out_form == CRC_NTT, lazy, a, nt, lds, st);
}

// ---- host twin (any context, device = -1 included): the drops one after another in 128-bit integer arithmetic, the reference transforms of ctx.cpp around them ---
int k_mod_switch_host(const crc_ctx *from, const crc_ctx *to, const u64 *in, int in_form, size_t polys, u64 *out, int out_form)
{
    const int n = from->n, k = from->k, kept = to->k;
    crc_host::parallel_for(polys, 1, [&](size_t b, size_t e) {
        std::vector<u64> r((size_t)k * n);
        for (size_t p = b; p < e; p++) {
            memcpy(r.data(), in + p * (size_t)k * n, (size_t)k * n * 8);
            if (in_form == CRC_NTT) for (int i = 0; i < k; i++) h_ntt_inv(from->tabs[i], r.data() + (size_t)i * n, n);
            for (int top = k - 1; top >= kept; top--) {
                const u64 pm = from->q[top], h = pm >> 1;
                for (int i = 0; i < top; i++) {
                    const u64 q = from->q[i], pinv = h_invmod(pm % q, q);
                    u64 *row = r.data() + (size_t)i * n; const u64 *last = r.data() + (size_t)top * n;
                    for (int s = 0; s < n; s++) {
                        const u64 u = (u64)(((u128)last[s] + h) % pm);                  // the centred remainder is u - h
                        const u64 x = (u64)(((u128)row[s] + (q - u % q) + h % q) % q);
                        row[s] = (u64)((u128)x * pinv % q);
                    }
                }
            }
            if (out_form == CRC_NTT) for (int i = 0; i < kept; i++) h_ntt_fwd(to->tabs[i], r.data() + (size_t)i * n, n);
            memcpy(out + p * (size_t)kept * n, r.data(), (size_t)kept * n * 8);
        }
    });
    return CRC_OK;
}
