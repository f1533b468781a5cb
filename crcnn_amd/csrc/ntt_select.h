// ntt_select.h -- which kernel a 64-bit row transform takes: THE map (ring, modulus class, request) -> (kernel family, template arguments, launch geometry).
// Pure (no side effects, no allocation, no HIP types): tests/cpp/ntt_select_check.cpp walks it with plain g++; ntt_launch (kernels.hip) turns the choice into a
// function pointer and launches it.  DESIGN.md 4.3 has the same map as a table.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include "xcd_grid.h"
#include "../../include/crcnn_hip.h"

// NttArgs::prologue: what a row's load does on the way in (SQUARE, SCALED and PRODUCT belong to the inverse transform, DIGIT to the forward one)
enum NttPrologue { NTT_PRO_NONE = 0, NTT_PRO_LIFT = 1, NTT_PRO_DELTA = 2, NTT_PRO_DIGIT = 3, NTT_PRO_SQUARE = 4, NTT_PRO_SCALED = 5, NTT_PRO_PRODUCT = 6 };
// the product fused into a forward transform: + fma_u . fma_k (public-key encryptor), x the plaintext row fma_k (multiply_plain), - c1 . fma_k (fma_neg)
enum NttFma { NTT_FMA_NONE = 0, NTT_FMA_ADD = 1, NTT_FMA_MUL = 2, NTT_FMA_NEG = 3 };
// bits of the tuning value ntt_wave: the rings that take ntt_rows_wave_kernel (16384 apart for plain transforms and for those with a prologue); HALVE: its
// inverse keeps the butterflies that halve per stage.  -1 stands for the measured default
enum { NTT_WAVE_8192 = 1, NTT_WAVE_4096 = 2, NTT_WAVE_16384 = 4, NTT_WAVE_16384_PRO = 8, NTT_WAVE_HALVE = 16, NTT_WAVE_2048 = 32,
       NTT_WAVE_DEFAULT = NTT_WAVE_8192 | NTT_WAVE_4096 | NTT_WAVE_16384 | NTT_WAVE_16384_PRO | NTT_WAVE_2048 };
enum NttFamily { NTT_FAM_ROWS, NTT_FAM_INV61, NTT_FAM_WAVE, NTT_FAM_SPLIT, NTT_FAM_PREFETCH };   // ntt_rows_kernel, ntt_rows_inv61_kernel, ntt_rows_wave_kernel, ...

struct NttRing {                // the ring, the tuning, the moduli of the launch: their count, the narrowest and the widest, every one below 2^55
    int n, logn, cus, ntt_wave, ntt_split, ntt_inv61_loose, mod_count, min_bits, max_bits; bool below55;
};
struct NttRequest {             // opt_mul: post_mul is offered to a kernel that ends in a multiplication anyway; pairs: of the product prologues
    bool inv; int prologue, fma; bool addend, pack_out, box, opt_mul; size_t rows, pairs;
    bool fma_u, in_place; int src_ct_rows, dst_ct_rows;         // what NTT_FMA_NEG asks of its rows
};
struct NttChoice {              // status CRC_OK without launch: nothing to do.  Each family reads its own template arguments
    int status; bool launch; int family; bool inv, lazy; int pro, cs; bool uns; int fma; bool box; size_t grid; int block; size_t lds;
    bool takes_post_mul;        // uns: n^-1 goes into post_mul -- times the caller's constant (true) or alone
};

// the one rule of prologue and direction; also which <INV, ., PRO> instances of ntt_rows_kernel / ntt_rows_split_kernel exist
constexpr bool ntt_prologue_dir_ok(bool inv, int pro) { return pro == NTT_PRO_DIGIT ? !inv : pro >= NTT_PRO_SQUARE ? inv : true; }
// which ntt_rows_wave_kernel<INV, PRO, ., UNS, FMA, BOX> exist: inverse NONE / SQUARE / SCALED / PRODUCT either way of scaling; forward plain, fused or boxed
constexpr bool ntt_wave_instance(bool inv, int pro, bool uns, int fma, bool box) { return inv ? !fma && !box : !pro && !uns && !(fma && box); }

static inline NttChoice ntt_select(const NttRing &g, const NttRequest &r)
{
    NttChoice k{}; const int pro = r.prologue;
    const auto refuse = [](int status) { NttChoice no{}; no.status = status; return no; };
    if (r.rows == 0) return k;
    k.lds = (size_t)g.n * 8;                                    // the row itself
    if (k.lds > 128 * 1024) return refuse(CRC_ERR_UNSUPPORTED);       // (n = 32768: the row does not fit one workgroup's LDS image, in halves or whole)
    if (!ntt_prologue_dir_ok(r.inv, pro)) return refuse(CRC_ERR_INVALID_ARGUMENT);
    k.launch = true; k.inv = r.inv;
    // lazy butterflies need (1 + 4 log2 n) q < 2^64 (and the float quotient estimate a q of 45+ bits): every coefficient modulus of the reference's parameter
    // sets qualifies (54..55 bits), the 61-bit auxiliary base of Square does not
    k.lazy = g.min_bits >= 45 && g.max_bits <= 57;
    k.grid = pro == NTT_PRO_SQUARE || pro == NTT_PRO_PRODUCT ? xcd_grid(r.pairs, 3) : r.rows;      // a pair's three products on one XCD (ntt_rows_body)
    // wave-local passes: the ring's bit of ntt_wave, lazy moduli, no addend, a prologue the kernel has.  (16384 with the Square prologues is slower than the split
    // kernel with the halving butterflies, 11.9 against 11.7 us per squared ciphertext, faster with the ones that do not halve: 11.27 against 11.6 --
    // profiles/r05_ntt_u64_wave_local_ab.txt, r05_ntt_inverse_unscaled_ab.txt)
    const int sel = g.ntt_wave < 0 ? NTT_WAVE_DEFAULT : g.ntt_wave;
    const int bit = g.n == 8192 ? NTT_WAVE_8192 : g.n == 4096 ? NTT_WAVE_4096 : g.n == 16384 ? (pro ? NTT_WAVE_16384_PRO : NTT_WAVE_16384)
                  : g.n == 2048 ? NTT_WAVE_2048 : 0;
    const bool wave = (sel & bit) && k.lazy && !r.addend && (pro == NTT_PRO_NONE || pro >= NTT_PRO_SQUARE);
    if (r.fma || r.box) {                                       // only the wave-local kernel has those: elsewhere the caller runs a pass of its own
        if (!wave) return refuse(CRC_ERR_UNSUPPORTED);
        if (r.inv || pro || r.pack_out || (r.fma && r.box)) return refuse(CRC_ERR_INVALID_ARGUMENT);
        if (r.fma == NTT_FMA_NEG && (r.fma_u || !r.in_place || r.dst_ct_rows != g.mod_count || r.src_ct_rows != 2 * g.mod_count))
            return refuse(CRC_ERR_INVALID_ARGUMENT);
    }
    if (wave) {
        k.family = NTT_FAM_WAVE; k.pro = pro; k.cs = g.logn - 10; k.fma = r.fma; k.box = r.box; k.block = g.n / 16;
        // inverse transforms over moduli below 2^55 take the butterflies that do not halve (inv_stages_unscaled): the table of plain inverse powers, and n^-1
        // in the constant of the closing multiplication
        k.uns = r.inv && !(sel & NTT_WAVE_HALVE) && g.below55; k.takes_post_mul = k.uns && (pro == NTT_PRO_SCALED || r.opt_mul);
        return k;
    }
    k.block = g.n / 8 < 64 ? 64 : g.n / 8 > 1024 ? 1024 : g.n / 8;
    k.pro = pro < NTT_PRO_DIGIT ? NTT_PRO_NONE : pro;           // (the plain lift and the delta scale are run-time branches of the NONE instances)
    if (g.n == 16384 && g.ntt_split) { k.family = NTT_FAM_SPLIT; k.lds /= 2; }   // the row as two halves through a 64-KiB image: two workgroups per CU
    else if (g.n == 16384 && r.rows > (size_t)g.cus && pro < NTT_PRO_DIGIT) { k.family = NTT_FAM_PREFETCH; k.grid = (size_t)g.cus; }   // a resident workgroup per CU
    // (a strict inverse is the 61-bit auxiliary base's: held to 64 registers unless the tuning says not to)
    else k.family = !k.lazy && r.inv && pro != NTT_PRO_SCALED && !g.ntt_inv61_loose ? NTT_FAM_INV61 : NTT_FAM_ROWS;
    return k;
}

// the instantiation's name as a kernel trace prints it (profiles/ntt_paths_kernels.md); returns snprintf's count
static inline int ntt_choice_name(const NttChoice &k, char *buf, size_t len)
{
    static const char *const tf[2] = {"false", "true"};
    if (k.family == NTT_FAM_WAVE) return snprintf(buf, len, "ntt_rows_wave_kernel<%s, %d, %d, %s, %d%s>", tf[k.inv], k.pro, k.cs, tf[k.uns], k.fma, k.box ? ", true" : "");
    if (k.family == NTT_FAM_INV61) return snprintf(buf, len, "ntt_rows_inv61_kernel<%d>", k.pro);
    if (k.family == NTT_FAM_PREFETCH) return snprintf(buf, len, "ntt_rows_prefetch_kernel<%s, %s>", tf[k.inv], tf[k.lazy]);
    return snprintf(buf, len, "ntt_rows_%skernel<%s, %s, %d>", k.family == NTT_FAM_SPLIT ? "split_" : "", tf[k.inv], tf[k.lazy], k.pro);
}
