// ntt_select_check.cpp -- the map (ring, modulus class, request) -> row-transform kernel of crcnn_amd/csrc/ntt_select.h, checked on the CPU against expectations
// WRITTEN OUT here: the rows of the DESIGN.md table "Which kernel a transform takes" as data (TABLE below; exactly one row must claim every valid case), the
// tuning switches and the refusals case by case.  Nothing here asks the selector what to expect.  The paths behind ntt_split = 0 (the prefetch kernel, the
// one-image kernel at n = 16384) and ntt_inv61_loose have no GPU test: this program is their only check.
//   g++ -std=c++17 -fsanitize=address,undefined -I crcnn_amd/csrc tests/cpp/ntt_select_check.cpp && ./a.out   -> "ok cases <N> tuning <N> refusals <N> names <N>"
#include "ntt_select.h"
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

static int failures = 0;
#define FAIL(...) do { if (++failures <= 20) { printf("FAILED " __VA_ARGS__); printf("\n"); } } while (0)

// ---- the classes of tests/test_gpu_ntt_paths.py: [p, 0x3fffffff000001], and the 61-bit auxiliary base (three primes just below 2^61) ----------------------
static int bit_length(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
struct Class { const char *name; std::vector<uint64_t> q; };
static const uint64_t Q54 = 0x3fffffff000001ull;
static const std::vector<Class> CLASSES = {
    {"w44", {0xfffffdf8001ull, Q54}}, {"w45", {0x100000020001ull, Q54}}, {"w52", {0xffffffff58001ull, Q54}}, {"w53", {0x1ffffffff38001ull, Q54}},
    {"w55", {0x7fffffffe90001ull, Q54}}, {"w56", {0x80000000068001ull, Q54}}, {"w57", {0x1fffffffffc0001ull, Q54}}, {"w58", {0x200000000208001ull, Q54}},
    {"w60", {0xffffffffffe8001ull, Q54}}, {"aux61", {0x1fffffffffe00001ull, 0x1fffffffffc80001ull, 0x1fffffffffb40001ull}}};
static const int WIDTHS[] = {44, 45, 52, 53, 55, 56, 57, 58, 60, 61};
static const int CUS = 256;

static NttRing ring_of(int n, const Class &c, int wave = -1, int split = 1, int loose = 0)
{
    NttRing g{};
    g.n = n; g.logn = bit_length((uint64_t)n) - 1; g.cus = CUS; g.ntt_wave = wave; g.ntt_split = split; g.ntt_inv61_loose = loose;
    g.mod_count = (int)c.q.size(); g.min_bits = 64; g.max_bits = 0; g.below55 = true;
    for (uint64_t q : c.q) {
        const int b = bit_length(q);
        if (b < g.min_bits) g.min_bits = b;
        if (b > g.max_bits) g.max_bits = b;
        if (q >> 55) g.below55 = false;
    }
    return g;
}
// a request whose NTT_FMA_NEG shape is the valid one (in place, c0 rows of size-2 ciphertexts)
static NttRequest request_of(const NttRing &g, bool inv, int pro, bool addend, int fma, bool box, bool opt_mul, size_t rows, size_t pairs)
{
    NttRequest r{};
    r.inv = inv; r.prologue = pro; r.fma = fma; r.addend = addend; r.box = box; r.opt_mul = opt_mul; r.rows = rows; r.pairs = pairs;
    r.fma_u = fma == NTT_FMA_ADD; r.in_place = true; r.src_ct_rows = 2 * g.mod_count; r.dst_ct_rows = g.mod_count;
    return r;
}

// ---- default tuning: the DESIGN.md table, row by row ---------------------------------------------------------------------------------------------------------
enum Cls { LAZY, STRICT, UNS, LAZY_WIDE };            // LAZY: every modulus 45..57 bits; UNS: LAZY and every modulus below 2^55; LAZY_WIDE: LAZY, not UNS
enum Dir { FWD = 1, INV = 2, BOTH = 3 };
enum Add { NO_ADDEND = 1, ADDEND = 2, ANY_ADDEND = 3 };
#define P(x) (1 << (x))
struct Row {
    int ring_lo, ring_hi, cls, dir; unsigned pros; int addend;
    bool fused;                                       // the row (and no other) admits a fused product or a box
    int family; bool lazy, uns;
};
static const unsigned PLAIN = P(0) | P(1) | P(2), ALL = 0x7f;
static const Row TABLE[] = {
    // 64 .. 1024 | lazy | 0, 3, 4, 5, 6; any addend | ntt_rows_kernel<., true, PRO>
    {64, 1024, LAZY, BOTH, ALL, ANY_ADDEND, false, NTT_FAM_ROWS, true, false},
    // 64 .. 8192 | strict | forward 0, 3; inverse 5 | ntt_rows_kernel<., false, PRO>
    {64, 8192, STRICT, FWD, PLAIN | P(3), ANY_ADDEND, false, NTT_FAM_ROWS, false, false},
    {64, 8192, STRICT, INV, P(5), ANY_ADDEND, false, NTT_FAM_ROWS, false, false},
    // 64 .. 8192 | strict | inverse 0, 4, 6 | ntt_rows_inv61_kernel<PRO>
    {64, 8192, STRICT, INV, PLAIN | P(4) | P(6), ANY_ADDEND, false, NTT_FAM_INV61, false, false},
    // 2048 .. 16384 | lazy | forward 0 without addend; fused product FMA 1, 2, 3; a window sum (box) | ntt_rows_wave_kernel<false, 0, CS, false, FMA(, true)>
    {2048, 16384, LAZY, FWD, P(0), NO_ADDEND, true, NTT_FAM_WAVE, true, false},
    // 2048 .. 16384 | uns | inverse 0, 4, 5, 6 without addend | ntt_rows_wave_kernel<true, PRO, CS, true>
    {2048, 16384, UNS, INV, P(0) | P(4) | P(5) | P(6), NO_ADDEND, false, NTT_FAM_WAVE, true, true},
    // 2048 .. 16384 | lazy, a modulus of 56 or 57 bits | the same | ntt_rows_wave_kernel<true, PRO, CS, false>
    {2048, 16384, LAZY_WIDE, INV, P(0) | P(4) | P(5) | P(6), NO_ADDEND, false, NTT_FAM_WAVE, true, false},
    // 2048 .. 8192 | lazy | forward 1, 2 (plain lift, delta scale), forward 3, forward / inverse with an addend | ntt_rows_kernel<., true, PRO>
    {2048, 8192, LAZY, FWD, P(1) | P(2) | P(3), NO_ADDEND, false, NTT_FAM_ROWS, true, false},
    {2048, 8192, LAZY, INV, P(1) | P(2), NO_ADDEND, false, NTT_FAM_ROWS, true, false},
    {2048, 8192, LAZY, BOTH, ALL, ADDEND, false, NTT_FAM_ROWS, true, false},
    // 16384 | lazy | the same | ntt_rows_split_kernel<., true, PRO>
    {16384, 16384, LAZY, FWD, P(1) | P(2) | P(3), NO_ADDEND, false, NTT_FAM_SPLIT, true, false},
    {16384, 16384, LAZY, INV, P(1) | P(2), NO_ADDEND, false, NTT_FAM_SPLIT, true, false},
    {16384, 16384, LAZY, BOTH, ALL, ADDEND, false, NTT_FAM_SPLIT, true, false},
    // 16384 | strict | everything | ntt_rows_split_kernel<., false, PRO>
    {16384, 16384, STRICT, BOTH, ALL, ANY_ADDEND, false, NTT_FAM_SPLIT, false, false},
};
static bool class_is(int width, int cls)              // `width` beside a 54-bit modulus (61: the auxiliary base on its own)
{
    const bool lazy = width >= 45 && width <= 57, uns = lazy && width <= 55;
    return cls == LAZY ? lazy : cls == STRICT ? !lazy : cls == UNS ? uns : lazy && !uns;
}
// inverse with the digit prologue, forward with the square / scaled / product prologues: CRC_ERR_INVALID_ARGUMENT
static bool direction_ok(bool inv, int pro) { return inv ? pro != 3 : pro < 4; }
static const Row *row_of(int n, int width, bool inv, int pro, bool addend, int *matches)
{
    const Row *hit = nullptr; *matches = 0;
    for (const Row &t : TABLE)
        if (n >= t.ring_lo && n <= t.ring_hi && class_is(width, t.cls) && (t.dir & (inv ? INV : FWD)) && (t.pros & P(pro)) && (t.addend & (addend ? ADDEND : NO_ADDEND))) {
            hit = &t; (*matches)++;
        }
    return hit;
}
static std::set<std::string> names;
static std::string name_of(const NttChoice &k) { char b[96]; ntt_choice_name(k, b, sizeof b); return b; }

static long walk_default()
{
    long cases = 0;
    const size_t rows = 1000, pairs = 333;
    for (int n = 64; n <= 32768; n *= 2) for (size_t ci = 0; ci < CLASSES.size(); ci++) for (int inv = 0; inv < 2; inv++) for (int pro = 0; pro <= 6; pro++)
    for (int addend = 0; addend < 2; addend++) for (int fma = 0; fma <= 3; fma++) for (int box = 0; box < 2; box++) for (int opt = 0; opt < 2; opt++) {
        cases++;
        const int width = WIDTHS[ci];
        const NttRing g = ring_of(n, CLASSES[ci]);
        const NttChoice k = ntt_select(g, request_of(g, inv, pro, addend, fma, box, opt, rows, pairs));
        char what[160]; snprintf(what, sizeof what, "n=%d %s inv=%d pro=%d addend=%d fma=%d box=%d opt=%d", n, CLASSES[ci].name, inv, pro, addend, fma, box, opt);
        // the refusals, in the parent's order: the ring, the direction, then a fused product or a box off the wave-local kernel
        int want = CRC_OK, matches = 0;
        const Row *t = nullptr;
        if (n > 16384) want = CRC_ERR_UNSUPPORTED;
        else if (!direction_ok(inv, pro)) want = CRC_ERR_INVALID_ARGUMENT;
        else {
            t = row_of(n, width, inv, pro, addend, &matches);
            if (matches != 1) { FAIL("%s: %d table rows", what, matches); continue; }
            if (fma || box) want = t->family != NTT_FAM_WAVE ? CRC_ERR_UNSUPPORTED : (!t->fused || (fma && box)) ? CRC_ERR_INVALID_ARGUMENT : CRC_OK;
        }
        if (k.status != want) { FAIL("%s: status %d, want %d", what, k.status, want); continue; }
        if (want != CRC_OK) { if (k.launch) FAIL("%s: a refusal that launches", what); continue; }
        const bool wave = t->family == NTT_FAM_WAVE;
        const int wpro = wave || pro >= 3 ? pro : 0;                                  // (1 and 2 run on the PRO 0 instances)
        const size_t wgrid = pro == 4 || pro == 6 ? xcd_grid(pairs, 3) : rows;        // (xcd_grid.h, the launchers' own; X below is typed out)
        const int wblock = wave ? n / 16 : n / 8 < 64 ? 64 : n / 8 > 1024 ? 1024 : n / 8;
        const size_t wlds = t->family == NTT_FAM_SPLIT ? (size_t)n * 4 : (size_t)n * 8;
        if (!k.launch || k.family != t->family || k.inv != (bool)inv || k.pro != wpro) FAIL("%s: launch %d family %d inv %d pro %d", what, k.launch, k.family, k.inv, k.pro);
        if (k.family != NTT_FAM_INV61 && k.lazy != t->lazy) FAIL("%s: lazy %d", what, k.lazy);
        if (wave && (k.cs != g.logn - 10 || k.uns != t->uns || k.fma != fma || k.box != (bool)box)) FAIL("%s: cs %d uns %d fma %d box %d", what, k.cs, k.uns, k.fma, k.box);
        if (k.uns != (wave && t->uns) || k.takes_post_mul != (k.uns && (pro == 5 || opt))) FAIL("%s: uns %d takes_post_mul %d", what, k.uns, k.takes_post_mul);
        if (k.grid != wgrid || k.block != wblock || k.lds != wlds) FAIL("%s: grid %zu block %d lds %zu, want %zu %d %zu", what, k.grid, k.block, k.lds, wgrid, wblock, wlds);
        names.insert(name_of(k));
    }
    return cases;
}

// ---- the tuning switches and single cases: every expectation typed out -------------------------------------------------------------------------------------
struct Case {
    int n; const char *cls; bool inv; int pro; bool addend; int fma; bool box, opt_mul; size_t rows;
    int wave, split, loose;                           // the three tuning values
    int status; const char *name; size_t grid; int block; size_t lds; bool uns, takes_post_mul;
};
static const size_t R = 1000, X = 1008;               // rows of the launch; X = xcd_grid(333 pairs, 3)
#define OK(name, grid, block, lds, uns, takes) CRC_OK, name, grid, block, lds, uns, takes
#define UNSUP CRC_ERR_UNSUPPORTED, "", 0, 0, 0, false, false
static const int W = NTT_WAVE_DEFAULT;
static const Case CASES[] = {
    // ntt_wave: each ring's bit off in turn -- that ring (and no other) goes back to the kernels with a barrier per pass; a fused product or a box is refused
    {8192, "w55", false, 0, false, 0, false, false, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_kernel<false, true, 0>", R, 1024, 65536, false, false)},
    {8192, "w55", true, 0, false, 0, false, false, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_kernel<true, true, 0>", R, 1024, 65536, false, false)},
    {8192, "w55", true, 4, false, 0, false, true, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_kernel<true, true, 4>", X, 1024, 65536, false, false)},
    {8192, "w55", true, 5, false, 0, false, false, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_kernel<true, true, 5>", R, 1024, 65536, false, false)},
    {8192, "w55", true, 6, false, 0, false, true, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_kernel<true, true, 6>", X, 1024, 65536, false, false)},
    {8192, "w55", false, 0, false, 2, false, false, R, W & ~NTT_WAVE_8192, 1, 0, UNSUP},
    {8192, "w55", false, 0, false, 0, true, false, R, W & ~NTT_WAVE_8192, 1, 0, UNSUP},
    {4096, "w55", false, 0, false, 0, false, false, R, W & ~NTT_WAVE_8192, 1, 0, OK("ntt_rows_wave_kernel<false, 0, 2, false, 0>", R, 256, 32768, false, false)},
    {4096, "w55", false, 0, false, 0, false, false, R, W & ~NTT_WAVE_4096, 1, 0, OK("ntt_rows_kernel<false, true, 0>", R, 512, 32768, false, false)},
    {4096, "w55", true, 0, false, 0, false, false, R, W & ~NTT_WAVE_4096, 1, 0, OK("ntt_rows_kernel<true, true, 0>", R, 512, 32768, false, false)},
    {4096, "w55", true, 5, false, 0, false, false, R, W & ~NTT_WAVE_4096, 1, 0, OK("ntt_rows_kernel<true, true, 5>", R, 512, 32768, false, false)},
    {4096, "w55", false, 0, false, 1, false, false, R, W & ~NTT_WAVE_4096, 1, 0, UNSUP},
    {8192, "w55", true, 0, false, 0, false, false, R, W & ~NTT_WAVE_4096, 1, 0, OK("ntt_rows_wave_kernel<true, 0, 3, true, 0>", R, 512, 65536, true, false)},
    {2048, "w55", false, 0, false, 0, false, false, R, W & ~NTT_WAVE_2048, 1, 0, OK("ntt_rows_kernel<false, true, 0>", R, 256, 16384, false, false)},
    {2048, "w55", true, 4, false, 0, false, false, R, W & ~NTT_WAVE_2048, 1, 0, OK("ntt_rows_kernel<true, true, 4>", X, 256, 16384, false, false)},
    {2048, "w55", false, 0, false, 3, false, false, R, W & ~NTT_WAVE_2048, 1, 0, UNSUP},
    {2048, "w55", false, 0, false, 0, true, false, R, W & ~NTT_WAVE_2048, 1, 0, UNSUP},
    {4096, "w55", false, 0, false, 0, true, false, R, W & ~NTT_WAVE_2048, 1, 0, OK("ntt_rows_wave_kernel<false, 0, 2, false, 0, true>", R, 256, 32768, false, false)},
    // n = 16384 has two bits: plain transforms (fused product and box with them), and the transforms with a prologue
    {16384, "w55", false, 0, false, 0, false, false, R, W & ~NTT_WAVE_16384, 1, 0, OK("ntt_rows_split_kernel<false, true, 0>", R, 1024, 65536, false, false)},
    {16384, "w55", true, 0, false, 0, false, false, R, W & ~NTT_WAVE_16384, 1, 0, OK("ntt_rows_split_kernel<true, true, 0>", R, 1024, 65536, false, false)},
    {16384, "w55", false, 0, false, 1, false, false, R, W & ~NTT_WAVE_16384, 1, 0, UNSUP},
    {16384, "w55", false, 0, false, 0, true, false, R, W & ~NTT_WAVE_16384, 1, 0, UNSUP},
    {16384, "w55", true, 4, false, 0, false, true, R, W & ~NTT_WAVE_16384, 1, 0, OK("ntt_rows_wave_kernel<true, 4, 4, true, 0>", X, 1024, 131072, true, true)},
    {16384, "w55", true, 5, false, 0, false, false, R, W & ~NTT_WAVE_16384, 1, 0, OK("ntt_rows_wave_kernel<true, 5, 4, true, 0>", R, 1024, 131072, true, true)},
    {16384, "w55", true, 4, false, 0, false, true, R, W & ~NTT_WAVE_16384_PRO, 1, 0, OK("ntt_rows_split_kernel<true, true, 4>", X, 1024, 65536, false, false)},
    {16384, "w55", true, 5, false, 0, false, false, R, W & ~NTT_WAVE_16384_PRO, 1, 0, OK("ntt_rows_split_kernel<true, true, 5>", R, 1024, 65536, false, false)},
    {16384, "w55", true, 6, false, 0, false, false, R, W & ~NTT_WAVE_16384_PRO, 1, 0, OK("ntt_rows_split_kernel<true, true, 6>", X, 1024, 65536, false, false)},
    {16384, "w55", true, 0, false, 0, false, false, R, W & ~NTT_WAVE_16384_PRO, 1, 0, OK("ntt_rows_wave_kernel<true, 0, 4, true, 0>", R, 1024, 131072, true, false)},
    {16384, "w55", false, 0, false, 2, false, false, R, W & ~NTT_WAVE_16384_PRO, 1, 0, OK("ntt_rows_wave_kernel<false, 0, 4, false, 2>", R, 1024, 131072, false, false)},
    // NTT_WAVE_HALVE: the wave-local inverse keeps the halving butterflies -- UNS false, post_mul untouched even where it is offered or asked for
    {2048, "w55", true, 0, false, 0, false, false, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 0, 1, false, 0>", R, 128, 16384, false, false)},
    {4096, "w45", true, 0, false, 0, false, false, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 0, 2, false, 0>", R, 256, 32768, false, false)},
    {8192, "w55", true, 4, false, 0, false, true, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 4, 3, false, 0>", X, 512, 65536, false, false)},
    {8192, "w53", true, 5, false, 0, false, false, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 5, 3, false, 0>", R, 512, 65536, false, false)},
    {16384, "w55", true, 6, false, 0, false, true, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 6, 4, false, 0>", X, 1024, 131072, false, false)},
    {16384, "w52", true, 5, false, 0, false, false, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<true, 5, 4, false, 0>", R, 1024, 131072, false, false)},
    {8192, "w55", false, 0, false, 1, false, false, R, W | NTT_WAVE_HALVE, 1, 0, OK("ntt_rows_wave_kernel<false, 0, 3, false, 1>", R, 512, 65536, false, false)},
    //   ... against the default: the unscaled butterflies; post_mul taken in at SCALED, and at SQUARE / PRODUCT where the caller offers it
    {8192, "w55", true, 4, false, 0, false, true, R, -1, 1, 0, OK("ntt_rows_wave_kernel<true, 4, 3, true, 0>", X, 512, 65536, true, true)},
    {8192, "w55", true, 4, false, 0, false, false, R, -1, 1, 0, OK("ntt_rows_wave_kernel<true, 4, 3, true, 0>", X, 512, 65536, true, false)},
    {8192, "w53", true, 5, false, 0, false, false, R, -1, 1, 0, OK("ntt_rows_wave_kernel<true, 5, 3, true, 0>", R, 512, 65536, true, true)},
    {8192, "w56", true, 5, false, 0, false, false, R, -1, 1, 0, OK("ntt_rows_wave_kernel<true, 5, 3, false, 0>", R, 512, 65536, false, false)},
    // ntt_wave = 0: no ring has the wave-local kernel
    {2048, "w55", false, 0, false, 0, false, false, R, 0, 1, 0, OK("ntt_rows_kernel<false, true, 0>", R, 256, 16384, false, false)},
    {4096, "w55", true, 0, false, 0, false, false, R, 0, 1, 0, OK("ntt_rows_kernel<true, true, 0>", R, 512, 32768, false, false)},
    {8192, "w55", true, 6, false, 0, false, true, R, 0, 1, 0, OK("ntt_rows_kernel<true, true, 6>", X, 1024, 65536, false, false)},
    {16384, "w55", false, 0, false, 0, false, false, R, 0, 1, 0, OK("ntt_rows_split_kernel<false, true, 0>", R, 1024, 65536, false, false)},
    {16384, "w55", true, 5, false, 0, false, false, R, 0, 1, 0, OK("ntt_rows_split_kernel<true, true, 5>", R, 1024, 65536, false, false)},
    {2048, "w55", false, 0, false, 1, false, false, R, 0, 1, 0, UNSUP},
    {4096, "w55", false, 0, false, 2, false, false, R, 0, 1, 0, UNSUP},
    {8192, "w55", false, 0, false, 3, false, false, R, 0, 1, 0, UNSUP},
    {16384, "w55", false, 0, false, 2, false, false, R, 0, 1, 0, UNSUP},
    {8192, "w55", false, 0, false, 0, true, false, R, 0, 1, 0, UNSUP},
    {1024, "w55", false, 0, false, 0, false, false, R, 0, 1, 0, OK("ntt_rows_kernel<false, true, 0>", R, 128, 8192, false, false)},
    // ntt_split = 0 at n = 16384, more rows than CUs: the prefetch kernel for the prologues below DIGIT, one workgroup per CU, the whole 128-KiB image
    {16384, "w55", false, 0, false, 0, false, false, R, 0, 0, 0, OK("ntt_rows_prefetch_kernel<false, true>", CUS, 1024, 131072, false, false)},
    {16384, "w55", true, 0, false, 0, false, false, R, 0, 0, 0, OK("ntt_rows_prefetch_kernel<true, true>", CUS, 1024, 131072, false, false)},
    {16384, "w55", false, 1, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<false, true>", CUS, 1024, 131072, false, false)},
    {16384, "w55", false, 2, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<false, true>", CUS, 1024, 131072, false, false)},
    {16384, "w55", true, 0, true, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<true, true>", CUS, 1024, 131072, false, false)},
    {16384, "w55", false, 0, true, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<false, true>", CUS, 1024, 131072, false, false)},
    {16384, "w60", false, 0, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<false, false>", CUS, 1024, 131072, false, false)},
    {16384, "aux61", true, 0, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_prefetch_kernel<true, false>", CUS, 1024, 131072, false, false)},
    {16384, "aux61", true, 0, false, 0, false, false, R, -1, 0, 1, OK("ntt_rows_prefetch_kernel<true, false>", CUS, 1024, 131072, false, false)},
    {16384, "w55", false, 0, false, 0, false, false, CUS + 1, 0, 0, 0, OK("ntt_rows_prefetch_kernel<false, true>", CUS, 1024, 131072, false, false)},
    //   ... the prologues from DIGIT on never prefetch: the one-image ntt_rows_kernel, a workgroup per row
    {16384, "w55", false, 3, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_kernel<false, true, 3>", R, 1024, 131072, false, false)},
    {16384, "w60", false, 3, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_kernel<false, false, 3>", R, 1024, 131072, false, false)},
    {16384, "w55", true, 4, false, 0, false, true, R, 0, 0, 0, OK("ntt_rows_kernel<true, true, 4>", X, 1024, 131072, false, false)},
    {16384, "w55", true, 5, false, 0, false, false, R, 0, 0, 0, OK("ntt_rows_kernel<true, true, 5>", R, 1024, 131072, false, false)},
    {16384, "w55", true, 6, true, 0, false, false, R, -1, 0, 0, OK("ntt_rows_kernel<true, true, 6>", X, 1024, 131072, false, false)},
    {16384, "aux61", true, 4, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_inv61_kernel<4>", X, 1024, 131072, false, false)},
    {16384, "aux61", true, 5, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_kernel<true, false, 5>", R, 1024, 131072, false, false)},
    {16384, "aux61", true, 6, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_inv61_kernel<6>", X, 1024, 131072, false, false)},
    //   ... rows <= CUs: the one-image ntt_rows_kernel for every prologue
    {16384, "w55", false, 0, false, 0, false, false, CUS, 0, 0, 0, OK("ntt_rows_kernel<false, true, 0>", CUS, 1024, 131072, false, false)},
    {16384, "w55", true, 0, false, 0, false, false, CUS, 0, 0, 0, OK("ntt_rows_kernel<true, true, 0>", CUS, 1024, 131072, false, false)},
    {16384, "w55", false, 2, false, 0, false, false, 8, -1, 0, 0, OK("ntt_rows_kernel<false, true, 0>", 8, 1024, 131072, false, false)},
    {16384, "w55", true, 0, true, 0, false, false, 8, -1, 0, 0, OK("ntt_rows_kernel<true, true, 0>", 8, 1024, 131072, false, false)},
    {16384, "w44", false, 0, false, 0, false, false, 8, -1, 0, 0, OK("ntt_rows_kernel<false, false, 0>", 8, 1024, 131072, false, false)},
    {16384, "aux61", true, 0, false, 0, false, false, 8, -1, 0, 0, OK("ntt_rows_inv61_kernel<0>", 8, 1024, 131072, false, false)},
    {16384, "aux61", true, 0, false, 0, false, false, 8, -1, 0, 1, OK("ntt_rows_kernel<true, false, 0>", 8, 1024, 131072, false, false)},
    //   ... and the wave-local kernel, where its bit is on, comes first: ntt_split only decides among the others
    {16384, "w55", false, 0, false, 0, false, false, R, -1, 0, 0, OK("ntt_rows_wave_kernel<false, 0, 4, false, 0>", R, 1024, 131072, false, false)},
    {16384, "w55", false, 0, false, 1, false, false, R, 0, 0, 0, UNSUP},
    {8192, "w55", false, 0, false, 0, false, false, R, 0, 0, 0, OK("ntt_rows_kernel<false, true, 0>", R, 1024, 65536, false, false)},
    // ntt_inv61_loose = 1: the strict inverse with the prologues NONE (LIFT, DELTA), SQUARE, PRODUCT on ntt_rows_kernel<true, false, .>, nothing else moves
    {64, "aux61", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 0>", R, 64, 512, false, false)},
    {1024, "aux61", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 0>", R, 128, 8192, false, false)},
    {8192, "aux61", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 0>", R, 1024, 65536, false, false)},
    {8192, "aux61", true, 0, true, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 0>", R, 1024, 65536, false, false)},
    {8192, "aux61", true, 4, false, 0, false, true, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 4>", X, 1024, 65536, false, false)},
    {8192, "aux61", true, 6, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 6>", X, 1024, 65536, false, false)},
    {4096, "w44", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 0>", R, 512, 32768, false, false)},
    {2048, "w58", true, 4, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 4>", X, 256, 16384, false, false)},
    {2048, "w60", true, 6, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 6>", X, 256, 16384, false, false)},
    {8192, "aux61", true, 5, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, false, 5>", R, 1024, 65536, false, false)},
    {8192, "aux61", false, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<false, false, 0>", R, 1024, 65536, false, false)},
    {8192, "aux61", false, 3, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<false, false, 3>", R, 1024, 65536, false, false)},
    {8192, "w55", true, 0, true, 0, false, false, R, -1, 1, 1, OK("ntt_rows_kernel<true, true, 0>", R, 1024, 65536, false, false)},
    {8192, "w55", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_wave_kernel<true, 0, 3, true, 0>", R, 512, 65536, true, false)},
    {16384, "aux61", true, 0, false, 0, false, false, R, -1, 1, 1, OK("ntt_rows_split_kernel<true, false, 0>", R, 1024, 65536, false, false)},
    {8192, "aux61", true, 0, false, 0, false, false, R, -1, 1, 0, OK("ntt_rows_inv61_kernel<0>", R, 1024, 65536, false, false)},
};

static const Class &class_named(const char *name)
{
    for (const Class &c : CLASSES) if (!strcmp(c.name, name)) return c;
    printf("no class %s\n", name); exit(2);
}
static long walk_cases()
{
    long count = 0;
    for (const Case &w : CASES) {
        count++;
        const NttRing g = ring_of(w.n, class_named(w.cls), w.wave, w.split, w.loose);
        const NttChoice k = ntt_select(g, request_of(g, w.inv, w.pro, w.addend, w.fma, w.box, w.opt_mul, w.rows, 333));
        char what[200]; snprintf(what, sizeof what, "case %ld: n=%d %s inv=%d pro=%d addend=%d fma=%d box=%d rows=%zu wave=%d split=%d loose=%d", count, w.n, w.cls,
                                 w.inv, w.pro, w.addend, w.fma, w.box, w.rows, w.wave, w.split, w.loose);
        if (k.status != w.status || k.launch != (w.status == CRC_OK)) { FAIL("%s: status %d launch %d", what, k.status, k.launch); continue; }
        if (w.status != CRC_OK) continue;
        if (name_of(k) != w.name) FAIL("%s: %s, want %s", what, name_of(k).c_str(), w.name);
        if (k.grid != w.grid || k.block != w.block || k.lds != w.lds) FAIL("%s: grid %zu block %d lds %zu", what, k.grid, k.block, k.lds);
        if (k.uns != w.uns || k.takes_post_mul != w.takes_post_mul) FAIL("%s: uns %d takes_post_mul %d", what, k.uns, k.takes_post_mul);
    }
    return count;
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------------------------------
static long refusals = 0;
static void want_status(const char *what, const NttRing &g, const NttRequest &r, int status, bool launch)
{
    refusals++;
    const NttChoice k = ntt_select(g, r);
    if (k.status != status || k.launch != launch) FAIL("%s: status %d launch %d, want %d %d", what, k.status, k.launch, status, launch);
}
static void walk_refusals()
{
    const int INVALID = CRC_ERR_INVALID_ARGUMENT, UNSUPPORTED = CRC_ERR_UNSUPPORTED;
    for (const Class &c : CLASSES) for (int n = 64; n <= 16384; n *= 2) {
        const NttRing g = ring_of(n, c);
        // the direction comes before every other question: any ring, class, addend, fused product
        for (int addend = 0; addend < 2; addend++) for (int fma = 0; fma <= 3; fma++) {
            want_status("inverse DIGIT", g, request_of(g, true, NTT_PRO_DIGIT, addend, fma, false, false, R, 333), INVALID, false);
            for (int pro = NTT_PRO_SQUARE; pro <= NTT_PRO_PRODUCT; pro++) want_status("forward SQUARE / SCALED / PRODUCT", g, request_of(g, false, pro, addend, fma, false, false, R, 333), INVALID, false);
        }
        // no rows: CRC_OK, nothing launched, whatever else the request says
        want_status("rows == 0", g, request_of(g, false, 0, false, 0, false, false, 0, 0), CRC_OK, false);
        want_status("rows == 0", g, request_of(g, true, NTT_PRO_DIGIT, false, NTT_FMA_ADD, false, false, 0, 0), CRC_OK, false);
    }
    for (const Class &c : CLASSES) for (int wave : {-1, 0, 63}) for (int inv = 0; inv < 2; inv++) for (int pro = 0; pro <= 6; pro++) for (int fma = 0; fma <= 3; fma++) {
        const NttRing g = ring_of(32768, c, wave, wave ? 1 : 0, 0);     // n = 32768: unsupported before the direction is looked at, as ntt_launch always had it
        want_status("n = 32768", g, request_of(g, inv, pro, false, fma, false, false, R, 333), UNSUPPORTED, false);
    }
    const NttRing rings[] = {ring_of(2048, class_named("w55")), ring_of(4096, class_named("w45")), ring_of(8192, class_named("w57")), ring_of(16384, class_named("w53"))};
    for (const NttRing &g : rings) for (int fma = 1; fma <= 3; fma++) {
        // where the wave-local kernel is taken, a fused product wants the plain forward transform, unpacked
        want_status("fused product", g, request_of(g, false, 0, false, fma, false, false, R, 333), CRC_OK, true);
        want_status("fused product, inverse", g, request_of(g, true, 0, false, fma, false, false, R, 333), INVALID, false);
        for (int pro : {NTT_PRO_SQUARE, NTT_PRO_SCALED, NTT_PRO_PRODUCT}) want_status("fused product, inverse prologue", g, request_of(g, true, pro, false, fma, false, false, R, 333), INVALID, false);
        NttRequest r = request_of(g, false, 0, false, fma, false, false, R, 333);
        r.pack_out = true; want_status("fused product, pack_out", g, r, INVALID, false);
        want_status("fused product and box", g, request_of(g, false, 0, false, fma, true, false, R, 333), INVALID, false);
        // ... and where it is not -- a prologue it does not have, an addend -- the product is UNSUPPORTED, never INVALID
        for (int pro : {NTT_PRO_LIFT, NTT_PRO_DELTA, NTT_PRO_DIGIT}) want_status("fused product, forward prologue", g, request_of(g, false, pro, false, fma, false, false, R, 333), UNSUPPORTED, false);
        want_status("fused product, addend", g, request_of(g, false, 0, true, fma, false, false, R, 333), UNSUPPORTED, false);
        want_status("fused product, inverse with addend", g, request_of(g, true, 0, true, fma, false, false, R, 333), UNSUPPORTED, false);
    }
    for (const NttRing &g : rings) {
        // the four shape conditions of NTT_FMA_NEG, one at a time
        NttRequest r = request_of(g, false, 0, false, NTT_FMA_NEG, false, false, R, 333);
        want_status("fma_neg", g, r, CRC_OK, true);
        r.fma_u = true; want_status("fma_neg with fma_u", g, r, INVALID, false); r.fma_u = false;
        r.in_place = false; want_status("fma_neg out of place", g, r, INVALID, false); r.in_place = true;
        r.dst_ct_rows = 2 * g.mod_count; want_status("fma_neg dst_ct_rows", g, r, INVALID, false); r.dst_ct_rows = g.mod_count;
        r.src_ct_rows = g.mod_count; want_status("fma_neg src_ct_rows", g, r, INVALID, false); r.src_ct_rows = 0; want_status("fma_neg src_ct_rows 0", g, r, INVALID, false);
        // (the other products do not care)
        r = request_of(g, false, 0, false, NTT_FMA_MUL, false, false, R, 333); r.in_place = false; r.src_ct_rows = r.dst_ct_rows = 0; want_status("fma_mul any shape", g, r, CRC_OK, true);
        // a box: the plain forward transform on the wave-local kernel or nothing
        want_status("box", g, request_of(g, false, 0, false, 0, true, false, R, 333), CRC_OK, true);
        want_status("box, inverse", g, request_of(g, true, 0, false, 0, true, false, R, 333), INVALID, false);
        want_status("box, addend", g, request_of(g, false, 0, true, 0, true, false, R, 333), UNSUPPORTED, false);
    }
    // a fused product or a box off the wave-local kernel: rings without one, strict classes
    for (int n : {64, 128, 256, 512, 1024}) for (int fma = 0; fma <= 3; fma++) for (int box = 0; box < 2; box++) if (fma || box) {
        const NttRing g = ring_of(n, class_named("w55"));
        want_status("fused product / box, small ring", g, request_of(g, false, 0, false, fma, box, false, R, 333), UNSUPPORTED, false);
        want_status("fused product / box, small ring, inverse", g, request_of(g, true, 0, false, fma, box, false, R, 333), UNSUPPORTED, false);
    }
    for (int n : {2048, 4096, 8192, 16384}) for (const char *cls : {"w44", "w58", "w60", "aux61"}) for (int fma = 0; fma <= 3; fma++) for (int box = 0; box < 2; box++) if (fma || box) {
        const NttRing g = ring_of(n, class_named(cls));
        want_status("fused product / box, strict class", g, request_of(g, false, 0, false, fma, box, false, R, 333), UNSUPPORTED, false);
    }
}

// ---- the 60 instantiations profiles/ntt_paths_kernels.md recorded from tests/test_gpu_ntt_paths.py ----------------------------------------------------------
static const char *const RECORDED[] = {
    "ntt_rows_inv61_kernel<0>", "ntt_rows_inv61_kernel<4>", "ntt_rows_inv61_kernel<6>",
    "ntt_rows_kernel<false, false, 0>", "ntt_rows_kernel<false, false, 3>", "ntt_rows_kernel<false, true, 0>", "ntt_rows_kernel<false, true, 3>",
    "ntt_rows_kernel<true, false, 5>", "ntt_rows_kernel<true, true, 0>", "ntt_rows_kernel<true, true, 4>", "ntt_rows_kernel<true, true, 5>", "ntt_rows_kernel<true, true, 6>",
    "ntt_rows_split_kernel<false, false, 0>", "ntt_rows_split_kernel<false, false, 3>", "ntt_rows_split_kernel<false, true, 0>", "ntt_rows_split_kernel<false, true, 3>",
    "ntt_rows_split_kernel<true, false, 0>", "ntt_rows_split_kernel<true, false, 4>", "ntt_rows_split_kernel<true, false, 5>", "ntt_rows_split_kernel<true, false, 6>",
    "ntt_rows_split_kernel<true, true, 0>",
    "ntt_rows_wave_kernel<false, 0, 1, false, 0>", "ntt_rows_wave_kernel<false, 0, 1, false, 1>", "ntt_rows_wave_kernel<false, 0, 1, false, 2>", "ntt_rows_wave_kernel<false, 0, 1, false, 3>",
    "ntt_rows_wave_kernel<false, 0, 2, false, 0>",
    "ntt_rows_wave_kernel<false, 0, 3, false, 0>", "ntt_rows_wave_kernel<false, 0, 3, false, 1>", "ntt_rows_wave_kernel<false, 0, 3, false, 2>", "ntt_rows_wave_kernel<false, 0, 3, false, 3>",
    "ntt_rows_wave_kernel<false, 0, 4, false, 0>", "ntt_rows_wave_kernel<false, 0, 4, false, 1>", "ntt_rows_wave_kernel<false, 0, 4, false, 2>", "ntt_rows_wave_kernel<false, 0, 4, false, 3>",
    "ntt_rows_wave_kernel<true, 0, 1, false, 0>", "ntt_rows_wave_kernel<true, 0, 1, true, 0>", "ntt_rows_wave_kernel<true, 0, 2, false, 0>", "ntt_rows_wave_kernel<true, 0, 2, true, 0>",
    "ntt_rows_wave_kernel<true, 0, 3, false, 0>", "ntt_rows_wave_kernel<true, 0, 3, true, 0>", "ntt_rows_wave_kernel<true, 0, 4, false, 0>", "ntt_rows_wave_kernel<true, 0, 4, true, 0>",
    "ntt_rows_wave_kernel<true, 4, 1, false, 0>", "ntt_rows_wave_kernel<true, 4, 1, true, 0>", "ntt_rows_wave_kernel<true, 4, 3, false, 0>", "ntt_rows_wave_kernel<true, 4, 3, true, 0>",
    "ntt_rows_wave_kernel<true, 4, 4, false, 0>", "ntt_rows_wave_kernel<true, 4, 4, true, 0>",
    "ntt_rows_wave_kernel<true, 5, 1, false, 0>", "ntt_rows_wave_kernel<true, 5, 1, true, 0>", "ntt_rows_wave_kernel<true, 5, 3, false, 0>", "ntt_rows_wave_kernel<true, 5, 3, true, 0>",
    "ntt_rows_wave_kernel<true, 5, 4, false, 0>", "ntt_rows_wave_kernel<true, 5, 4, true, 0>",
    "ntt_rows_wave_kernel<true, 6, 1, false, 0>", "ntt_rows_wave_kernel<true, 6, 1, true, 0>", "ntt_rows_wave_kernel<true, 6, 3, false, 0>", "ntt_rows_wave_kernel<true, 6, 3, true, 0>",
    "ntt_rows_wave_kernel<true, 6, 4, false, 0>", "ntt_rows_wave_kernel<true, 6, 4, true, 0>"};

int main()
{
    for (size_t i = 0; i < CLASSES.size(); i++) {                  // the classes are what their names say
        int widest = 0;
        for (uint64_t q : CLASSES[i].q) if (q != Q54) widest = bit_length(q) > widest ? bit_length(q) : widest;
        if (widest != WIDTHS[i]) FAIL("class %s is %d bits wide", CLASSES[i].name, widest);
    }
    const long cases = walk_default();
    const long tuning = walk_cases();
    walk_refusals();
    size_t recorded = 0;
    for (const char *name : RECORDED) { recorded++; if (!names.count(name)) FAIL("the default walk never named %s", name); }
    if (recorded != 60) FAIL("%zu recorded names", recorded);
    for (const std::string &s : names) if (s.find("prefetch") != std::string::npos) FAIL("default tuning reached %s", s.c_str());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok cases %ld tuning %ld refusals %ld names %zu\n", cases, tuning, refusals, names.size());
    return 0;
}
