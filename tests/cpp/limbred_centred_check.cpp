// limbred_centred_check.cpp -- the one-pass centred reduction of the limb GEMM's epilogue (limbred.h: diag_reduce_w_centred) on the CPU.
//
// For every modulus of default_coeff_modulus_128(n), n = 2048 .. 16384, that has a fold constant: biased diagonals D'_d = B_d + D_d, B = limb_bias_table(q, T) for
// T in {32, 800, 1024, 1152, 17 984}, |D_d| <= T (min(d, 12 - d) + 1) 2^14 --
//   * random diagonals in that range;
//   * every diagonal at its largest and at its smallest admissible value: all 13 at once, one at a time beside random ones, and random patterns of the two ends;
//   * diagonals moved (by the balanced digits of the distance, as bias_to_multiple moves the table) so that U 2^-64 mod q is exactly 0, (q - 1) / 2 and
//     -(q - 1) / 2, and biases chosen so that U 2^-64 + bias hits the same three values;
// each with the biases 0, 1, (q - 1) / 2, (q + 1) / 2, q - 1 and a random one through diag_reduce_w_centred<true>, and through diag_reduce_w_centred<false>.
// The result must be the centred representative of addmod(diag_reduce_w(D), bias) -- the three-correction sequence it replaces -- and of (U 2^-64 + bias) mod q in
// unsigned __int128 arithmetic, and lie in [-(q - 1) / 2, (q - 1) / 2].  Prints "ok <checked results>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include "limbred.h"

typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static ModParams make(u64 q)
{
    ModParams m{}; const u128 quo = ~(u128)0 / q;
    m.q = q; m.r0 = (u64)quo; m.r1 = (u64)(quo >> 64); m.two_q = 2 * q; m.bits = 64 - __builtin_clzll(q);
    m.fold = fold_constant(q, m.bits);
    return m;
}
static u64 powmod(u64 b, u64 e, u64 q) { u64 r = 1; b %= q; while (e) { if (e & 1) r = (u64)((u128)r * b % q); b = (u64)((u128)b * b % q); e >>= 1; } return r; }
static long long centre(u64 r, u64 q) { return r > (q >> 1) ? (long long)(r - q) : (long long)r; }

static long checked = 0;

struct Case {
    ModParams m; u64 qinv, Rinv; int B[13]; long long bound[13];      // Rinv: 2^-64 mod q (q prime)
};

static u128 value_of(const int (&D)[13]) { u128 U = 0; for (int d = 0; d < 13; d++) U += (u128)(u32)D[d] << (8 * d); return U; }
// U 2^-64 mod q in 128-bit arithmetic
static u64 direct(const Case &c, const int (&D)[13]) { return (u64)((u128)(u64)(value_of(D) % c.m.q) * c.Rinv % c.m.q); }

static void check_one(const Case &c, const int (&D)[13], u64 bias, bool has_bias, const char *what)
{
    const u64 q = c.m.q;
    const long long h = (long long)(q >> 1);
    const u64 canon = diag_reduce_w(D, c.m, c.qinv);
    const u64 dir = direct(c, D);
    CHECK(canon == dir, "%s: diag_reduce_w %llx differs from 128-bit arithmetic %llx (q %llx)", what, (unsigned long long)canon, (unsigned long long)dir, (unsigned long long)q);
    long long got, want_seq, want_dir;
    if (has_bias) {
        got = diag_reduce_w_centred<true>(D, c.m, c.qinv, centred_rep(bias, q));
        want_seq = centre(addmod(canon, bias, q), q);
        want_dir = centre((u64)(((u128)dir + bias) % q), q);
    } else {
        got = diag_reduce_w_centred<false>(D, c.m, c.qinv, 0);
        want_seq = centre(canon, q); want_dir = centre(dir, q);
    }
    CHECK(got == want_seq && got == want_dir, "%s: q %llx bias %llx (%d): got %lld, sequence %lld, 128-bit %lld", what, (unsigned long long)q, (unsigned long long)bias, (int)has_bias,
          got, want_seq, want_dir);
    CHECK(got >= -h && got <= h, "%s: %lld outside the centred range of q %llx", what, got, (unsigned long long)q);
    CHECK(centred_digit_bytes(got) == balanced_digit_bytes((u64)(got < 0 ? got + (long long)q : got), q), "%s: digit bytes differ", what);
    checked++;
}

static void check_all_biases(const Case &c, const int (&D)[13], std::mt19937_64 &rng, const char *what)
{
    const u64 q = c.m.q;
    const u64 biases[] = {0, 1, (q - 1) / 2, (q + 1) / 2, q - 1, rng() % q};
    for (u64 b : biases) check_one(c, D, b, true, what);
    check_one(c, D, 0, false, what);
}

// move U 2^-64 mod q to `target` (canonical) by adding the balanced digits of the centred distance to D_0 .. D_7 (at most 128 each)
static void move_to(const Case &c, int (&D)[13], u64 target)
{
    const u64 q = c.m.q;
    const u64 R = (u64)(((u128)1 << 64) % q);
    const u64 have = (u64)(value_of(D) % q), need = (u64)((u128)target * R % q);
    long long delta = centre(submod(need, have, q), q);
    for (int d = 0; d < 8 && delta; d++) { const long long dg = (long long)(signed char)(delta & 0xff); D[d] = (int)((u32)D[d] + (u32)(int)dg); delta = (delta - dg) >> 8; }
    if (delta) { printf("FAIL: the distance does not fit eight balanced digits\n"); exit(1); }
}

static void run(u64 q, int T, std::mt19937_64 &rng)
{
    Case c; c.m = make(q); c.qinv = inverse_mod_2_64(q); c.Rinv = powmod((u64)(((u128)1 << 64) % q), q - 2, q);
    CHECK(q * c.qinv == 1, "inverse_mod_2_64");
    CHECK((u64)((u128)(u64)(((u128)1 << 64) % q) * c.Rinv % q) == 1, "2^-64 mod q");
    limb_bias_table(q, T, c.B);
    for (int d = 0; d < 13; d++) {
        c.bound[d] = (long long)T * ((d < 12 - d ? d : 12 - d) + 1) * 16384;
        CHECK((long long)(u32)c.B[d] - c.bound[d] > 0 && (long long)(u32)c.B[d] + c.bound[d] < ((long long)1 << 32), "bias %d of T = %d leaves the word", d, T);
    }
    CHECK(value_of(c.B) % q == 0, "the bias table is not a multiple of q");
    auto biased = [&](int d, long long v) { return (int)(u32)((long long)(u32)c.B[d] + v); };
    auto rand_in = [&](int d, long long slack) { const long long b = c.bound[d] - slack; return (long long)(rng() % (u64)(2 * b + 1)) - b; };
    int D[13];
    // random diagonals
    for (int rep = 0; rep < 700; rep++) {
        for (int d = 0; d < 13; d++) D[d] = biased(d, rand_in(d, 0));
        check_all_biases(c, D, rng, "random");
    }
    // the ends of the range: all at once, one at a time, random patterns
    for (int end = 0; end < 2; end++) {
        for (int d = 0; d < 13; d++) D[d] = biased(d, end ? c.bound[d] : -c.bound[d]);
        check_all_biases(c, D, rng, "all diagonals at one end");
        for (int one = 0; one < 13; one++)
            for (int rep = 0; rep < 4; rep++) {
                for (int d = 0; d < 13; d++) D[d] = biased(d, d == one ? (end ? c.bound[d] : -c.bound[d]) : rand_in(d, 0));
                check_all_biases(c, D, rng, "one diagonal at its end");
            }
    }
    for (int rep = 0; rep < 150; rep++) {
        const u64 pat = rng();
        for (int d = 0; d < 13; d++) D[d] = biased(d, (pat >> d) & 1 ? c.bound[d] : -c.bound[d]);
        check_all_biases(c, D, rng, "a pattern of ends");
    }
    // results exactly 0, (q - 1) / 2, -(q - 1) / 2: from the diagonals alone, and from the bias
    const u64 targets[] = {0, (q - 1) / 2, q - (q - 1) / 2};
    for (int rep = 0; rep < 60; rep++)
        for (u64 target : targets) {
            for (int d = 0; d < 13; d++) D[d] = biased(d, rand_in(d, 128));
            move_to(c, D, target);
            CHECK(direct(c, D) == target, "move_to missed its target");
            CHECK(diag_reduce_w_centred<false>(D, c.m, c.qinv, 0) == centre(target, q), "the exact value %lld is missed", centre(target, q));
            CHECK(diag_reduce_w_centred<true>(D, c.m, c.qinv, 0) == centre(target, q), "the exact value %lld is missed with a zero bias", centre(target, q));
            check_all_biases(c, D, rng, "diagonals at an exact value");
            for (int d = 0; d < 13; d++) D[d] = biased(d, rand_in(d, 0));
            const u64 bias = submod(target, direct(c, D), q);
            CHECK(diag_reduce_w_centred<true>(D, c.m, c.qinv, centred_rep(bias, q)) == centre(target, q), "the exact value %lld is missed through the bias", centre(target, q));
            check_one(c, D, bias, true, "bias to an exact value");
        }
}

int main()
{
    std::mt19937_64 rng(20261019);
    // default_coeff_modulus_128(n), n = 2048 .. 16384 (ctx.cpp crc_default_coeff_modulus_128): the union of the sets
    const u64 mods[] = {0x3fffffff000001, 0x7fffffff380001, 0x7ffffffef00001, 0x3ffffffef40001, 0x7ffffffeac0001, 0x7ffffffe700001, 0x7ffffffe600001, 0x7ffffffe4c0001};
    const int Ts[] = {32, 800, 1024, 1152, 17984};
    int folded = 0;
    for (u64 q : mods) {
        if (!make(q).fold) continue;
        folded++;
        for (int T : Ts) run(q, T, rng);
    }
    CHECK(folded == 8, "only %d of the 8 default moduli have a fold constant", folded);
    if (fails) { printf("FAILED %d checks\n", fails); return 1; }
    printf("ok %ld\n", checked);
    return 0;
}
