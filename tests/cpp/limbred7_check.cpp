// limbred7_check.cpp -- the seven-diagonal, one-fold reduction of the pixel-major one-channel kernel (limbred.h: conv1_bias7_table, conv1_fold7_ok,
// diag7_pack_words, fold7_words_centred) on the CPU against 128-bit arithmetic.
//
// For every modulus conv1_fold7_ok accepts among the default 128-bit-security sets (n = 2048 .. 16384) and T in {1, 36, 40, 64} taps: image residues x_t and
// weights w_t (random, and the edge values 0, 1, q-1, q/2, q/2+1, all-extreme digits); the kernel's arithmetic is replayed literally -- image digits a_l, weight
// digits W'_{l,m} of centred(w 256^l mod q), E_m accumulated in int32 -- and diag7_fold_centred(E, bias) must be the centred representative of
// sum x_t w_t + bias mod q.  Worst-case diagonals (every E_m at +-T 7 2^14, beyond what digits of a value below q/2 can reach) check the bounds of the pack and
// of the fold: U positive, U >> b within 20 bits, the folded value below 2q.  conv1_fold7_ok must refuse f >= 2^26, b outside 53..55 and q != 2^b - f.
// Prints "ok <checked outputs>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "limbred.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void digits7(long long v, int (&d)[7])
{
    for (int l = 0; l < 7; l++) { d[l] = (int)(signed char)(v & 0xff); v = (v - d[l]) >> 8; }
    if (v != 0) { printf("FAIL: a centred value does not fit seven balanced digits\n"); exit(1); }
}
static long long centred(u64 r, u64 q) { return r > (q >> 1) ? (long long)(r - q) : (long long)r; }
static u64 mulmod128(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }

// what diag7_fold_centred must return for the integer V (any sign) and a centred bias
static long long want_centred(i128 V, long long bias, u64 q)
{
    i128 r = (V + bias) % (i128)q;
    if (r < 0) r += q;
    return centred((u64)r, q);
}

static long checked = 0;

static void check_fold_bounds(const int (&E)[7], const u32 (&PB)[4], u64 q, u32 bits, u32 fold)
{
    u32 u[3];
    diag7_pack_words(E, PB, u);
    const u128 U = ((u128)u[2] << 64) | ((u128)u[1] << 32) | u[0];
    CHECK(U > 0 && u[2] < (1u << 9), "U out of range");
    const u128 uh = U >> bits;
    CHECK(uh < ((u128)1 << 20), "U >> b exceeds 20 bits");
    const u128 folded = (U & (((u128)1 << bits) - 1)) + uh * fold;
    CHECK(folded < (u128)2 * q, "the folded value reaches 2q");
}

static void run_modulus(u64 q, std::mt19937_64 &rng)
{
    u32 bits = 0; while ((q >> bits) != 0) bits++;
    const u32 fold = fold_constant(q, bits);
    if (!conv1_fold7_ok(q, bits, fold)) { printf("FAIL: conv1_fold7_ok refuses %llx\n", (unsigned long long)q); fails++; return; }
    int B[7]; conv1_bias7_table(q, B);
    u128 K0 = 0;
    for (int m = 0; m < 7; m++) { K0 += (u128)(u64)B[m] << (8 * m); CHECK(B[m] > 64 * 7 * 16384 && B[m] + 64 * 7 * 16384 < (1 << 24), "bias %d out of range", m); }
    CHECK(K0 % q == 0, "the biases are not a multiple of q");
    u32 PB[4];
    for (int j = 0; j < 3; j++) PB[j] = (u32)B[2 * j] + ((u32)B[2 * j + 1] << 8);
    PB[3] = (u32)B[6];
    // the residues with extreme digits: d0..d5 all -128 / all +127 and d6 as far out as |c| <= q/2 allows
    auto extreme = [&](bool low) {
        const long long d05 = low ? -128 : 127, h = (long long)(q >> 1);
        long long base = 0;
        for (int l = 0; l < 6; l++) base += d05 * ((long long)1 << (8 * l));
        long long d6 = low ? -((h + base) >> 48) : (h - base) >> 48;
        const long long c = base + d6 * ((long long)1 << 48);
        return (u64)(c < 0 ? c + (long long)q : c);
    };
    const u64 edge[] = {0, 1, q - 1, q >> 1, (q >> 1) + 1, extreme(true), extreme(false)};
    const int NE = sizeof(edge) / sizeof(edge[0]);
    // 256^-l mod q: weights e 256^-l make W'_l = e, every digit of that plane extreme
    u64 inv256 = 1;
    { u64 base = 256 % q, e = q - 2, r = 1; while (e) { if (e & 1) r = mulmod128(r, base, q); base = mulmod128(base, base, q); e >>= 1; } inv256 = r; }
    const long long biases[] = {0, (long long)(q >> 1), -(long long)(q >> 1), -1, 1};
    const int Ts[] = {1, 36, 40, 64};
    for (int T : Ts) {
        for (int mode = 0; mode < 12; mode++) {
            const int reps = mode == 0 ? 400 : 40;
            for (int rep = 0; rep < reps; rep++) {
                std::vector<u64> x(T), w(T);
                for (int t = 0; t < T; t++) {
                    if (mode == 0) { x[t] = rng() % q; w[t] = rng() % q; }
                    else if (mode == 1) { x[t] = edge[rng() % NE]; w[t] = edge[rng() % NE]; }
                    else if (mode <= 4) { x[t] = edge[mode == 4 ? 6 : 5]; w[t] = edge[mode == 2 ? 5 : 6]; }        // all-extreme digits: (-,-), (-,+), (+,+)
                    else {                                                                                           // W'_l extreme for l = mode - 5
                        x[t] = edge[5 + (rep & 1)];
                        u64 e = edge[5 + ((rep >> 1) & 1)];
                        for (int l = 0; l < mode - 5; l++) e = mulmod128(e, inv256, q);
                        w[t] = e;
                    }
                }
                int E[7] = {0, 0, 0, 0, 0, 0, 0};
                i128 V = 0;
                for (int t = 0; t < T; t++) {
                    int a[7]; digits7(centred(x[t], q), a);
                    u64 wl = w[t];
                    for (int l = 0; l < 7; l++) {
                        int d[7]; digits7(centred(wl, q), d);
                        for (int m = 0; m < 7; m++) E[m] += a[l] * d[m];
                        wl = mulmod128(wl, 256, q);
                    }
                    V += (i128)centred(x[t], q) * centred(w[t], q);
                }
                // the seven diagonals are V up to a multiple of q
                i128 S = 0;
                for (int m = 0; m < 7; m++) { S += (i128)E[m] << (8 * m); CHECK(E[m] <= T * 7 * 16384 && E[m] >= -T * 7 * 16384, "E_%d out of bounds", m); }
                CHECK((S - V) % (i128)q == 0, "sum E_m 256^m differs from x w mod q");
                check_fold_bounds(E, PB, q, bits, fold);
                for (long long bias : biases) {
                    const long long got = diag7_fold_centred(E, q, bits, fold, bias, PB), want = want_centred(V, bias, q);
                    CHECK(got == want, "q %llx T %d mode %d: got %lld want %lld", (unsigned long long)q, T, mode, got, want);
                    // the same from diagonals that arrive biased already
                    int Eb[7]; for (int m = 0; m < 7; m++) Eb[m] = E[m] + B[m];
                    CHECK(diag7_fold_centred(Eb, q, bits, fold, bias) == want, "pre-biased diagonals differ");
                    checked++;
                }
            }
        }
    }
    // worst-case diagonals at 64 taps: every E_m at either end of its range, all 128 sign patterns, and random values in the range
    const int EM = 64 * 7 * 16384;
    for (int pat = 0; pat < 128 + 2000; pat++) {
        int E[7];
        for (int m = 0; m < 7; m++) E[m] = pat < 128 ? ((pat >> m) & 1 ? EM : -EM) : (int)((long long)(rng() % (2 * (u64)EM + 1)) - EM);
        i128 V = 0;
        for (int m = 0; m < 7; m++) V += (i128)E[m] << (8 * m);
        check_fold_bounds(E, PB, q, bits, fold);
        for (long long bias : biases) {
            const long long got = diag7_fold_centred(E, q, bits, fold, bias, PB), want = want_centred(V, bias, q);
            CHECK(got == want, "q %llx worst-case pattern %d: got %lld want %lld", (unsigned long long)q, pat, got, want);
            checked++;
        }
    }
}

int main()
{
    std::mt19937_64 rng(20250607);
    // default_coeff_modulus_128(n), n = 2048 .. 16384 (ctx.cpp crc_default_coeff_modulus_128): the union of the sets
    const u64 mods[] = {0x3fffffff000001, 0x7fffffff380001, 0x7ffffffef00001, 0x3ffffffef40001, 0x7ffffffeac0001, 0x7ffffffe700001, 0x7ffffffe600001, 0x7ffffffe4c0001};
    int accepted = 0;
    for (u64 q : mods) {
        u32 bits = 0; while ((q >> bits) != 0) bits++;
        if (!conv1_fold7_ok(q, bits, fold_constant(q, bits))) continue;
        accepted++;
        run_modulus(q, rng);
    }
    CHECK(accepted == 8, "only %d of the 8 default moduli accepted", accepted);
    // refusals: f >= 2^26 (a 55-bit modulus without a fold constant, and one given its true distance), bits outside 53..55, q that is not 2^b - f
    const u64 q55nf = 0x7fffffbffd0001;
    CHECK(fold_constant(q55nf, 55) == 0 && !conv1_fold7_ok(q55nf, 55, 0), "a modulus without a fold constant passes");
    CHECK(!conv1_fold7_ok(q55nf, 55, (u32)(((u64)1 << 55) - q55nf)), "f >= 2^26 passes");
    CHECK(!conv1_fold7_ok(((u64)1 << 55) - (1u << 26), 55, 1u << 26), "f = 2^26 passes");
    CHECK(conv1_fold7_ok(((u64)1 << 55) - ((1u << 26) - 1), 55, (1u << 26) - 1), "f = 2^26 - 1 is refused");
    CHECK(!conv1_fold7_ok(0xffffe80001, 40, 0x17ffff), "a 40-bit modulus passes");
    CHECK(!conv1_fold7_ok(((u64)1 << 52) - 0xc0001 + 2, 52, 0xc0001 - 2), "a 52-bit modulus passes");
    CHECK(!conv1_fold7_ok(((u64)1 << 56) - 27, 56, 27), "a 56-bit modulus passes");
    CHECK(!conv1_fold7_ok(0x7fffffff380001, 55, 0xc7fffe), "a fold constant that is not 2^b - q passes");
    if (fails) { printf("FAILED %d checks\n", fails); return 1; }
    printf("ok %ld\n", checked);
    return 0;
}
