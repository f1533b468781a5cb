// box_sum_check.cpp -- the reduction of the one-channel kernel's box (crcnn_amd/csrc/limbred.h sum_reduce16: the canonical residue of a sum of canonical residues)
// against 128-bit arithmetic: all eight moduli of default_coeff_modulus_128, every term count from 1 to 9 (the kernel's cap) and on to 15 (the helper's own
// bound), operands 0, q - 1, (q - 1) / 2, (q + 1) / 2 in every position pattern and random ones.  A stand-alone program: it builds with host sanitizers.
#include <cstdio>
#include <cstdlib>
#include "limbred.h"

// default_coeff_modulus_128(n), n = 2048 .. 16384 (ctx.cpp crc_default_coeff_modulus_128): the union of the sets
static const u64 kModuli[8] = {0x3fffffff000001ULL, 0x7fffffff380001ULL, 0x7ffffffef00001ULL, 0x3ffffffef40001ULL,
                               0x7ffffffeac0001ULL, 0x7ffffffe700001ULL, 0x7ffffffe600001ULL, 0x7ffffffe4c0001ULL};
static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main()
{
    typedef unsigned __int128 u128;
    long checked = 0;
    for (u64 q : kModuli) {
        const u64 edge[4] = {0, q - 1, (q - 1) / 2, (q + 1) / 2};
        for (int terms = 1; terms <= 15; terms++) {
            auto check = [&](const u64 *v) {
                u64 s = 0; u128 wide = 0;
                for (int t = 0; t < terms; t++) { s += v[t]; wide += v[t]; }
                const u64 got = sum_reduce16(s, q), want = (u64)(wide % q);
                if (got != want || (u128)s != wide) {
                    printf("FAIL q=%llx terms=%d got=%llx want=%llx\n", (unsigned long long)q, terms, (unsigned long long)got, (unsigned long long)want);
                    exit(1);
                }
                checked++;
            };
            u64 v[15];
            // every term the same edge value; one term different; edge values cycling from every start
            for (int e = 0; e < 4; e++) {
                for (int t = 0; t < terms; t++) v[t] = edge[e];
                check(v);
                for (int o = 0; o < 4; o++) for (int at = 0; at < terms; at++) { const u64 keep = v[at]; v[at] = edge[o]; check(v); v[at] = keep; }
                for (int t = 0; t < terms; t++) v[t] = edge[(e + t) & 3];
                check(v);
            }
            for (int it = 0; it < 4000; it++) {
                for (int t = 0; t < terms; t++) v[t] = (it & 3) == 3 ? edge[rnd() & 3] : rnd() % q;
                check(v);
            }
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}
