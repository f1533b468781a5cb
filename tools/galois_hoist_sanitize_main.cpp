// galois_hoist_sanitize_main -- the host side of the hoisted rotations (the NTT-domain index table, the key conjugation, the diagonal planner) as a stand-alone
// program for the host sanitizers.  Host code only: it creates a host-only context (device = -1), launches nothing and is loaded into no interpreter.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -I crcnn_amd/csrc \
//         tools/galois_hoist_sanitize_main.cpp crcnn_amd/csrc/client.cpp crcnn_amd/csrc/ctx.cpp -o galois_hoist_sanitize -pthread && ./galois_hoist_sanitize
//
// (client.cpp's secret-key encryptor reads the device encryptor's threshold table, which lives with the kernels: a stub stands in for it here, that code is not run)
#include "../include/crcnn_hip.h"
#include "../crcnn_amd/host/diag_plan.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

void k_encrypt_cdt(uint64_t *out19) { for (int i = 0; i < 19; i++) out19[i] = ~(uint64_t)0; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "galois_hoist_sanitize: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    const struct { int n; std::vector<uint64_t> q; } sets[] = {{64, {0x3fffffff000001ULL}}, {256, {0x7fffffff380001ULL, 0x3fffffff000001ULL}}, {2048, {0x3fffffff000001ULL}}};
    for (const auto &s : sets) {
        crc_ctx *c = nullptr;
        CHECK(crc_ctx_create(s.n, s.q.data(), (int)s.q.size(), 1 << 20, -1, &c) == CRC_OK);
        const int n = s.n, k = (int)s.q.size();
        // the table of every element is a permutation of 0..n-1; tables compose as the elements multiply; invalid elements and a null table are refused
        std::vector<uint32_t> ta(n), tb(n), tab(n);
        for (uint64_t g = 0; g < 2 * (uint64_t)n + 4; g++) {
            const int rc = crc_galois_ntt_table(c, g, ta.data());
            CHECK(crc_galois_elt_valid(c, g) ? rc == CRC_OK : rc == CRC_ERR_INVALID_ARGUMENT);
            if (rc) continue;
            std::vector<uint32_t> sorted(ta);
            std::sort(sorted.begin(), sorted.end());
            for (int i = 0; i < n; i++) CHECK(sorted[i] == (uint32_t)i);
            const uint64_t h = 3;
            CHECK(crc_galois_ntt_table(c, h, tb.data()) == CRC_OK && crc_galois_ntt_table(c, g * h % (2 * (uint64_t)n), tab.data()) == CRC_OK);
            for (int i = 0; i < n; i++) CHECK(tab[i] == ta[tb[i]]);            // the gather of g h is the gather of h, then the gather of g
        }
        CHECK(crc_galois_ntt_table(c, 3, nullptr) == CRC_ERR_INVALID_ARGUMENT && crc_galois_ntt_table(nullptr, 3, ta.data()) == CRC_ERR_INVALID_ARGUMENT);
        std::vector<uint64_t> elts(crc_galois_default_elts(c, nullptr, 0));
        CHECK((int)elts.size() == crc_galois_default_elts(c, elts.data(), (int)elts.size()));
        std::vector<uint64_t> sk((size_t)k * n), pk((size_t)2 * k * n);
        CHECK(crc_keygen(c, 5, sk.data(), pk.data()) == CRC_OK);
        for (int dbc : {16, 8, 60}) {
            const size_t words = crc_evk_words(c, dbc);
            std::vector<uint64_t> gk(elts.size() * words), cg(gk.size()), back(gk.size());
            CHECK(crc_gen_galois_keys(c, 6, sk.data(), dbc, elts.data(), (int)elts.size(), gk.data()) == CRC_OK);
            CHECK(crc_galois_conjugate_keys(c, elts.data(), (int)elts.size(), dbc, gk.data(), cg.data()) == CRC_OK);
            for (size_t i = 0; i < cg.size(); i++) CHECK(cg[i] < s.q[(i / n) % k]);
            // conjugating the conjugated blob of g with the element g^-1 gives the blob back: sigma_g(sigma_g^-1(K)) = K
            std::vector<uint64_t> inv(elts.size());
            for (size_t e = 0; e < elts.size(); e++) { uint64_t h = 1; for (int i = 0; i < n - 1; i++) h = h * elts[e] % (2 * (uint64_t)n); inv[e] = h; }
            CHECK(crc_galois_conjugate_keys(c, inv.data(), (int)inv.size(), dbc, cg.data(), back.data()) == CRC_OK);
            CHECK(back == gk);
            CHECK(crc_galois_conjugate_keys(c, elts.data(), (int)elts.size(), dbc, gk.data(), gk.data()) == CRC_ERR_INVALID_ARGUMENT);
        }
        std::vector<uint64_t> one(crc_evk_words(c, 16)), two(one.size());
        const uint64_t bad = 2, unit = 1, last = 2 * (uint64_t)n - 1;
        CHECK(crc_galois_conjugate_keys(c, &bad, 1, 16, one.data(), two.data()) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_galois_conjugate_keys(c, &unit, 1, 16, one.data(), two.data()) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_galois_conjugate_keys(c, &last, 1, 0, one.data(), two.data()) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_galois_conjugate_keys(c, &last, 1, 16, one.data(), nullptr) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_galois_conjugate_keys(c, &last, 1, 16, one.data(), two.data()) == CRC_OK);
        CHECK(crc_galois_conjugate_keys(c, nullptr, 0, 16, nullptr, nullptr) == CRC_OK);
        // the diagonal planner: every M up to n/2 with square, rectangular, ragged and empty matrices; the plan reproduces W x on a tiled vector
        std::vector<int> steps; std::vector<int64_t> rows;
        for (int M = 1; M <= n / 2; M *= 2) {
            if (M > 32 && M != n / 2) continue;
            std::vector<std::vector<int64_t>> W(M, std::vector<int64_t>(M));
            for (int i = 0; i < M; i++) for (int j = 0; j < M; j++) W[i][j] = (i * 31 + j * 7) % 5 == 0 ? 0 : i * M + j + 1;
            if (M > 2) { W.resize(M - 1); W[0].resize(M - 2); }                 // rectangular and ragged
            CHECK(crc_diag_plan(W, M, n, steps, rows));
            CHECK(rows.size() == steps.size() * (size_t)n);
            std::vector<int64_t> x(M), y(M, 0), want(M, 0);
            for (int j = 0; j < M; j++) x[j] = j + 2;
            for (size_t i = 0; i < W.size(); i++) for (size_t j = 0; j < W[i].size(); j++) want[i] += W[i][j] * x[j];
            for (size_t r = 0; r < steps.size(); r++) for (int i = 0; i < M; i++) y[i] += rows[r * n + i] * x[(i + steps[r]) % M];
            CHECK(y == want);
            for (size_t r = 0; r < steps.size(); r++) for (int i = 0; i < n; i++) CHECK(rows[r * n + i] == rows[r * n + i % M]);
        }
        CHECK(crc_diag_plan({}, 4, n, steps, rows) && steps.empty() && rows.empty());
        CHECK(!crc_diag_plan({{1}}, 3, n, steps, rows) && !crc_diag_plan({{1}}, 0, n, steps, rows) && !crc_diag_plan({{1}}, n, n, steps, rows));
        CHECK(!crc_diag_plan({{1, 2, 3}}, 2, n, steps, rows) && !crc_diag_plan({{1}, {2}, {3}}, 2, n, steps, rows));
        crc_ctx_destroy(c);
    }
    printf("galois_hoist_sanitize ok\n");
    return 0;
}
