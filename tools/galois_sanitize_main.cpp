// galois_sanitize_main -- the host side of the Galois feature (element helpers, the rotation planner, Galois key generation) as a stand-alone program for the
// host sanitizers.  Host code only: it creates a host-only context (device = -1), launches nothing and is loaded into no interpreter.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -I crcnn_amd/csrc \
//         tools/galois_sanitize_main.cpp crcnn_amd/csrc/client.cpp crcnn_amd/csrc/ctx.cpp -o galois_sanitize -pthread && ./galois_sanitize
//
// (client.cpp's secret-key encryptor reads the device encryptor's threshold table, which lives with the kernels: a stub stands in for it here, that code is not run)
#include "../include/crcnn_hip.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

void k_encrypt_cdt(uint64_t *out19) { for (int i = 0; i < 19; i++) out19[i] = ~(uint64_t)0; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "galois_sanitize: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    const struct { int n; std::vector<uint64_t> q; } sets[] = {{64, {0x3fffffff000001ULL}}, {256, {0x7fffffff380001ULL, 0x3fffffff000001ULL}}, {2048, {0x3fffffff000001ULL}}};
    for (const auto &s : sets) {
        crc_ctx *c = nullptr;
        CHECK(crc_ctx_create(s.n, s.q.data(), (int)s.q.size(), 1 << 20, -1, &c) == CRC_OK);
        const int n = s.n, k = (int)s.q.size();
        std::vector<uint64_t> elts(crc_galois_default_elts(c, nullptr, 0));
        CHECK((int)elts.size() == crc_galois_default_elts(c, elts.data(), (int)elts.size()));
        CHECK(crc_galois_default_elts(c, elts.data(), (int)elts.size() - 1) == CRC_ERR_INVALID_ARGUMENT);
        // every element and every step count through the planner, with the full set, with a set that lacks an element, with no room for the answer
        std::vector<int> plan(64);
        for (uint64_t g = 0; g < 2 * (uint64_t)n + 4; g++) {
            const int full = crc_galois_plan(c, g, elts.data(), (int)elts.size(), plan.data(), (int)plan.size());
            CHECK(crc_galois_elt_valid(c, g) ? full >= 0 : full == CRC_ERR_INVALID_ARGUMENT);
            for (int i = 0; i < full; i++) CHECK(plan[i] >= 0 && plan[i] < (int)elts.size());
            crc_galois_plan(c, g, elts.data() + 1, (int)elts.size() - 1, plan.data(), (int)plan.size());
            crc_galois_plan(c, g, elts.data(), (int)elts.size(), plan.data(), 1);
            crc_galois_plan(c, g, nullptr, 0, nullptr, 0);
        }
        for (int st = -n; st <= n; st++) {
            const uint64_t g = crc_galois_elt_rows(c, st);
            CHECK((g != 0) == (st > -n / 2 && st < n / 2));
        }
        CHECK(crc_galois_elt_rows(c, INT32_MIN) == 0 && crc_galois_elt_rows(c, INT32_MAX) == 0);
        std::vector<uint64_t> sk((size_t)k * n), pk((size_t)2 * k * n);
        CHECK(crc_keygen(c, 5, sk.data(), pk.data()) == CRC_OK);
        for (int dbc : {16, 8, 60}) {
            const size_t words = crc_evk_words(c, dbc);
            std::vector<uint64_t> gk(elts.size() * words), again(gk.size());
            CHECK(crc_gen_galois_keys(c, 6, sk.data(), dbc, elts.data(), (int)elts.size(), gk.data()) == CRC_OK);
            CHECK(crc_gen_galois_keys(c, 6, sk.data(), dbc, elts.data(), (int)elts.size(), again.data()) == CRC_OK);
            CHECK(gk == again);
            for (size_t i = 0; i < gk.size(); i++) CHECK(gk[i] < s.q[(i / n) % k]);
        }
        std::vector<uint64_t> one(crc_evk_words(c, 16));
        const uint64_t bad = 2, last = 2 * (uint64_t)n - 1;
        CHECK(crc_gen_galois_keys(c, 6, sk.data(), 16, &bad, 1, one.data()) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_gen_galois_keys(c, 6, sk.data(), 0, &last, 1, one.data()) == CRC_ERR_INVALID_ARGUMENT);
        CHECK(crc_gen_galois_keys(c, 6, sk.data(), 16, &last, 1, one.data()) == CRC_OK);
        CHECK(crc_gen_galois_keys(c, 6, sk.data(), 16, nullptr, 0, nullptr) == CRC_OK);
        crc_ctx_destroy(c);
    }
    printf("galois_sanitize ok\n");
    return 0;
}
