// level_keys_host -- a derived level of the host classes (tests/test_gpu_level_keys.py): makeLevel(kept, true) restricts the evaluation and Galois keys of the
// parameters on the device, and a tensor goes on there without a key generated at the level.
//
//   level_keys_host <dir>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/values.i64 = [n] int64: slot j of the one ciphertext holds values[j].
// The chain: encryptImageSlots under all k moduli -> modSwitch to the derived level of k - 1 -> squareRelin -> rotateRows(1) -> decryptSlots through the level.
// Writes <dir>/switched.i64, <dir>/square.i64 and <dir>/rotated.i64 ([n], decrypted and decomposed); prints "budget <name> <min bits>", "level key_moduli <K> k
// <k'> derived <0|1>", "throws <case> <exception kind>" and "level_keys_host ok" at the end.
#include "crcnn_host.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
using namespace std;

static vector<uint64_t> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<uint64_t> v(sz / 8); f.read((char *)v.data(), sz); return v;
}
static string dir;
static int n = 0;
static void put(const string &name, const LevelTensor &t)
{
    printf("budget %s %d\n", name.c_str(), minNoiseBudget(t));
    const vector<vector<int64_t>> v = decryptSlots(t, n);
    vector<int64_t> flat((size_t)n);
    for (int i = 0; i < n; i++) flat[i] = v[i][0];
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    f.write((const char *)flat.data(), flat.size() * 8);
}
static void thrown(const char *name, const function<void()> &call)
{
    const char *kind = "nothing";
    try { call(); } catch (const invalid_argument &) { kind = "invalid_argument"; } catch (const logic_error &) { kind = "logic_error"; }
    catch (const exception &) { kind = "exception"; }
    printf("throws %s %s\n", name, kind);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: level_keys_host <dir>\n"); return 1; }
    try {
        dir = argv[1];
        setDeterministicSeed(20250301);
        const auto p = rd(dir + "/params.u64");
        n = (int)p[0]; const int k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        setParameters(n, q, p[2], 0);
        setSlotEncoding(0, 0);
        generateGaloisKeys(16);
        const auto raw = rd(dir + "/values.i64");
        vector<vector<int64_t>> images(n, vector<int64_t>(1));
        for (int j = 0; j < n; j++) images[j][0] = (int64_t)raw[j];
        const ciphertext3D x = encryptImageSlots(images, 1, 1, 1);

        const shared_ptr<Level> L = makeLevel(k - 1, true), plain = makeLevel(k - 1);
        printf("level key_moduli %d k %d derived %d\n", crc_ctx_key_moduli(L->ctx), crc_ctx_k(L->ctx), (int)L->derived);
        printf("level key_moduli %d k %d derived %d\n", crc_ctx_key_moduli(plain->ctx), crc_ctx_k(plain->ctx), (int)plain->derived);
        const LevelTensor y = modSwitch(x, L);
        put("switched", y);
        const LevelTensor s = squareRelin(y);
        put("square", s);
        const LevelTensor r = rotateRows(s, 1);
        put("rotated", r);
        // NTT-resident between the two: the same plaintext
        put("rotated_ntt", rotateRows(squareRelin(modSwitch(x, L, CRC_NTT), CRC_NTT), 1));

        const LevelTensor yp = modSwitch(x, plain);
        thrown("square_plain_level", [&] { squareRelin(yp); });
        thrown("rotate_plain_level", [&] { rotateRows(yp, 1); });
        thrown("rotate_too_far", [&] { rotateRows(y, n / 2); });
        thrown("square_bad_form", [&] { squareRelin(y, CRC_NTTP); });
        thrown("square_no_level", [&] { LevelTensor e = y; e.level.reset(); squareRelin(e); });
        // a key set without the element of the step: the planner's exception, as at the top
        generateGaloisKeys(16, {crc_galois_elt_columns(context)});
        const shared_ptr<Level> few = makeLevel(k - 1, true);
        thrown("rotate_key_not_present", [&] { rotateRows(modSwitch(x, few), 1); });
        delParameters();
        thrown("stale_level_square", [&] { squareRelin(y); });
        clearDeterministicSeed();
        printf("level_keys_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "level_keys_host: %s\n", e.what()); return 4; }
}
