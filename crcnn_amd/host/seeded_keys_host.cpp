// seeded_keys_host -- seeded Galois keys through the host classes (tests/test_gpu_seeded_keys.py): the client makes the first rows on the host and on the
// device, the server installs them from a saved container, and rotations and a dense layer decrypt to what they decrypt to under generateGaloisKeys.
//
//   seeded_keys_host <dir>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/values.i64 = [n] int64: slot j of the one ciphertext holds values[j] (the test tiles a vector with period
// 16 whose entries sit at the even slots 0, 2, .., 10), <dir>/w.i64 = [3][1][6] int64 weights of a dense layer over those six entries, outputs at slots 0, 2, 4.
// Keys: the default set, 3^5, and densePlanesElements of the layer, each element once.
// Prints "seeded host_device equal|differs" (generateGaloisKeysSeeded on the host threads against the device, under the deterministic seed), "bytes seeded <container>
// blobs <blobs>", then per case (rows_1 = rotateRows(1), many_1 and many_5 = one rotateRowsMany call, dense = the densePlanes layer) writes <dir>/ref_<name>.i64
// under generateGaloisKeys and <dir>/seeded_<name>.i64 after save -> load -> installGaloisKeys (both [n], decrypted and decomposed) with "budget <case> <min bits>"
// and "plaintexts <name> equal|differs", then "throws <case> <exception kind>"; then, WITHOUT the deterministic seed, "repeat seed equal|differs element
// equal|differs others differ|equal" (element 3 made in two sets under one master key) and "fresh seed differs|equal element differs|equal" (after new parameters);
// "seeded_keys_host ok" at the end.
//
//   seeded_keys_host <dir> time <elements> <rounds>          (tools/measure_seeded_keys.py)
//
// The elements 3, 5, 7, ... at dbc 16: per round, alternating, the wall-clock time of generateGaloisKeys (host generation, upload, conjugation) and of
// installGaloisKeys on a set made once (upload of the rows, both expansions); both end in a stream synchronise.  Prints "time generate <ms> install <ms>" per
// round and "seeded_keys_host time ok".
#include "crcnn_host.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
using namespace std;

static vector<uint64_t> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<uint64_t> v(sz / 8); f.read((char *)v.data(), sz); return v;
}
static string dir;
static int n = 0;
static vector<int64_t> put(const string &name, const ciphertext3D &t)
{
    printf("budget %s %d\n", name.c_str(), minNoiseBudget(t));
    const vector<vector<int64_t>> v = decryptSlots(t, n);
    vector<int64_t> flat((size_t)n);
    for (int i = 0; i < n; i++) flat[i] = v[i][0];
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    f.write((const char *)flat.data(), flat.size() * 8);
    return flat;
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
    if (argc < 2) { fprintf(stderr, "usage: seeded_keys_host <dir>\n"); return 1; }
    try {
        dir = argv[1];
        setDeterministicSeed(20250117);
        const auto p = rd(dir + "/params.u64");
        n = (int)p[0]; const int k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        setParameters(n, q, p[2], 0);
        setSlotEncoding(0, 0);
        if (argc > 4 && string(argv[2]) == "time") {
            vector<uint64_t> e((size_t)atoi(argv[3]));
            for (size_t i = 0; i < e.size(); i++) e[i] = 2 * i + 3;
            const SeededKeys S = generateGaloisKeysSeeded(16, e, true);
            auto ms = [](const function<void()> &f) { const auto t0 = chrono::steady_clock::now(); f(); return chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count(); };
            installGaloisKeys(S);                                                   // (warm-up: code objects, allocations)
            for (int r = 0; r < atoi(argv[4]); r++) {
                const double g = ms([&] { generateGaloisKeys(16, e); }), i = ms([&] { installGaloisKeys(S); });
                printf("time generate %.3f install %.3f\n", g, i);
            }
            delParameters(); clearDeterministicSeed();
            printf("seeded_keys_host time ok\n");
            return 0;
        }
        const auto raw = rd(dir + "/values.i64"), wraw = rd(dir + "/w.i64");
        vector<vector<int64_t>> images(n, vector<int64_t>(1));
        for (int j = 0; j < n; j++) images[j][0] = (int64_t)raw[j];
        const vector<int64_t> w(wraw.begin(), wraw.end());
        const ciphertext3D x = encryptImageSlots(images, 1, 1, 1);
        const int M = 16;
        const vector<int> in_slots{0, 2, 4, 6, 8, 10}, out_slots{0, 2, 4};
        vector<uint64_t> elts(crc_galois_default_elts(context, nullptr, 0));
        crc_galois_default_elts(context, elts.data(), (int)elts.size());
        auto add = [&](uint64_t e) { if (find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e); };
        add(crc_galois_elt_rows(context, 5));
        for (uint64_t e : densePlanesElements(M, in_slots, 3, out_slots)) add(e);

        // the client, twice: host threads and device
        const SeededKeys A = generateGaloisKeysSeeded(16, elts, false), B = generateGaloisKeysSeeded(16, elts, true);
        const bool same = A.dbc == B.dbc && A.ids == B.ids && A.rows == B.rows && !memcmp(A.seed, B.seed, 32) && A.ids == elts;
        printf("seeded host_device %s\n", same ? "equal" : "differs");
        stringstream file;
        B.save(file);
        printf("bytes seeded %zu blobs %zu\n", file.str().size(), elts.size() * crc_evk_words(context, 16) * 8);

        auto run = [&](const string &tag) {
            map<string, vector<int64_t>> out;
            out["rows_1"] = put(tag + "_rows_1", rotateRows(x, 1));
            const vector<ciphertext3D> many = rotateRowsMany(x, {1, 5});
            out["many_1"] = put(tag + "_many_1", many[0]);
            out["many_5"] = put(tag + "_many_5", many[1]);
            out["dense"] = put(tag + "_dense", densePlanes(x, w, 3, M, in_slots, out_slots));
            return out;
        };
        generateGaloisKeys(16, elts);
        const auto ref = run("ref");
        // the server: nothing but the file
        SeededKeys C;
        C.load(file);
        installGaloisKeys(C);
        if (galois_elts != elts || !galois_keys_host.empty()) { fprintf(stderr, "seeded_keys_host: key set state\n"); return 5; }
        const auto got = run("seeded");
        for (auto &kv : ref) printf("plaintexts %s %s\n", kv.first.c_str(), kv.second == got.at(kv.first) ? "equal" : "differs");

        thrown("install_bad_dbc", [&] { SeededKeys D = C; D.dbc = 61; installGaloisKeys(D); });
        thrown("install_bad_element", [&] { SeededKeys D = C; D.ids[0] = 2; installGaloisKeys(D); });
        thrown("install_short_rows", [&] { SeededKeys D = C; D.rows.pop_back(); installGaloisKeys(D); });
        thrown("load_truncated", [&] { const string s = file.str(); stringstream half(s.substr(0, s.size() / 2)); SeededKeys D; D.load(half); });
        thrown("load_huge_count", [&] { string s = file.str().substr(0, 4096); const uint64_t c = 1u << 24; memcpy(&s[48], &c, 8); stringstream big(s); SeededKeys D; D.load(big); });
        thrown("load_other_parameters", [&] { string s = file.str(); s[20] ^= 1; stringstream other(s); SeededKeys D; D.load(other); });
        thrown("load_not_a_key_file", [&] { stringstream junk(string(200, 'x')); SeededKeys D; D.load(junk); });
        thrown("generate_bad_dbc", [&] { generateGaloisKeysSeeded(0, elts); });
        thrown("generate_bad_element", [&] { generateGaloisKeysSeeded(16, {4}); });
        put("seeded_after_refusals_rows_1", rotateRows(x, 1));                      // a refused set leaves the installed one in place
        // WITHOUT the deterministic seed: an element made twice under one master key -- in two sets, on the host and on the device -- is the same key under the
        // same public seed (equal noise around two different masks would give the secret key away); new parameters bring a new master key and a new seed
        clearDeterministicSeed();
        setParameters(n, q, p[2], 0);
        {
            const size_t rw = crc_seeded_key_words(context, 16);
            const SeededKeys R1 = generateGaloisKeysSeeded(16, {3, 5}), R2 = generateGaloisKeysSeeded(16, {9, 3}, true);
            const bool seed_same = !memcmp(R1.seed, R2.seed, 32);
            const bool key_same = R1.rows.size() == 2 * rw && R2.rows.size() == 2 * rw && equal(R1.rows.begin(), R1.rows.begin() + rw, R2.rows.begin() + rw);
            const bool others_differ = !equal(R1.rows.begin(), R1.rows.begin() + rw, R1.rows.begin() + rw) && !equal(R2.rows.begin(), R2.rows.begin() + rw, R2.rows.begin() + rw);
            printf("repeat seed %s element %s others %s\n", seed_same ? "equal" : "differs", key_same ? "equal" : "differs", others_differ ? "differ" : "equal");
            setParameters(n, q, p[2], 0);
            const SeededKeys R3 = generateGaloisKeysSeeded(16, {3});
            printf("fresh seed %s element %s\n", memcmp(R1.seed, R3.seed, 32) ? "differs" : "equal",
                   equal(R1.rows.begin(), R1.rows.begin() + rw, R3.rows.begin()) ? "equal" : "differs");
        }
        delParameters();
        printf("seeded_keys_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "seeded_keys_host: %s\n", e.what()); return 4; }
}
