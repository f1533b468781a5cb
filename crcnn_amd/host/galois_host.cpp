// galois_host -- rotateRows / rotateColumns / sumSlots of the host classes on a slot-encrypted batch (tests/test_gpu_galois_cpp.py).
//
//   galois_host <dir>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/values.i64 = [n][P] int64: n images of P pixels, image j in slot j of each of the P ciphertexts.
// Writes <dir>/<name>.i64 = [n][P] (decrypted and decomposed) for name in rows_1, rows_m1, rows_5, rows_last (n/2 - 1 steps), cols, rows_5_cols_ntt (through NTT
// form), sum, and a custom key set's rows_3; prints "budget <name> <min bits>" per result, "throws <case> <exception kind>" for the reference's exceptions and
// "galois_host ok" at the end.
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
static void put(const char *name, const ciphertext3D &t)
{
    printf("budget %s %d\n", name, minNoiseBudget(t));
    const vector<vector<int64_t>> v = decryptSlots(t, n);
    ofstream f(dir + "/" + name + ".i64", ios::binary);
    for (auto &row : v) f.write((const char *)row.data(), row.size() * 8);
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
    if (argc < 2) { fprintf(stderr, "usage: galois_host <dir>\n"); return 1; }
    try {
        dir = argv[1];
        setDeterministicSeed(20240923);
        const auto p = rd(dir + "/params.u64");
        n = (int)p[0]; const int k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        // a plain modulus without slots: the reference's logic_error, before any key is looked at
        setParameters(n, q, (uint64_t)1 << 20, 0);
        {
            ciphertext3D none(1, 1, 1, 1);
            thrown("no_batching_rows", [&] { rotateRows(none, 1); });
            thrown("no_batching_columns", [&] { rotateColumns(none); });
            thrown("no_batching_sum", [&] { sumSlots(none); });
        }
        setParameters(n, q, p[2], 0);
        setSlotEncoding(0, 0);
        const auto raw = rd(dir + "/values.i64");
        const size_t P = raw.size() / n;
        vector<vector<int64_t>> images(n, vector<int64_t>(P));
        for (int j = 0; j < n; j++) for (size_t c = 0; c < P; c++) images[j][c] = (int64_t)raw[(size_t)j * P + c];
        const ciphertext3D x = encryptImageSlots(images, 1, 1, (int)P);
        thrown("no_keys", [&] { rotateRows(x, 1); });
        generateGaloisKeys(16);
        put("fresh", x);
        put("rows_1", rotateRows(x, 1));
        put("rows_m1", rotateRows(x, -1));
        put("rows_5", rotateRows(x, 5));
        put("rows_last", rotateRows(x, n / 2 - 1));
        put("cols", rotateColumns(x));
        { ciphertext3D r = rotateRows(x, 5, CRC_NTT); put("rows_5_cols_ntt", rotateColumns(r, CRC_NTT)); }
        put("sum", sumSlots(x));
        put("rows_0", rotateRows(x, 0));
        thrown("steps_too_large", [&] { rotateRows(x, n / 2); });
        thrown("steps_too_large_negative", [&] { rotateRows(x, -(n / 2)); });
        thrown("bad_dbc", [&] { generateGaloisKeys(61); });
        thrown("bad_element", [&] { generateGaloisKeys(16, {2}); });
        // a set of the caller's: the key of 27 = 3^3 alone serves rotateRows(3) in ONE step and nothing else
        generateGaloisKeys(8, {27});
        put("rows_3", rotateRows(x, 3));
        thrown("missing_key_rows", [&] { rotateRows(x, 1); });
        thrown("missing_key_columns", [&] { rotateColumns(x); });
        thrown("missing_key_sum", [&] { sumSlots(x); });
        delParameters();
        clearDeterministicSeed();
        printf("galois_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "galois_host: %s\n", e.what()); return 4; }
}
