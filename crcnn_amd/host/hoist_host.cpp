// hoist_host -- rotateRowsMany / matvecSlots of the host classes on slot-encrypted vectors (tests/test_gpu_hoist_cpp.py).
//
//   hoist_host <dir>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/values.i64 = [n][P] int64: slot j of ciphertext c holds values[j][c] (the test tiles a vector of 8 entries
// with period 8), <dir>/w8.i64 = [8][8] and <dir>/w5.i64 = [5][8] int64 matrices.  Keys: 3^d for d = 1..7.
// Writes <dir>/<name>.i64 = [n][P] (decrypted and decomposed) for name in many_0, many_1, many_5, many_7 (one rotateRowsMany call), many_5_ntt (NTT form in and
// out), rows_1 and rows_5 (rotateRows, for the budget comparison), matvec_8x8, matvec_5x8, matvec_8x8_ntt, matvec_zero; prints "budget <name> <min bits>" per
// result, "throws <case> <exception kind>" for the exceptions and "hoist_host ok" at the end.
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
static vector<vector<int64_t>> matrix(const string &p, int rows, int cols)
{
    const auto raw = rd(p);
    vector<vector<int64_t>> W(rows, vector<int64_t>(cols));
    for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) W[i][j] = (int64_t)raw[(size_t)i * cols + j];
    return W;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: hoist_host <dir>\n"); return 1; }
    try {
        dir = argv[1];
        setDeterministicSeed(20241019);
        const auto p = rd(dir + "/params.u64");
        n = (int)p[0]; const int k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        const vector<vector<int64_t>> W8 = matrix(dir + "/w8.i64", 8, 8), W5 = matrix(dir + "/w5.i64", 5, 8);
        // a plain modulus without slots: the reference's logic_error, before any key is looked at
        setParameters(n, q, (uint64_t)1 << 20, 0);
        {
            ciphertext3D none(1, 1, 1, 1);
            thrown("no_batching_many", [&] { rotateRowsMany(none, {1}); });
            thrown("no_batching_matvec", [&] { matvecSlots(none, W8, 8); });
        }
        setParameters(n, q, p[2], 0);
        setSlotEncoding(0, 0);
        const auto raw = rd(dir + "/values.i64");
        const size_t P = raw.size() / n;
        vector<vector<int64_t>> images(n, vector<int64_t>(P));
        for (int j = 0; j < n; j++) for (size_t c = 0; c < P; c++) images[j][c] = (int64_t)raw[(size_t)j * P + c];
        const ciphertext3D x = encryptImageSlots(images, 1, 1, (int)P);
        thrown("no_keys_many", [&] { rotateRowsMany(x, {1}); });
        thrown("no_keys_matvec", [&] { matvecSlots(x, W8, 8); });
        vector<uint64_t> elts;
        for (int d = 1; d < 8; d++) elts.push_back(crc_galois_elt_rows(context, d));
        generateGaloisKeys(16, elts);
        put("fresh", x);
        {
            const vector<ciphertext3D> r = rotateRowsMany(x, {0, 1, 5, 7});
            put("many_0", r[0]); put("many_1", r[1]); put("many_5", r[2]); put("many_7", r[3]);
        }
        { ciphertext3D xn = rotateRowsMany(x, {0}, CRC_NTT)[0]; put("many_5_ntt", rotateRowsMany(xn, {5}, CRC_NTT)[0]); }
        put("rows_1", rotateRows(x, 1));
        put("rows_5", rotateRows(x, 5));
        put("matvec_8x8", matvecSlots(x, W8, 8));
        put("matvec_5x8", matvecSlots(x, W5, 8));
        { ciphertext3D xn = rotateRowsMany(x, {0}, CRC_NTT)[0]; put("matvec_8x8_ntt", matvecSlots(xn, W8, 8, CRC_NTT)); }
        put("matvec_zero", matvecSlots(x, vector<vector<int64_t>>(8, vector<int64_t>(8, 0)), 8));
        printf("empty %zu\n", rotateRowsMany(x, {}).size());
        thrown("steps_too_large", [&] { rotateRowsMany(x, {1, n / 2}); });
        thrown("missing_key_many", [&] { rotateRowsMany(x, {1, 9}); });                 // 3^9 has no key of its own: no chain is planned
        thrown("bad_M", [&] { matvecSlots(x, W8, 6); });
        thrown("M_too_large", [&] { matvecSlots(x, W8, n); });
        thrown("W_too_large", [&] { matvecSlots(x, W8, 4); });
        {
            vector<vector<int64_t>> W16(16, vector<int64_t>(16, 0));
            W16[0][9] = 1;                                                              // diagonal 9: the key of 3^9 is absent
            thrown("missing_key_matvec", [&] { matvecSlots(x, W16, 16); });
        }
        thrown("bad_form", [&] { rotateRowsMany(x, {1}, CRC_NTTP); });
        delParameters();
        clearDeterministicSeed();
        printf("hoist_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "hoist_host: %s\n", e.what()); return 4; }
}
