// modswitch_host -- makeLevel / modSwitch / LevelTensor of the host classes on one encrypted image (tests/test_gpu_mod_switch_cpp.py).
//
//   modswitch_host <dir>
//
// <dir>/params.u64 (n, k, t, q..., then a slot prime t'), <dir>/image.f32 = [xd * yd] float32 pixels of one xd x yd image (xd = yd = 4).
// The image is encrypted under all k moduli and switched to the level of k - 1.  Writes <dir>/full.f32 and <dir>/level.f32 (decryptImages of the two tensors),
// <dir>/level.ct (LevelTensor::save); prints "budget <name> <min bits>", "bytes <name> <n>", "equal <name> <0|1>", "throws <case> <exception kind>" and
// "modswitch_host ok" at the end.
#include "crcnn_host.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
using namespace std;

template <class T> static vector<T> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<T> v(sz / sizeof(T)); f.read((char *)v.data(), sz); return v;
}
static void thrown(const char *name, const function<void()> &call)
{
    const char *kind = "nothing";
    try { call(); } catch (const invalid_argument &) { kind = "invalid_argument"; } catch (const logic_error &) { kind = "logic_error"; }
    catch (const exception &) { kind = "exception"; }
    printf("throws %s %s\n", name, kind);
}
static vector<float> flat(const vector<floatCube> &v)
{
    vector<float> out;
    for (auto &im : v) for (auto &z : im) for (auto &x : z) for (float y : x) out.push_back(y);
    return out;
}
static void put(const string &path, const vector<float> &v) { ofstream f(path, ios::binary); f.write((const char *)v.data(), v.size() * 4); }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: modswitch_host <dir>\n"); return 1; }
    try {
        const string dir = argv[1];
        setDeterministicSeed(20241020);
        const auto p = rd<uint64_t>(dir + "/params.u64");
        const int n = (int)p[0], k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        const uint64_t slot_t = p[3 + k];
        const vector<float> px = rd<float>(dir + "/image.f32");
        thrown("level_before_parameters", [&] { makeLevel(1); });
        setParameters(n, q, p[2], 0);
        thrown("level_0", [&] { makeLevel(0); });
        thrown("level_k", [&] { makeLevel(k); });
        shared_ptr<Level> L = makeLevel(k - 1);
        const ciphertext3D x = encryptImage(px, 1, 4, 4);
        const LevelTensor y = modSwitch(x, L);
        printf("budget full %d\nbudget level %d\n", minNoiseBudget(x), minNoiseBudget(y));
        {
            const vector<int> all = noiseBudgets(y); size_t at = 0;
            const int mn = minNoiseBudget(y, &at);
            bool ok = all.size() == y.count() && at < all.size() && all[at] == mn;
            for (int b : all) ok = ok && b >= mn;
            printf("equal budgets_and_min %d\n", (int)ok);
            const LevelTensor yn = modSwitch(x, L, CRC_NTT);           // an NTT-resident tensor is measured as it stands
            printf("equal budgets_ntt %d\n", (int)(noiseBudgets(yn) == all));
            thrown("save_ntt", [&] { yn.save(dir + "/never.ct"); });
            thrown("decrypt_ntt", [&] { decryptImages(yn); });
        }
        const vector<float> full = flat(decryptImages(x)), low = flat(decryptImages(y));
        put(dir + "/full.f32", full); put(dir + "/level.f32", low);
        printf("equal decrypt %d\n", (int)(full == low && full.size() == px.size()));
        y.save(dir + "/level.ct");
        printf("bytes level_ct %zu\nbytes expected %zu\nbytes full_ct %zu\n", rd<char>(dir + "/level.ct").size(), y.count() * crc_seal_ct_bytes(L->ctx, 2),
               y.count() * crc_seal_ct_bytes(context, 2));
        const LevelTensor z = LevelTensor::load(L, 1, 1, 4, 4, dir + "/level.ct");
        printf("equal load %d\n", (int)(z.toHost() == y.toHost() && flat(decryptImages(z)) == low));
        encryptAndSaveImage(px, 1, 4, 4, dir + "/full.ct");
        thrown("load_full_file_at_level", [&] { LevelTensor::load(L, 1, 1, 4, 4, dir + "/full.ct"); });
        thrown("load_more_than_the_file", [&] { LevelTensor::load(L, 2, 1, 4, 4, dir + "/level.ct"); });
        thrown("load_less_than_the_file", [&] { LevelTensor::load(L, 1, 1, 4, 2, dir + "/level.ct"); });
        thrown("switch_to_no_level", [&] { modSwitch(x, nullptr); });
        thrown("switch_bad_form", [&] { modSwitch(x, L, CRC_NTTP); });
        thrown("slots_without_batching", [&] { decryptSlots(y, 1); });
        // slot encoding: the slots of a switched tensor are those of the tensor
        setParameters(n, q, slot_t, 0);
        // the level of the parameters before: refused wherever it turns up
        thrown("stale_level_switch", [&] { const ciphertext3D e = encryptImage(px, 1, 4, 4); modSwitch(e, L); });
        thrown("stale_level_decrypt", [&] { decryptImages(y); });
        thrown("stale_level_budget", [&] { minNoiseBudget(y); });
        thrown("stale_level_load", [&] { LevelTensor::load(L, 1, 1, 4, 4, dir + "/level.ct"); });
        setSlotEncoding(0, 0);
        L = makeLevel(k - 1);
        vector<vector<int64_t>> images(5, vector<int64_t>(16));
        for (int j = 0; j < 5; j++) for (int c = 0; c < 16; c++) images[j][c] = (int64_t)((j * 16 + c) * 37 % 1001) - 500;
        const ciphertext3D s = encryptImageSlots(images, 1, 4, 4);
        const LevelTensor sl = modSwitch(s, L, CRC_NTT);
        printf("budget slots_full %d\nbudget slots_level %d\n", minNoiseBudget(s), minNoiseBudget(sl));
        const vector<vector<int64_t>> a = decryptSlots(s, 5), b = decryptSlots(sl, 5);
        bool same = a == b && a.size() == 5;
        for (int j = 0; j < 5 && same; j++) same = a[j] == images[j];
        printf("equal slots %d\n", (int)same);
        delParameters();
        thrown("stale_level_after_del", [&] { decryptSlots(sl, 5); });
        clearDeterministicSeed();
        printf("modswitch_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "modswitch_host: %s\n", e.what()); return 4; }
}
