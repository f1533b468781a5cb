// flood_host -- floodImages / floodBits / sanitizeResponse / Network::flood_bits of the host classes (tests/test_gpu_flood_cpp.py).
//
//   flood_host <dir> [<model.h5>]
//
// <dir>/params.u64 = (n, k, t, q_0 .. q_{k-1}, a-priori budget of a fresh encryption at the full modulus, the same at the level of k - 1, a-priori budget of the
// network's output), <dir>/image.f32 = 16 float32 pixels of one 4 x 4 image.  Prints "bits <name> <flood width>", "budget <name> <min bits>",
// "equal <name> <0|1>", "throws <case> <exception kind>", "digest <name> <fnv-1a of the tensor's words>" and "flood_host ok" at the end.  With a model file:
// PlainModelTiny on two seeded synthetic images at (4096, 2, t = 2^20), once as it is and once with Network::flood_bits.
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
static unsigned long long digest(const vector<uint64_t> &w)
{
    unsigned long long h = 1469598103934665603ULL;
    for (uint64_t v : w) for (int b = 0; b < 8; b++) { h ^= (v >> (8 * b)) & 0xff; h *= 1099511628211ULL; }
    return h;
}
static uint64_t splitmix(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// budget_host's synthetic image: 81 % background, the rest uniform in 1..255, normalised
static vector<float> synthImage(int index)
{
    uint64_t s = 0xC0FFEEULL + (uint64_t)index;
    vector<float> px(784);
    for (int i = 0; i < 784; i++) {
        const uint64_t z = splitmix(s);
        const int v = (z & 0xFFFF) >= (uint64_t)(0.81 * 65536) ? 1 + (int)((z >> 16) % 255) : 0;
        px[i] = ((float)v / 255.0f - 0.1307f) / 0.3081f;
    }
    return px;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: flood_host <dir> [<model.h5>]\n"); return 1; }
    try {
        const string dir = argv[1];
        setDeterministicSeed(20261021);
        const auto p = rd<uint64_t>(dir + "/params.u64");
        const int n = (int)p[0], k = (int)p[1];
        const vector<uint64_t> q(p.begin() + 3, p.begin() + 3 + k);
        const int b_full = (int)p[3 + k], b_level = (int)p[4 + k], b_net = (int)p[5 + k];
        const vector<float> px = rd<float>(dir + "/image.f32");
        setParameters(n, q, p[2], 0);
        shared_ptr<Level> L = makeLevel(k - 1);
        const int B = floodBits(b_full), BL = crc_flood_bits(L->ctx, b_level, 40);
        printf("bits full %d\nbits level %d\n", B, BL);
        thrown("flood_bits_impossible", [&] { floodBits(0, 126); });
        {
            ciphertext3D x = encryptImage(px, 1, 4, 4);
            LevelTensor xl = modSwitch(x, L, CRC_NTT);
            const vector<float> before = flat(decryptImages(x));
            printf("budget full %d\nbudget level %d\n", minNoiseBudget(x), minNoiseBudget(xl));
            thrown("flood_width_0", [&] { floodImages(x, 0); });
            thrown("flood_width_127", [&] { floodImages(x, 127); });
            printf("equal refusals_wrote_nothing %d\n", (int)(flat(decryptImages(x)) == before));
            LevelTensor xlc = modSwitch(x, L, CRC_COEFF);               // (before x is flooded: the same unflooded image at the level, coefficient form)
            const vector<uint64_t> h = x.toHost();
            floodImages(x, B);
            printf("budget full_flooded %d\n", minNoiseBudget(x));
            printf("equal decrypt_full %d\nequal flood_changed_full %d\n", (int)(flat(decryptImages(x)) == before && before.size() == px.size()), (int)(x.toHost() != h));
            // a LevelTensor in each form, under the level's public-key rows and context: the coefficient-form one decrypts as before (decryptImages takes
            // that form); the NTT-resident one is flooded as it stands and its budget is measured as it stands
            const vector<uint64_t> hl = xl.toHost(), hlc = xlc.toHost();
            floodImages(xlc, BL);
            printf("budget level_flooded %d\n", minNoiseBudget(xlc));
            printf("equal decrypt_level %d\nequal flood_changed_level %d\n", (int)(flat(decryptImages(xlc)) == before), (int)(xlc.toHost() != hlc));
            floodImages(xl, BL);
            printf("budget level_flooded_ntt %d\nequal flood_changed_level_ntt %d\n", minNoiseBudget(xl), (int)(xl.toHost() != hl));
            const LevelTensor xc = modSwitch(x, L);                     // the flooded full tensor, switched: what sanitizeResponse returns
            printf("equal decrypt_switched %d\n", (int)(flat(decryptImages(xc)) == before));
            thrown("flood_level_width", [&] { floodImages(xl, 127); });
        }
        // sanitizeResponse = flood, then modSwitch: the same parameters and the same keystream counter twice under the deterministic seed
        vector<uint64_t> a, b;
        bool untouched = false;
        {
            setParameters(n, q, p[2], 0); L = makeLevel(k - 1);
            const ciphertext3D x = encryptImage(px, 1, 4, 4);
            const vector<uint64_t> h = x.toHost();
            a = sanitizeResponse(x, B, L).toHost();
            untouched = x.toHost() == h;
        }
        {
            setParameters(n, q, p[2], 0); L = makeLevel(k - 1);
            ciphertext3D x = encryptImage(px, 1, 4, 4);
            floodImages(x, B);
            b = modSwitch(x, L).toHost();
        }
        printf("equal sanitize_is_flood_then_switch %d\nequal sanitize_leaves_its_input %d\n", (int)(a == b && !a.empty()), (int)untouched);
        thrown("sanitize_no_level", [&] { const ciphertext3D x = encryptImage(px, 1, 4, 4); sanitizeResponse(x, B, nullptr); });

        if (argc > 2) {
            uint64_t q2[16];
            if (crc_default_coeff_modulus_128(4096, q2, 16) < 2) throw invalid_argument("coeff_modulus_128(4096)");
            setParameters(4096, vector<uint64_t>(q2, q2 + 2), 1 << 20, 0);
            CnnBuilder build(argv[2]);
            Network net = build.buildNetworkByName("PlainModelTiny");
            vector<ciphertext3D> imgs;
            for (int i = 0; i < 2; i++) imgs.push_back(encryptImage(synthImage(i), 1, 28, 28));
            const ciphertext3D x = stackImages(imgs);
            const ciphertext3D out0 = net.forward(x);
            const vector<int> launches0 = net.last_layer_launches;
            const vector<float> logits0 = flat(decryptImages(out0));
            const unsigned long long d0 = digest(out0.toHost());
            printf("digest plain %llu\nbudget net %d\n", d0, minNoiseBudget(out0));
            net.flood_bits = floodBits(b_net);
            printf("bits net %d\n", net.flood_bits);
            const ciphertext3D out1 = net.forward(x);
            printf("budget net_flooded %d\n", minNoiseBudget(out1));
            printf("equal logits %d\nequal flood_changed_net %d\n", (int)(flat(decryptImages(out1)) == logits0 && logits0.size() == 20), (int)(digest(out1.toHost()) != d0));
            net.flood_bits = 0;
            const ciphertext3D out2 = net.forward(x);
            printf("digest plain_again %llu\nequal launches %d\n", digest(out2.toHost()), (int)(net.last_layer_launches == launches0));
            net.flood_bits = 127;
            thrown("net_bad_width", [&] { net.forward(x); });
        }
        delParameters();
        clearDeterministicSeed();
        printf("flood_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "flood_host: %s\n", e.what()); return 4; }
}
