// seeded_host -- driver of the device encryptor of the seeded form behind the host classes (encryptImageSeeded(..., on_device = true)).
//   seeded_host roundtrip <n> <t>                    host path against device path byte for byte, then through save / load / expandSeeded / decryptImages
//   seeded_host time <n> <t> <images> <rounds>       wall clock of the whole client call per 28 x 28 image, host path and device path alternating; one JSON line
#include "crcnn_host.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

using namespace std;
typedef uint64_t u64;

static floatCube cubeOf(const vector<float> &px, int b, int zd, int xd, int yd)
{
    const size_t per = (size_t)zd * xd * yd;
    floatCube img(zd, vector<vector<float>>(xd, vector<float>(yd)));
    for (int z = 0; z < zd; z++) for (int i = 0; i < xd; i++) for (int j = 0; j < yd; j++) img[z][i][j] = px[(size_t)b * per + ((size_t)z * xd + i) * yd + j];
    return img;
}

// save -> load -> expandSeeded in both forms -> decryptImages against `want` (the floats encryptImage's ciphertexts of the same pixels decrypt to)
static int checkDecrypts(const SeededImages &made, const vector<floatCube> &want, const char *what)
{
    const size_t n = (size_t)crc_ctx_n(context), k = (size_t)crc_ctx_k(context);
    stringstream file;
    made.save(file);
    SeededImages im;
    im.load(file);
    if (im.c0 != made.c0 || memcmp(im.seed, made.seed, 32) || im.stream_base != made.stream_base) { fprintf(stderr, "%s: save -> load is not the identity\n", what); return 4; }
    ciphertext3D a = expandSeeded(im, CRC_COEFF), an = expandSeeded(im, CRC_NTT);
    const vector<u64> ha = a.toHost(), hn = an.toHost();
    for (size_t m = 0; m < im.count(); m++)
        if (memcmp(hn.data() + m * 2 * k * n, im.c0.data() + m * k * n, k * n * 8)) { fprintf(stderr, "%s: the NTT-form c0 is not the row that travelled\n", what); return 5; }
    vector<u64> back(hn.size());
    { DeviceBuffer d(hn.size() * 8);
      if (crc_memcpy_h2d(context, d.ptr, hn.data(), hn.size() * 8, nullptr) || crc_ntt_inv(context, (uint64_t *)d.ptr, a.count(), 2, nullptr) ||
          crc_memcpy_d2h(context, back.data(), d.ptr, hn.size() * 8, nullptr) || crc_stream_sync(context, nullptr)) return 3; }
    if (back != ha) { fprintf(stderr, "%s: the coefficient form is not the inverse transform of the NTT form\n", what); return 5; }
    if (decryptImages(a) != want) { fprintf(stderr, "%s: floats differ from encryptImage's\n", what); return 6; }
    return 0;
}

static int do_roundtrip(int argc, char **argv)
{
    if (argc < 4) return 1;
    const int n = atoi(argv[2]); const u64 t = strtoull(argv[3], 0, 0);
    const int B = 2, zd = 2, xd = 5, yd = 4, per = zd * xd * yd;
    vector<float> px((size_t)B * per);
    for (size_t i = 0; i < px.size(); i++) px[i] = (float)((int)((i * 37) % 201) - 100) / 16.0f;
    const u64 det = 99;
    setDeterministicSeed(det);
    setParameters(n, t);
    const SeededImages host = encryptImageSeeded(px, zd, xd, yd);
    vector<floatCube> want;
    for (int b = 0; b < B; b++) want.push_back(decryptImage(encryptImage(cubeOf(px, b, zd, xd, yd))));
    setDeterministicSeed(det);
    setParameters(n, t);                                    // the same keys, the ciphertext counter back at 0
    const SeededImages dev = encryptImageSeeded(px, zd, xd, yd, true);
    if (dev.B != B || dev.zd != zd || dev.xd != xd || dev.yd != yd || dev.c0.size() != host.c0.size()) { fprintf(stderr, "device path: wrong shape\n"); return 4; }
    if (memcmp(dev.seed, host.seed, 32) || dev.stream_base != host.stream_base) { fprintf(stderr, "device path: seed or stream base differ from the host path's\n"); return 4; }
    if (dev.c0 != host.c0) {
        size_t w = 0; while (dev.c0[w] == host.c0[w]) w++;
        fprintf(stderr, "device path: c0 differs from the host path's at word %zu\n", w); return 5;
    }
    // the private key of a deterministic call is the expansion of its 64-bit seed (crc_seeded_public_seed of the complement): never the public seed
    uint8_t priv[32];
    if (crc_seeded_public_seed(~(det + 1000003), priv)) return 3;
    if (!memcmp(priv, dev.seed, 32)) { fprintf(stderr, "device path: the public seed is the private key\n"); return 4; }
    int rc;
    if ((rc = checkDecrypts(host, want, "host path"))) return rc;
    if ((rc = checkDecrypts(dev, want, "device path"))) return rc;
    // OS entropy: another public seed per call, the same floats.  The private key in use (the master key of setParameters) is not visible from here: that the seed
    // differs from IT is what crc_encrypt_f32_seeded_dev_key's own refusal of byte-equal arguments guarantees -- the calls below succeed.  What can be compared is
    // compared: the seeds of the two calls, the deterministic call's seed and that call's private key
    clearDeterministicSeed();
    setParameters(n, t);
    want.clear();
    for (int b = 0; b < B; b++) want.push_back(decryptImage(encryptImage(cubeOf(px, b, zd, xd, yd))));
    const u64 base0 = (u64)B * per;                         // encryptImage took one keystream id per ciphertext
    const SeededImages r1 = encryptImageSeeded(px, zd, xd, yd, true), r2 = encryptImageSeeded(px, zd, xd, yd, true);
    if (!memcmp(r1.seed, dev.seed, 32) || !memcmp(r1.seed, priv, 32) || !memcmp(r1.seed, r2.seed, 32)) { fprintf(stderr, "OS-entropy mode: a public seed was reused\n"); return 4; }
    if (r1.stream_base != base0 || r2.stream_base != base0 + r1.count()) { fprintf(stderr, "OS-entropy mode: the stream base did not move on\n"); return 4; }
    if (r1.c0 == dev.c0 || r1.c0 == r2.c0) { fprintf(stderr, "OS-entropy mode: two calls reused their randomness\n"); return 4; }
    if ((rc = checkDecrypts(r1, want, "device path, OS entropy"))) return rc;
    if ((rc = checkDecrypts(r2, want, "device path, OS entropy, second call"))) return rc;
    delParameters();
    printf("seeded_host ok\n");
    return 0;
}

static int do_time(int argc, char **argv)
{
    if (argc < 6) return 1;
    const int n = atoi(argv[2]); const u64 t = strtoull(argv[3], 0, 0);
    const int images = atoi(argv[4]), rounds = atoi(argv[5]);
    if (images < 1 || rounds < 1) return 1;
    const int xd = 28, yd = 28;
    vector<float> px((size_t)images * xd * yd);
    for (size_t i = 0; i < px.size(); i++) px[i] = (float)((int)((i * 37) % 201) - 30) / 60.0f;
    setDeterministicSeed(7);
    setParameters(n, t);
    (void)encryptImageSeeded(px, 1, xd, yd, true);           // the device copy of the secret key, first launches
    vector<double> ms[2];
    for (int r = 0; r < rounds; r++)
        for (int dev = 0; dev < 2; dev++) {
            const auto t0 = chrono::steady_clock::now();
            const SeededImages im = encryptImageSeeded(px, 1, xd, yd, dev == 1);
            const auto t1 = chrono::steady_clock::now();
            if (im.c0.empty()) return 3;
            ms[dev].push_back(chrono::duration<double, milli>(t1 - t0).count() / images);
        }
    printf("{\"n\": %d, \"k\": %d, \"images\": %d, \"unit\": \"ms per 28x28 image, whole encryptImageSeeded call\"", n, crc_ctx_k(context), images);
    for (int dev = 0; dev < 2; dev++) {
        vector<double> s(ms[dev]); sort(s.begin(), s.end());
        printf(", \"%s\": {\"rounds\": [", dev ? "device" : "host");
        for (size_t i = 0; i < ms[dev].size(); i++) printf("%s%.4f", i ? ", " : "", ms[dev][i]);
        printf("], \"median\": %.4f, \"max_minus_min\": %.4f}", s[s.size() / 2], s.back() - s.front());
    }
    printf("}\n");
    delParameters();
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 1;
    try {
        if (!strcmp(argv[1], "roundtrip")) return do_roundtrip(argc, argv);
        if (!strcmp(argv[1], "time")) return do_time(argc, argv);
    } catch (const exception &e) { fprintf(stderr, "exception: %s\n", e.what()); return 10; }
    return 1;
}
