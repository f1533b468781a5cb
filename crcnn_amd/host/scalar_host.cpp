// scalar_host -- slot-batched inference with the scalar limb form (CRC_NTTLS) switched off and on (tests/test_gpu_scalar_net.py).
//
//   scalar_host <description> <h5> <dir> <S> <input_bits> <weight_bits>
//
// <dir>/params.u64 (n, k, t, q...: t a slot prime), <dir>/images.f32 = [S][zd xd yd] float32 pixels, as test_host slots_build takes them.  The S images are
// encrypted into ONE tensor, once; then for the tuning key scalar_mac = 0 and 1, unfused and after Network::fuse(), a freshly built network runs
// Network::forward on it.  Per run <dir>/slots_<key>_<fused>.i64 = [S][outputs] int64 (decrypted and decomposed) and on stdout
//   run <key> <fused> digest <FNV-1a of the output ciphertexts>
//   mac <key> <fused> <layer index> <zd> <xd> <yd> <xs> <ys> <xf> <yf> <nf> <deviceBytes> <kernelName>
// and "scalar_host ok" at the end.
#include "crcnn_host.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
using namespace std;

static vector<uint64_t> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<uint64_t> v(sz / 8); f.read((char *)v.data(), sz); return v;
}

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: scalar_host <description> <h5> <dir> <S> <input_bits> <weight_bits>\n"); return 1; }
    try {
        const string desc = argv[1], h5 = argv[2], dir = argv[3]; const int S = atoi(argv[4]), in_bits = atoi(argv[5]), w_bits = atoi(argv[6]);
        setDeterministicSeed(20240611);
        { auto p = rd(dir + "/params.u64"); const int n = (int)p[0], k = (int)p[1];
          setParameters(n, vector<uint64_t>(p.begin() + 3, p.begin() + 3 + k), p[2], 0); }
        setSlotEncoding(in_bits, w_bits);
        ciphertext3D in;
        for (int key = 0; key < 2; key++) for (int fused = 0; fused < 2; fused++) {
            // the key is read when a layer plans its kernel: set before the network is built, the weights are packed at its first forward
            if (crc_ctx_set_tuning(context, "scalar_mac", key) != CRC_OK) { fprintf(stderr, "no tuning key scalar_mac\n"); return 3; }
            CnnBuilder builder(h5);
            Network net = builder.buildNetworkFromDescription(desc);
            if (!in.buf) {
                const size_t px = (size_t)net.input_zd * net.input_xd * net.input_yd;
                vector<vector<float>> images(S, vector<float>(px));
                ifstream f(dir + "/images.f32", ios::binary);
                for (auto &im : images) f.read((char *)im.data(), px * 4);
                if (!f) { fprintf(stderr, "images.f32 is missing or too short\n"); return 2; }
                in = encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd);
            }
            net.ntt_resident = true;
            if (fused) net.fuse();
            const ciphertext3D out = net.forward(in);
            const vector<vector<int64_t>> v = decryptSlots(out, S);
            { ofstream f(dir + "/slots_" + to_string(key) + "_" + to_string(fused) + ".i64", ios::binary);
              for (auto &row : v) f.write((const char *)row.data(), row.size() * 8); }
            uint64_t h = 0xcbf29ce484222325ULL;
            for (uint64_t w : out.toHost()) for (int b = 0; b < 8; b++) { h ^= (w >> (8 * b)) & 0xff; h *= 0x100000001b3ULL; }
            printf("run %d %d digest %016llx\n", key, fused, (unsigned long long)h);
            for (int i = 0; i < net.getNumLayers(); i++)
                if (auto m = dynamic_pointer_cast<MacLayer>(net.getLayer(i)))
                    printf("mac %d %d %d %d %d %d %d %d %d %d %d %zu %s\n", key, fused, i, m->zd, m->xd, m->yd, m->xs, m->ys, m->xf, m->yf, m->nf, m->deviceBytes(),
                           m->kernelName().c_str());
        }
        in = ciphertext3D();
        delParameters();
        clearDeterministicSeed();
        printf("scalar_host ok\n");
        return 0;
    } catch (const exception &e) { fprintf(stderr, "scalar_host: %s\n", e.what()); return 4; }
}
