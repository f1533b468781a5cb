// test_host.cpp -- driver for the C++ host classes, run by tests/test_gpu_host_cpp.py on the GPU box.
//   test_host net <model> <h5> <dir> <resident 0|1> <batch> [fuse 0|1]      (fuse: Network::fuse() before the resident forward)
//     <dir>/params.u64 (n,k,t,q...), evk.u64, net_in.u64 ([1][1][28][28][2][k][n]) -> writes layer_<i>.u64 (layerwise mode) and out.u64
//     <model>: a built-in name or the path of a description file, here and in net3 / netr / netseeded / search (netr: a <layer_before_reenc> of -1 keeps the
//     description's refresh point)
//   test_host netgeom <model> <h5> <dir> <batch> <head_chunk>     `net` with Network::fuse(), NTT-resident, on <batch> copies of the image (out.u64); prints one line
//     "geom <i> <name> <zd> <xd> <yd> <xs> <ys> <xf> <yf> <nf>" per conv / dense layer the fused network runs
//   test_host describe <name | description file> [h5]     parse and validate a description (with h5: dataset sizes too); prints its canonical form.  No GPU work
//   test_host labels <model> <h5> <images.f32>     argmax of plainModelForward per image ("label <i> <class>").  No GPU work
//   test_host build <description> <h5> <dir> <batch>     see do_build
//   test_host multiply <dir> <count>     multiplyRelin on <dir>/mul_x.u64, mul_y.u64 ([count] ciphertexts each, coefficient form; params.u64, evk.u64):
//     writes mul_cc.u64 (coefficient form in and out) and mul_nn.u64 (both tensors NTT-resident, result NTT-resident, transformed back by the caller)
//   test_host api <h5> <dir>     exercises save/load of the encoded model, client-side encrypt/decrypt, and error behaviour
//   test_host files <dir>        CrCNN's own files: loads the encoded-model stream and the cipher_image file the REFERENCE wrote (<dir>/ref_encoded_layers.bin,
//     ref_cipher_image.bin; cnnBuilder.cpp:181-196, globals.cpp:174-205), runs conv -> bn -> dense on them (out_from_ref_files.u64), then writes the same two
//     files itself (our_encoded_layers.bin, our_cipher_image.bin) and runs those (out_from_our_files.u64)
//   test_host seeded <n> <t> / netseeded <model> <h5> <dir>     seeded secret-key images through the host classes (see do_seeded / do_netseeded)
//   test_host slots_describe <description> <input_bits> <weight_bits>     the scale ledger of slot encoding: "scale <i> <kind> <name> <sigma>" in front of every
//     layer, then "slot_scale <sigma>".  No GPU work
//   test_host slots_build <description> <h5> <dir> <S> <input_bits> <weight_bits> [reps]     see do_slots_build
//   test_host slots_rescale_plan <description> <h5> <dir> <S> <input_bits> <weight_bits>     see do_slots_rescale_plan
//   test_host slots_act_plan <description> <h5> <dir> <S> <input_bits> <weight_bits>         see do_slots_act_plan
//   test_host build_plain <description>                                                      see do_build_plain
//   test_host plain_base <n> <S> <divisor> <cap> <t_0> [<t_1> ...]                           see do_plain_base
//   test_host plan <model> <h5> <dir> <batch> <fuse 0|1> <head_chunk> <matrix_cores 0|1> <layer_before_reenc>     see do_plan
//   test_host searchlogic <min> <max> <first_good> <last_good> <min_q>
//     the plain-modulus search on a synthetic predicate (t < first_good: MISPREDICTED, t > last_good: OUT_OF_BUDGET); no GPU work.
//     prints "found <t>" and one "tried <t> <status>" line per test
//   test_host search <model> <h5> <images.f32> <n> <min> <max> <num_images> <seed> [q0 q1 ...]   (no q: coeff_modulus_128(n))
//     the real search: images.f32 = N x 784 normalised float32 pixels, labels from the float model; prints found / tried lines
#include "crcnn_host.h"
#include "plain_modulus_search.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <sstream>
#include <unistd.h>
#include <cstring>
#include <fstream>
#include <iostream>
using namespace std;
typedef uint64_t u64;

static vector<u64> rd(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<u64> v(sz / 8); f.read((char *)v.data(), sz); return v;
}
static void wr(const string &p, const vector<u64> &v) { ofstream f(p, ios::binary); f.write((const char *)v.data(), v.size() * 8); }

static void setup(const string &dir)
{
    auto p = rd(dir + "/params.u64");
    int n = (int)p[0], k = (int)p[1]; u64 t = p[2];
    setParameters(n, vector<u64>(p.begin() + 3, p.begin() + 3 + k), t, 0);
}

static int do_net(int argc, char **argv)
{
    if (argc < 7) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4]; bool resident = atoi(argv[5]); int batch = atoi(argv[6]);
    setup(dir);
    ifstream evf(dir + "/evk.u64", ios::binary);
    if (evf) {            // use the caller's evaluation keys (ev_keys16 is a public global in the reference as well, globals.h:26)
        auto evk = rd(dir + "/evk.u64");
        ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
        crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr);
    }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    net.ntt_resident = resident;
    if (argc > 7 && atoi(argv[7])) { const int removed = net.fuse(); fprintf(stderr, "fused: %d layers removed, %d left\n", removed, net.getNumLayers()); }
    // two-level chunking: the layers in front of the first dense layer on sub-batches of this many images
    if (argc > 8) net.head_chunk = atoi(argv[8]);
    if (argc > 9) net.matrix_cores = atoi(argv[9]) != 0;
    auto x = rd(dir + "/net_in.u64");
    vector<ciphertext3D> imgs;
    for (int b = 0; b < batch; b++) imgs.push_back(ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd));
    ciphertext3D in = stackImages(imgs);
    if (!resident) {      // layer by layer, coefficient form at every boundary: dump each output for the per-layer digests
        ciphertext3D t = in;
        for (int i = 0; i < net.getNumLayers(); i++) {
            net.getLayer(i)->out_form = CRC_COEFF;
            t = net.getLayer(i)->forward(t);
            wr(dir + "/layer_" + to_string(i) + ".u64", t.toHost());
        }
        wr(dir + "/out.u64", t.toHost());
    } else {
        ciphertext3D out = net.forward(in);
        wr(dir + "/out.u64", out.toHost());
        for (double ms : net.last_layer_ms) fprintf(stderr, "%.3f,", ms);
        fprintf(stderr, "\n");
    }
    delParameters();
    return 0;
}

static int do_netgeom(int argc, char **argv)
{
    if (argc < 7) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4]; const int batch = atoi(argv[5]);
    setup(dir);
    { auto evk = rd(dir + "/evk.u64");
      ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
      crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr); }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    net.ntt_resident = true;
    net.head_chunk = atoi(argv[6]);
    net.fuse();
    for (int i = 0; i < net.getNumLayers(); i++)
        if (auto m = dynamic_pointer_cast<MacLayer>(net.getLayer(i)))
            printf("geom %d %s %d %d %d %d %d %d %d %d\n", i, m->getName().c_str(), m->zd, m->xd, m->yd, m->xs, m->ys, m->xf, m->yf, m->nf);
    auto x = rd(dir + "/net_in.u64");
    vector<ciphertext3D> imgs;
    for (int b = 0; b < batch; b++) imgs.push_back(ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd));
    wr(dir + "/out.u64", net.forward(stackImages(imgs)).toHost());
    // (after the forward: a boxed layer that fell back to its enlarged window says 1 1 here)
    for (int i = 0; i < net.getNumLayers(); i++)
        if (auto m = dynamic_pointer_cast<MacLayer>(net.getLayer(i))) { int bx, by; m->boxSize(bx, by); printf("box %d %s %d %d\n", i, m->getName().c_str(), bx, by); }
    delParameters();
    return 0;
}

// net3 <model> <h5> <dir> <batch>: the three NTT-resident runs of tests/test_gpu_host_cpp.py's full-size cases from ONE built network (the encode + lift + NTT
// of 10^5 .. 10^6 plaintexts is most of a case's time): Network::forward as built (one image), after Network::fuse() (one image), and fused on `batch` images.
// Writes out_unfused.u64, out_fused.u64, out_fused_batch.u64
static int do_net3(int argc, char **argv)
{
    if (argc < 6) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4]; const int batch = atoi(argv[5]);
    setup(dir);
    ifstream evf(dir + "/evk.u64", ios::binary);
    if (evf) {
        auto evk = rd(dir + "/evk.u64");
        ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
        crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr);
    }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    net.ntt_resident = true;
    auto x = rd(dir + "/net_in.u64");
    const ciphertext3D one = ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd);
    // (the unfused run leaves the weights in the matrix-core forms; Network::fuse() rebuilds the canonical ones from the plaintexts before it folds)
    { ciphertext3D out = net.forward(one); wr(dir + "/out_unfused.u64", out.toHost()); }
    const int removed = net.fuse();
    fprintf(stderr, "fused: %d layers removed, %d left\n", removed, net.getNumLayers());
    { ciphertext3D out = net.forward(one); wr(dir + "/out_fused.u64", out.toHost()); }
    vector<ciphertext3D> imgs(batch, one);
    { ciphertext3D out = net.forward(stackImages(imgs)); wr(dir + "/out_fused_batch.u64", out.toHost()); }
    delParameters();
    return 0;
}

// netr <model> <h5> <dir> <batch> <layer_before_reenc> <fuse 0|1> <head_chunk> [sym]: the reference's published configurations -- Network::forward WITH the client-side
// refresh (network.cpp:30-34), now on the device (refreshImages).  <dir> holds params / evk / net_in as for `net` plus sk.u64 and pk.u64 (the client's keys).
// Writes pre_<i>.u64 for the layers in front of the refresh (layer by layer, coefficient form: the reference's digests; unfused runs only), reenc_floats.f32
// (the floats the client saw, per image), dec.u64 ([batch][10][n] decrypted output plaintexts), budget.u64, and prints the per-layer times with T_REENC.
// The optional trailing `sym` (or 1) sets Network::reenc_symmetric: the refresh re-encrypts under the secret key
static int do_netr(int argc, char **argv)
{
    if (argc < 9) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4]; const int batch = atoi(argv[5]); int reenc = atoi(argv[6]); const bool fuse = atoi(argv[7]) != 0;
    const int head_chunk = atoi(argv[8]);
    setDeterministicSeed(4242);
    setup(dir);
    secret_key = rd(dir + "/sk.u64"); public_key = rd(dir + "/pk.u64");
    { auto evk = rd(dir + "/evk.u64");
      ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
      crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr); }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    if (reenc < 0) reenc = net.layer_before_reenc;          // the description's own refresh point
    auto x = rd(dir + "/net_in.u64");
    const ciphertext3D one = ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd);
    if (!fuse) {
        ciphertext3D t = one;
        for (int i = 0; i < reenc; i++) { net.getLayer(i)->out_form = CRC_COEFF; t = net.getLayer(i)->forward(t); wr(dir + "/pre_" + to_string(i) + ".u64", t.toHost()); }
    }
    net.ntt_resident = true; net.layer_before_reenc = reenc; net.keep_reenc_values = true; net.head_chunk = head_chunk;
    if (argc > 9) net.reenc_symmetric = !strcmp(argv[9], "sym") || atoi(argv[9]) != 0;
    if (fuse) { const int removed = net.fuse(); fprintf(stderr, "fused: %d layers removed, %d left, refresh in front of layer %d\n", removed, net.getNumLayers(),
        net.layer_before_reenc); }
    vector<ciphertext3D> imgs(batch, one);
    ciphertext3D out = net.forward(stackImages(imgs));
    { ofstream f(dir + "/reenc_floats.f32", ios::binary); f.write((const char *)net.last_reenc_values.data(), net.last_reenc_values.size() * 4); }
    vector<u64> h = out.toHost(), pl(out.count() * (size_t)crc_ctx_n(context)), bud;
    if (crc_decrypt(context, secret_key.data(), h.data(), out.count(), 2, pl.data())) return 3;
    for (size_t i = 0; i < out.count(); i++) bud.push_back((u64)noiseBudget(out, i));
    wr(dir + "/dec.u64", pl); wr(dir + "/budget.u64", bud);
    for (double ms : net.last_layer_ms) fprintf(stderr, "%.3f,", ms);
    fprintf(stderr, " T_REENC %.3f\n", net.last_reenc_ms);
    // a second forward draws fresh randomness: other ciphertexts, the same plaintexts
    ciphertext3D out2 = net.forward(stackImages(imgs));
    vector<u64> h2 = out2.toHost(), pl2(pl.size());
    if (crc_decrypt(context, secret_key.data(), h2.data(), out2.count(), 2, pl2.data())) return 3;
    if (h2 == h) { fprintf(stderr, "the refresh reused its randomness\n"); return 4; }
    if (pl2 != pl) { fprintf(stderr, "second forward decrypts differently\n"); return 5; }
    delParameters();
    printf("netr ok\n");
    return 0;
}

// plan <model> <h5> <dir> <batch> <fuse 0|1> <head_chunk> <matrix_cores 0|1> <layer_before_reenc>: what ONE Network::forward planned -- the network built as `net` /
// `netr` build it (NTT-resident; <layer_before_reenc> >= 0 places the refresh and needs sk.u64 / pk.u64 in <dir>, -1: none), run once on <batch> copies of the image.
// Prints "refresh <layer>" (where Network::fuse() left the refresh point) and per layer "plan <i> <name> <out_form> <kernelName(), - for none> <launches>": identical
// output ciphertexts do not show that a boundary kept its limb hand-over or a layer its kernel, this table does (tests/test_gpu_host_plan.py)
static int do_plan(int argc, char **argv)
{
    if (argc < 10) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4]; const int batch = atoi(argv[5]); const bool fuse = atoi(argv[6]) != 0; const int reenc = atoi(argv[9]);
    setDeterministicSeed(4242);
    setup(dir);
    if (reenc >= 0) { secret_key = rd(dir + "/sk.u64"); public_key = rd(dir + "/pk.u64"); }
    { auto evk = rd(dir + "/evk.u64");
      ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
      crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr); }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    net.ntt_resident = true; net.layer_before_reenc = reenc; net.head_chunk = atoi(argv[7]); net.matrix_cores = atoi(argv[8]) != 0;
    if (fuse) net.fuse();
    auto x = rd(dir + "/net_in.u64");
    vector<ciphertext3D> imgs(batch, ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd));
    const ciphertext3D out = net.forward(stackImages(imgs));
    if (out.B != batch) { fprintf(stderr, "plan: %d images out of a batch of %d\n", out.B, batch); return 4; }
    printf("refresh %d\n", net.layer_before_reenc);
    for (int i = 0; i < net.getNumLayers(); i++) {
        const string kernel = net.getLayer(i)->kernelName();
        printf("plan %d %s %d %s %d\n", i, net.getLayer(i)->getName().c_str(), net.getLayer(i)->out_form, kernel.empty() ? "-" : kernel.c_str(), net.last_layer_launches[i]);
    }
    delParameters();
    return 0;
}

// encsym <n> <t>: encryptImageSymmetric on a batch (both result forms) decrypts to exactly what encryptImage decrypts to, image by image, under fresh
// randomness per call
static int do_encsym(int argc, char **argv)
{
    if (argc < 4) return 1;
    setDeterministicSeed(99);
    setParameters(atoi(argv[2]), strtoull(argv[3], 0, 0));
    const int B = 3, zd = 2, xd = 5, yd = 4, per = zd * xd * yd;
    vector<float> px((size_t)B * per);
    for (size_t i = 0; i < px.size(); i++) px[i] = (float)((int)((i * 37) % 201) - 100) / 16.0f;
    ciphertext3D a = encryptImageSymmetric(px, zd, xd, yd), an = encryptImageSymmetric(px, zd, xd, yd, CRC_NTT);
    if (a.B != B || a.form != CRC_COEFF || an.form != CRC_NTT) { fprintf(stderr, "encryptImageSymmetric: wrong shape or form\n"); return 4; }
    const vector<u64> ha = a.toHost(), hn = an.toHost();
    vector<u64> back(hn);
    { DeviceBuffer d(hn.size() * 8);
      if (crc_memcpy_h2d(context, d.ptr, hn.data(), hn.size() * 8, nullptr) || crc_ntt_inv(context, (uint64_t *)d.ptr, a.count(), 2, nullptr) ||
          crc_memcpy_d2h(context, back.data(), d.ptr, hn.size() * 8, nullptr) || crc_stream_sync(context, nullptr)) return 3; }
    if (back == ha) { fprintf(stderr, "two calls reused their randomness\n"); return 4; }
    const size_t n = (size_t)crc_ctx_n(context);
    vector<u64> pa(a.count() * n), pn(pa.size());
    if (crc_decrypt(context, secret_key.data(), ha.data(), a.count(), 2, pa.data()) || crc_decrypt(context, secret_key.data(), back.data(), a.count(), 2, pn.data())) return 3;
    if (pa != pn) { fprintf(stderr, "the two forms decrypt differently\n"); return 5; }
    const vector<floatCube> got = decryptImages(a);
    for (int b = 0; b < B; b++) {
        floatCube img(zd, vector<vector<float>>(xd, vector<float>(yd)));
        for (int z = 0; z < zd; z++) for (int i = 0; i < xd; i++) for (int j = 0; j < yd; j++) img[z][i][j] = px[(size_t)b * per + ((size_t)z * xd + i) * yd + j];
        const ciphertext3D pk_ct = encryptImage(img);
        const vector<u64> hp = pk_ct.toHost(); vector<u64> pp(pk_ct.count() * n);
        if (crc_decrypt(context, secret_key.data(), hp.data(), pk_ct.count(), 2, pp.data())) return 3;
        if (memcmp(pp.data(), pa.data() + (size_t)b * per * n, pp.size() * 8)) { fprintf(stderr, "image %d: plaintexts differ from encryptImage's\n", b); return 6; }
        if (decryptImage(pk_ct) != got[b]) { fprintf(stderr, "image %d: floats differ from encryptImage's\n", b); return 6; }
        if (noiseBudget(a, (size_t)b * per) < noiseBudget(pk_ct, 0)) { fprintf(stderr, "image %d: less budget than a public-key ciphertext\n", b); return 7; }
    }
    delParameters();
    printf("encsym ok\n");
    return 0;
}

// seeded <n> <t>: a batch through encryptImageSeeded -> save -> load -> expandSeeded in both forms decrypts to the floats and plaintexts that encryptImage's
// ciphertexts of the same pixels decrypt to, image by image; then the same once under OS entropy (fresh public seed per call, the counter as stream base)
static int do_seeded(int argc, char **argv)
{
    if (argc < 4) return 1;
    const int B = 3, zd = 2, xd = 5, yd = 4, per = zd * xd * yd;
    vector<float> px((size_t)B * per);
    for (size_t i = 0; i < px.size(); i++) px[i] = (float)((int)((i * 37) % 201) - 100) / 16.0f;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0) setDeterministicSeed(99); else clearDeterministicSeed();
        setParameters(atoi(argv[2]), strtoull(argv[3], 0, 0));
        const size_t n = (size_t)crc_ctx_n(context), k = (size_t)crc_ctx_k(context);
        const SeededImages made = encryptImageSeeded(px, zd, xd, yd);
        if (made.B != B || made.zd != zd || made.xd != xd || made.yd != yd || made.c0.size() != (size_t)B * per * k * n) { fprintf(stderr, "encryptImageSeeded: wrong shape\n"); return 4; }
        stringstream file;
        made.save(file);
        if (file.str().size() != 16 + crc_seeded_ct_bytes(context, made.count())) { fprintf(stderr, "SeededImages::save: unexpected size\n"); return 4; }
        if (2 * file.str().size() >= 1.02 * (double)made.count() * (double)crc_ct_words(context, 2) * 8) { fprintf(stderr, "the seeded form is not half a ciphertext\n"); return 4; }
        SeededImages im;
        im.load(file);
        if (im.B != B || im.zd != zd || im.xd != xd || im.yd != yd || im.c0 != made.c0 || memcmp(im.seed, made.seed, 32) || im.stream_base != made.stream_base) {
            fprintf(stderr, "SeededImages: save -> load is not the identity\n"); return 4; }
        { string bad = file.str(); bad[16 + 20] ^= 0x40;                        // a flipped bit in the parameter hash
          stringstream f2(bad); SeededImages x; bool threw = false;
          try { x.load(f2); } catch (const invalid_argument &) { threw = true; }
          if (!threw || !x.c0.empty()) { fprintf(stderr, "SeededImages::load accepted a wrong parameter hash\n"); return 4; } }
        { stringstream f2(file.str().substr(0, file.str().size() - 8)); SeededImages x; bool threw = false;
          try { x.load(f2); } catch (const invalid_argument &) { threw = true; }
          if (!threw) { fprintf(stderr, "SeededImages::load accepted a truncated file\n"); return 4; } }
        const SeededImages again = encryptImageSeeded(px, zd, xd, yd);          // fresh randomness per call
        if (again.c0 == made.c0) { fprintf(stderr, "two calls reused their randomness\n"); return 4; }
        if (pass == 1 && (!memcmp(again.seed, made.seed, 32) || again.stream_base != made.stream_base + made.count())) {
            fprintf(stderr, "OS-entropy mode: the public seed or the stream base did not move on\n"); return 4; }
        ciphertext3D a = expandSeeded(im, CRC_COEFF), an = expandSeeded(im);
        if (a.B != B || a.form != CRC_COEFF || an.form != CRC_NTT || an.count() != a.count()) { fprintf(stderr, "expandSeeded: wrong shape or form\n"); return 4; }
        const vector<u64> ha = a.toHost(), hn = an.toHost();
        if (memcmp(hn.data(), im.c0.data(), k * n * 8)) { fprintf(stderr, "the NTT-form c0 is not the row that travelled\n"); return 4; }
        vector<u64> back(hn);
        { DeviceBuffer d(hn.size() * 8);
          if (crc_memcpy_h2d(context, d.ptr, hn.data(), hn.size() * 8, nullptr) || crc_ntt_inv(context, (uint64_t *)d.ptr, a.count(), 2, nullptr) ||
              crc_memcpy_d2h(context, back.data(), d.ptr, hn.size() * 8, nullptr) || crc_stream_sync(context, nullptr)) return 3; }
        if (back != ha) { fprintf(stderr, "the coefficient form is not the inverse transform of the NTT form\n"); return 5; }
        vector<u64> pa(a.count() * n);
        if (crc_decrypt(context, secret_key.data(), ha.data(), a.count(), 2, pa.data())) return 3;
        const vector<floatCube> got = decryptImages(a);
        for (int b = 0; b < B; b++) {
            floatCube img(zd, vector<vector<float>>(xd, vector<float>(yd)));
            for (int z = 0; z < zd; z++) for (int i = 0; i < xd; i++) for (int j = 0; j < yd; j++) img[z][i][j] = px[(size_t)b * per + ((size_t)z * xd + i) * yd + j];
            const ciphertext3D pk_ct = encryptImage(img);
            const vector<u64> hp = pk_ct.toHost(); vector<u64> pp(pk_ct.count() * n);
            if (crc_decrypt(context, secret_key.data(), hp.data(), pk_ct.count(), 2, pp.data())) return 3;
            if (memcmp(pp.data(), pa.data() + (size_t)b * per * n, pp.size() * 8)) { fprintf(stderr, "image %d: plaintexts differ from encryptImage's\n", b); return 6; }
            if (decryptImage(pk_ct) != got[b]) { fprintf(stderr, "image %d: floats differ from encryptImage's\n", b); return 6; }
            if (noiseBudget(a, (size_t)b * per) < noiseBudget(pk_ct, 0)) { fprintf(stderr, "image %d: less budget than a public-key ciphertext\n", b); return 7; }
        }
        delParameters();
    }
    printf("seeded ok\n");
    return 0;
}

// netseeded <model> <h5> <dir>: <dir>/params.u64 and pixels.f32 ([B][28][28] normalised floats).  The fused, NTT-resident network on
// expandSeeded(encryptImageSeeded(x)) against the same network on encryptImage(x): the decrypted output plaintexts must be equal polynomial for polynomial, and
// every output of the seeded run must have at least the budget of its public-key counterpart.  Writes dec_seeded.u64, dec_pk.u64 and prints the budgets
static int do_netseeded(int argc, char **argv)
{
    if (argc < 5) return 1;
    string model = argv[2], h5 = argv[3], dir = argv[4];
    setDeterministicSeed(4242);
    setup(dir);
    vector<float> px;
    { ifstream f(dir + "/pixels.f32", ios::binary); if (!f) { fprintf(stderr, "missing pixels.f32\n"); return 2; }
      f.seekg(0, ios::end); const size_t sz = f.tellg(); f.seekg(0); px.resize(sz / 4); f.read((char *)px.data(), sz); }
    if (px.empty() || px.size() % 784) { fprintf(stderr, "pixels.f32 must hold [B][28][28] floats\n"); return 2; }
    const int B = (int)(px.size() / 784);
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkByName(model);
    net.ntt_resident = true;
    const int removed = net.fuse();
    fprintf(stderr, "fused: %d layers removed, %d left\n", removed, net.getNumLayers());
    vector<ciphertext3D> imgs;
    for (int b = 0; b < B; b++) {
        floatCube img(1, vector<vector<float>>(28, vector<float>(28)));
        for (int i = 0; i < 28; i++) for (int j = 0; j < 28; j++) img[0][i][j] = px[(size_t)b * 784 + i * 28 + j];
        imgs.push_back(encryptImage(img));
    }
    const ciphertext3D out_pk = net.forward(stackImages(imgs));
    const SeededImages sent = encryptImageSeeded(px, 1, 28, 28);
    const ciphertext3D out_sd = net.forward(expandSeeded(sent));
    if (out_sd.count() != out_pk.count() || out_sd.B != B) { fprintf(stderr, "output shapes differ\n"); return 4; }
    const size_t n = (size_t)crc_ctx_n(context);
    const vector<u64> hp = out_pk.toHost(), hs = out_sd.toHost();
    if (hp == hs) { fprintf(stderr, "the two runs produced the same ciphertexts: not two encryptions\n"); return 4; }
    vector<u64> pp(out_pk.count() * n), ps(pp.size());
    if (crc_decrypt(context, secret_key.data(), hp.data(), out_pk.count(), 2, pp.data()) || crc_decrypt(context, secret_key.data(), hs.data(), out_sd.count(), 2, ps.data())) return 3;
    wr(dir + "/dec_pk.u64", pp); wr(dir + "/dec_seeded.u64", ps);
    const vector<int> bp = noiseBudgets(out_pk), bs = noiseBudgets(out_sd);
    printf("budgets public-key:"); for (int v : bp) printf(" %d", v);
    printf("\nbudgets seeded:"); for (int v : bs) printf(" %d", v);
    printf("\n");
    if (pp != ps) { fprintf(stderr, "the seeded run decrypts to other plaintexts than the public-key run\n"); return 5; }
    for (size_t i = 0; i < bp.size(); i++) if (bs[i] < bp[i] || bs[i] <= 0) { fprintf(stderr, "output %zu: budget %d under seeded inputs, %d under public-key inputs\n", i, bs[i], bp[i]); return 7; }
    delParameters();
    printf("netseeded ok\n");
    return 0;
}

// budgetsym: the budget-checking forward (Network::max_num_of_reencryptions >= 0, network.cpp:52-96) with Network::reenc_symmetric.  Three Square layers at
// (4096, t = 2^29) run out of budget on the way, so the forward refreshes and repeats.  With the flag set every refresh must go through the secret key alone:
// the public key is taken away for that forward, and a public-key refresh would throw.  The result is what the arithmetic gives and what the public-key mode
// gives, the first refresh sees the same floats in both modes, and the secret-key mode does not need more refreshes
static int do_budgetsym(int, char **)
{
    setDeterministicSeed(123);
    setParameters(4096, 1ULL << 29);
    const float v[4] = {0.5f, -0.75f, 1.25f, 0.3f};
    const ciphertext3D x = encryptImage(floatCube{{{v[0], v[1]}, {v[2], v[3]}}});
    auto build = [&]() {
        Network nn;
        for (int i = 0; i < 3; i++) nn.getLayers().push_back(shared_ptr<Layer>(new SquareLayer("s" + to_string(i), 2)));
        nn.max_num_of_reencryptions = 6; nn.keep_reenc_values = true;
        return nn;
    };
    Network sym = build(); sym.reenc_symmetric = true;
    const vector<u64> pk_saved = public_key;
    public_key.clear();
    floatCube got;
    try { got = decryptImage(sym.forward(x)); }
    catch (const exception &e) { public_key = pk_saved; fprintf(stderr, "budget-checking forward with reenc_symmetric: %s\n", e.what()); return 4; }
    public_key = pk_saved;
    if (sym.last_reenc_values.empty() || sym.last_reenc_values.size() % 4) { fprintf(stderr, "no refresh ran: the case does not reach the branch (%zu values)\n",
        sym.last_reenc_values.size()); return 5; }
    for (int i = 0; i < 4; i++) {
        const double want = pow((double)v[i], 8.0), have = got[0][i / 2][i % 2];
        if (fabs(have - want) > 1e-3) { fprintf(stderr, "value %d: %f, expected %f\n", i, have, want); return 6; }
    }
    Network pkn = build();
    const floatCube ref = decryptImage(pkn.forward(x));
    for (int i = 0; i < 4; i++) if (fabs(ref[0][i / 2][i % 2] - got[0][i / 2][i % 2]) > 1e-3) { fprintf(stderr, "the two modes decrypt differently at %d\n", i); return 7; }
    if (pkn.last_reenc_values.size() < 4 || memcmp(pkn.last_reenc_values.data(), sym.last_reenc_values.data(), 4 * sizeof(float))) {
        fprintf(stderr, "the first refresh saw other floats than the public-key mode's\n"); return 8; }
    if (sym.last_reenc_values.size() > pkn.last_reenc_values.size()) { fprintf(stderr, "more refreshes with the secret key (%zu values) than with the public key (%zu)\n",
        sym.last_reenc_values.size(), pkn.last_reenc_values.size()); return 9; }
    fprintf(stderr, "refreshed values: secret key %zu, public key %zu\n", sym.last_reenc_values.size(), pkn.last_reenc_values.size());
    delParameters();
    printf("budgetsym ok\n");
    return 0;
}

static vector<double> rdf(const string &p)
{
    ifstream f(p, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", p.c_str()); exit(2); }
    f.seekg(0, ios::end); size_t sz = f.tellg(); f.seekg(0); vector<double> v(sz / 8); f.read((char *)v.data(), sz); return v;
}
static int do_files(int argc, char **argv)
{
    if (argc < 3) return 1;
    const string dir = argv[2];
    setup(dir);
    secret_key = rd(dir + "/sk.u64"); public_key = rd(dir + "/pk.u64");            // the fixture's key pair (globals are public, as in the reference)
    auto dims = rd(dir + "/layer_dims.u64");
    const int zd = (int)dims[0], xd = (int)dims[1], yd = (int)dims[2], xs = (int)dims[3], ys = (int)dims[4], xf = (int)dims[5], yf = (int)dims[6], nf =
        (int)dims[7], od = (int)dims[8];
    const int xo = (xd - xf) / xs + 1, yo = (yd - yf) / ys + 1;
    auto run = [&](Layer &c, Layer &b, Layer &f, const ciphertext3D &x, const string &out) {
        c.out_form = b.out_form = f.out_form = CRC_COEFF;
        wr(dir + "/" + out, f.forward(b.forward(c.forward(x))).toHost());
    };
    {   // what the reference wrote
        ifstream in(dir + "/ref_encoded_layers.bin", ios::binary); if (!in) { fprintf(stderr, "missing ref_encoded_layers.bin\n"); return 2; }
        ConvolutionalLayer c("conv", xd, yd, zd, xs, ys, xf, yf, nf, 2, &in);
        BatchNormLayer b("bn", nf, &in);
        FullyConnectedLayer f("fc", nf * xo * yo, od, 2, &in);
        if (in.peek() != EOF) { fprintf(stderr, "encoded-model stream not consumed exactly\n"); return 3; }
        run(c, b, f, loadEncryptedImage(zd, xd, yd, dir + "/ref_cipher_image.bin"), "out_from_ref_files.u64");
    }
    {   // the same files written by the host classes (encoding as CnnBuilder::build*Layer: float32 widened to double)
        auto enc = [&](const vector<double> &v) { vector<Plaintext> o; for (double d : v) o.push_back(fraencode((double)(float)d)); return o; };
        auto fw = enc(rdf(dir + "/conv_w.f64")), fb = enc(rdf(dir + "/conv_b.f64")), bm = enc(rdf(dir + "/bn_mean.f64")), dw = enc(rdf(dir + "/fc_w.f64")),
            db = enc(rdf(dir + "/fc_b.f64"));
        // cnnBuilder.cpp:100-102
        vector<Plaintext> bv; for (double d : rdf(dir + "/bn_var.f64")) { float v = (float)d; v = 1 / sqrt(v + 0.00001); bv.push_back(fraencode((double)v)); }
        plaintext4D ew(nf, plaintext3D(zd, plaintext2D(xf, vector<Plaintext>(yf)))); size_t w = 0;
        for (int n = 0; n < nf; n++) for (int z = 0; z < zd; z++) for (int i = 0; i < xf; i++) for (int j = 0; j < yf; j++) ew[n][z][i][j] = fw[w++];
        plaintext2D ed(od, vector<Plaintext>(nf * xo * yo)); w = 0;
        for (int i = 0; i < od; i++) for (int j = 0; j < nf * xo * yo; j++) ed[i][j] = dw[w++];
        ConvolutionalLayer c("conv", xd, yd, zd, xs, ys, xf, yf, nf, 2, ew, fb);
        BatchNormLayer b("bn", nf, bm, bv);
        FullyConnectedLayer f("fc", nf * xo * yo, od, 2, ed, db);
        { ofstream o(dir + "/our_encoded_layers.bin", ios::binary); c.savePlaintextParameters(&o); b.savePlaintextParameters(&o);
            f.savePlaintextParameters(&o); }
        vector<float> image; for (double d : rdf(dir + "/image.f64")) image.push_back((float)d);
        ciphertext3D x = encryptAndSaveImage(image, zd, xd, yd, dir + "/our_cipher_image.bin");
        run(c, b, f, x, "out_from_our_files.u64");
    }
    delParameters();
    printf("files ok\n");
    return 0;
}

static const char *status_name(exit_status_forward s) { return s == SUCCESS ? "SUCCESS" : s == OUT_OF_BUDGET ? "OUT_OF_BUDGET" : "MISPREDICTED"; }

static int do_searchlogic(int argc, char **argv)
{
    if (argc < 7) return 1;
    const u64 lo = strtoull(argv[2], 0, 0), hi = strtoull(argv[3], 0, 0), first_good = strtoull(argv[4], 0, 0), last_good = strtoull(argv[5], 0, 0), min_q =
        strtoull(argv[6], 0, 0);
    vector<pair<u64, exit_status_forward>> tried;
    auto pred = [&](u64 t) { exit_status_forward s = t < first_good ? MISPREDICTED : t > last_good ? OUT_OF_BUDGET : SUCCESS; tried.emplace_back(t, s);
        return s; };
    const u64 found = plainModulusBinarySearch(pred, lo, hi, min_q);
    printf("found %llu\n", (unsigned long long)found);
    for (auto &p : tried) printf("tried %llu %s\n", (unsigned long long)p.first, status_name(p.second));
    return 0;
}

static int do_search(int argc, char **argv)
{
    if (argc < 10) return 1;
    PlainModulusSearch s;
    s.model = argv[2];
    const string h5 = argv[3], images = argv[4];
    s.max_poly_modulus = atoi(argv[5]);
    const u64 lo = strtoull(argv[6], 0, 0), hi = strtoull(argv[7], 0, 0);
    const int num_images = atoi(argv[8]); s.seed = (unsigned)strtoul(argv[9], 0, 0);
    for (int i = 10; i < argc; i++) s.coeff_modulus.push_back(strtoull(argv[i], 0, 0));
    ifstream f(images, ios::binary); if (!f) { fprintf(stderr, "missing %s\n", images.c_str()); return 2; }
    const NetworkDescription desc = NetworkDescription::load(s.model);
    const size_t px = (size_t)desc.zd * desc.xd * desc.yd;
    f.seekg(0, ios::end); const size_t cnt = (size_t)f.tellg() / (px * 4); f.seekg(0);
    s.test_set.assign(cnt, vector<float>(px));
    for (auto &im : s.test_set) f.read((char *)im.data(), px * 4);
    s.predictWithPlainModel(h5);
    for (size_t i = 0; i < cnt; i++) printf("label %zu %d\n", i, (int)s.predicted_labels[i]);
    const u64 found = s.run(num_images, lo, hi, h5);
    printf("found %llu\n", (unsigned long long)found);
    for (size_t i = 0; i < s.tried.size(); i++) printf("tried %llu %s %.2f\n", (unsigned long long)s.tried[i].first, status_name(s.tried[i].second),
        s.test_seconds[i]);
    return 0;
}

// describe <name | description file> [h5]: the canonical form of a description on stdout; an invalid one ends in "exception: line N: ..." and status 10
static int do_describe(int argc, char **argv)
{
    if (argc < 3) return 1;
    fputs(NetworkDescription::load(argv[2], argc > 3 ? argv[3] : "").str().c_str(), stdout);
    return 0;
}

// labels <model> <h5> <images.f32>: the float forward of the model's description on every image: "label <i> <argmax>" and "logits <i> <v0> <v1> ..."
static int do_labels(int argc, char **argv)
{
    if (argc < 5) return 1;
    const string model = argv[2];
    const NetworkDescription desc = NetworkDescription::load(model);
    const size_t px = (size_t)desc.zd * desc.xd * desc.yd;
    ifstream f(argv[4], ios::binary); if (!f) { fprintf(stderr, "missing %s\n", argv[4]); return 2; }
    f.seekg(0, ios::end); const size_t cnt = (size_t)f.tellg() / (px * 4); f.seekg(0);
    CnnBuilder build(argv[3]);
    PlainModulusSearch s;
    s.model = model;
    s.test_set.assign(cnt, vector<float>(px));
    for (auto &im : s.test_set) f.read((char *)im.data(), px * 4);
    s.predictWithPlainModel(argv[3]);
    for (size_t i = 0; i < cnt; i++) {
        printf("label %zu %d\n", i, (int)s.predicted_labels[i]);
        printf("logits %zu", i);
        for (float v : plainModelForward(build, model, s.test_set[i])) printf(" %.9g", v);
        printf("\n");
    }
    return 0;
}

// build <description> <h5> <dir> <batch>: one network built from a description (<dir> as for `net`: params.u64, evk.u64, net_in.u64 = one encrypted image of
// the description's input shape), run four ways:
//   layer by layer in coefficient form      -> layer_<i>.u64, and one line "layer <i> <kind> <name> <zd> <xd> <yd> <fnv-1a 64 of the tensor>" per layer
//   Network::forward, NTT-resident           -> out_unfused.u64
//   after Network::fuse()                    -> out_fused.u64, and on <batch> images out_fused_batch.u64
// Prints "describe-ok" when Network::describe() is the description's canonical form and builds back to the same text, and the layer names after fuse()
// ("fused <name> <name> ...")
// multiplyRelin elementwise on two tensors; unequal shapes and forms must throw std::invalid_argument
static int do_multiply(int argc, char **argv)
{
    if (argc < 4) return 1;
    const string dir = argv[2]; const int count = atoi(argv[3]);
    setup(dir);
    { auto evk = rd(dir + "/evk.u64");
      ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
      crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr); }
    auto hx = rd(dir + "/mul_x.u64"), hy = rd(dir + "/mul_y.u64");
    const ciphertext3D x = ciphertext3D::fromHost(hx.data(), 1, 1, 1, count), y = ciphertext3D::fromHost(hy.data(), 1, 1, 1, count);
    wr(dir + "/mul_cc.u64", multiplyRelin(x, y, CRC_COEFF).toHost());
    ciphertext3D xn = ciphertext3D::fromHost(hx.data(), 1, 1, 1, count), yn = ciphertext3D::fromHost(hy.data(), 1, 1, 1, count);
    crc_ntt_fwd(context, xn.data(), count, 2, nullptr); xn.form = CRC_NTT;
    crc_ntt_fwd(context, yn.data(), count, 2, nullptr); yn.form = CRC_NTT;
    crc_stream_sync(context, nullptr);
    ciphertext3D out = multiplyRelin(xn, yn, CRC_NTT);
    if (out.form != CRC_NTT) return 4;
    wr(dir + "/mul_nn.u64", out.toHost());
    int refused = 0;
    try { multiplyRelin(x, yn); } catch (const invalid_argument &) { refused++; }                                       // forms differ
    try { multiplyRelin(x, ciphertext3D::fromHost(hy.data(), 1, 1, count, 1)); } catch (const invalid_argument &) { refused++; }      // shapes differ
    try { multiplyRelin(x, y, CRC_NTTP); } catch (const invalid_argument &) { refused++; }                              // no packed result
    try { multiplyRelin(ciphertext3D(), y); } catch (const invalid_argument &) { refused++; }                          // empty
    delParameters();
    printf("multiply ok refused %d\n", refused);
    return refused == 4 ? 0 : 4;
}

static int do_build(int argc, char **argv)
{
    if (argc < 6) return 1;
    string desc = argv[2], h5 = argv[3], dir = argv[4]; const int batch = atoi(argv[5]);
    setup(dir);
    { auto evk = rd(dir + "/evk.u64");
      ev_keys16 = make_shared<DeviceBuffer>(evk.size() * 8);
      crc_memcpy_h2d(context, ev_keys16->ptr, evk.data(), evk.size() * 8, nullptr); crc_stream_sync(context, nullptr); }
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkFromDescription(desc);
    const string canon = NetworkDescription::load(desc).str();
    if (net.describe() != canon) { fprintf(stderr, "describe() differs from the canonical form:\n%s", net.describe().c_str()); return 4; }
    if (builder.buildNetworkFromDescription(net.describe()).describe() != canon) { fprintf(stderr, "describe() does not build back\n"); return 4; }
    printf("describe-ok\n");
    auto x = rd(dir + "/net_in.u64");
    const ciphertext3D one = ciphertext3D::fromHost(x.data(), 1, net.input_zd, net.input_xd, net.input_yd);
    {
        ciphertext3D t = one;
        for (int i = 0; i < net.getNumLayers(); i++) {
            net.getLayer(i)->out_form = CRC_COEFF;
            t = net.getLayer(i)->forward(t);
            const vector<u64> h = t.toHost();
            u64 fnv = 1469598103934665603ULL;
            for (size_t j = 0; j < h.size() * 8; j++) fnv = (fnv ^ ((const unsigned char *)h.data())[j]) * 1099511628211ULL;
            wr(dir + "/layer_" + to_string(i) + ".u64", h);
            const string kind = NetworkDescription::load(desc).layers[i].kind;
            printf("layer %d %s %s %d %d %d %016llx\n", i, kind.c_str(), net.getLayer(i)->getName().c_str(), t.zd, t.xd, t.yd, (unsigned long long)fnv);
        }
    }
    net.ntt_resident = true;
    { ciphertext3D out = net.forward(one); wr(dir + "/out_unfused.u64", out.toHost()); }
    const int removed = net.fuse();
    fprintf(stderr, "fused: %d layers removed, %d left\n", removed, net.getNumLayers());
    printf("fused");
    for (int i = 0; i < net.getNumLayers(); i++) printf(" %s", net.getLayer(i)->getName().c_str());
    printf("\n");
    { ciphertext3D out = net.forward(one); wr(dir + "/out_fused.u64", out.toHost()); }
    vector<ciphertext3D> imgs(batch, one);
    { ciphertext3D out = net.forward(stackImages(imgs)); wr(dir + "/out_fused_batch.u64", out.toHost()); }
    delParameters();
    printf("build ok\n");
    return 0;
}

static int do_slots_describe(int argc, char **argv)
{
    if (argc < 5) return 1;
    const NetworkDescription d = NetworkDescription::load(argv[2]);
    const vector<double> s = slotScales(d, atoi(argv[3]), atoi(argv[4]));
    for (size_t i = 0; i < d.layers.size(); i++) printf("scale %zu %s %s %.17g\n", i, d.layers[i].kind.c_str(), d.layers[i].name.c_str(), s[i]);
    printf("slot_scale %.17g\n", s.back());
    return 0;
}

// build_plain <description>: the builder on a description WITHOUT slot encoding and without an engine -- for the lines only slot encoding admits, which it
// refuses ("exception: line N: ... needs slot encoding", status 10) before any layer in front of them needs a context when they come first
static int do_build_plain(int argc, char **argv)
{
    if (argc < 3) return 1;
    CnnBuilder builder("");
    Network net = builder.buildNetworkFromDescription(argv[2]);
    printf("build_plain ok %d layers\n", net.getNumLayers());
    return 0;
}

// slots_build <description> <h5> <dir> <S> <input_bits> <weight_bits>: slot-batched inference through the host classes.  <dir>/params.u64 (n, k, t, q...: t a
// slot prime), <dir>/images.f32 = [S][zd xd yd] float32 pixels.  Keys from a deterministic seed; the S images are encrypted into one tensor (encryptImageSlots),
// run through Network::forward unfused and after Network::fuse(), decrypted and decomposed: slots_unfused.i64 / slots_fused.i64 = [S][outputs] int64.
// Prints "slot_scale <sigma>", "budget unfused <bits> fused <bits>" (minNoiseBudget of the output tensors) and "describe-ok" when Network::describe() is the
// description's canonical form (slot encoding does not change it).  With <reps> > 0 the fused forward runs <reps> times more between two stream synchronisations:
// "forward_ms <milliseconds per tensor evaluation>" (tools/measure_slots.py)
static int do_slots_build(int argc, char **argv)
{
    if (argc < 8) return 1;
    const string desc = argv[2], h5 = argv[3], dir = argv[4]; const int S = atoi(argv[5]), in_bits = atoi(argv[6]), w_bits = atoi(argv[7]);
    setDeterministicSeed(20240611);
    setup(dir);
    setSlotEncoding(in_bits, w_bits);
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkFromDescription(desc);
    if (net.describe() != NetworkDescription::load(desc).str()) { fprintf(stderr, "describe() differs from the canonical form\n"); return 4; }
    printf("describe-ok\n");
    const size_t px = (size_t)net.input_zd * net.input_xd * net.input_yd;
    vector<vector<float>> images(S, vector<float>(px));
    { ifstream f(dir + "/images.f32", ios::binary); if (!f) { fprintf(stderr, "missing images.f32\n"); return 2; }
      for (auto &im : images) f.read((char *)im.data(), px * 4);
      if (!f) { fprintf(stderr, "images.f32 is too short\n"); return 2; } }
    const ciphertext3D in = encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd);
    auto dump = [&](const string &name, const ciphertext3D &out) {
        const vector<vector<int64_t>> v = decryptSlots(out, S);
        ofstream f(dir + "/" + name, ios::binary);
        for (auto &row : v) f.write((const char *)row.data(), row.size() * 8);
        return minNoiseBudget(out);
    };
    net.ntt_resident = true;
    const int b0 = dump("slots_unfused.i64", net.forward(in));
    const int removed = net.fuse();
    fprintf(stderr, "fused: %d layers removed, %d left\n", removed, net.getNumLayers());
    const int b1 = dump("slots_fused.i64", net.forward(in));
    printf("slot_scale %.17g\n", net.slot_scale());
    printf("budget unfused %d fused %d\n", b0, b1);
    const int reps = argc > 8 ? atoi(argv[8]) : 0;
    if (reps > 0) {
        crc_stream_sync(context, getStream());
        const auto t0 = chrono::steady_clock::now();
        for (int r = 0; r < reps; r++) net.forward(in);
        crc_stream_sync(context, getStream());
        printf("forward_ms %.6f\n", chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count() / reps);
    }
    delParameters();
    clearDeterministicSeed();
    printf("slots_build ok\n");
    return 0;
}

// slots_rescale_plan <description> <h5> <dir> <S> <input_bits> <weight_bits>: a slot-batched network with `rescale` layers (SlotRescaleLayer) under every way
// Network::forward can run it -- files as for slots_build.  The NTT-resident forward of one tensor is the yardstick; the same integers must come out of
//   a profiled forward timed with events (profile_budget, time_with_events): every rescale layer is timed as a layer (last_reenc_ms stays 0), its producer
//     hands over CRC_NTT, and its output has more noise budget than its input;
//   two-level chunking (three tensors stacked into a batch, head_chunk = 1): the layer works per ciphertext, so every image of the batch gives the yardstick;
//   a forward that is not NTT-resident; and one whose rescale layers re-encrypt under the secret key (SlotRescaleLayer::symmetric).
// A rescale layer asked for a form that is no ciphertext form throws std::invalid_argument.  Prints "slots_rescale_plan ok"
static int do_slots_rescale_plan(int argc, char **argv)
{
    if (argc < 8) return 1;
    const string desc = argv[2], h5 = argv[3], dir = argv[4]; const int S = atoi(argv[5]), in_bits = atoi(argv[6]), w_bits = atoi(argv[7]);
    // Every way out of this driver, a failed check's early return and an exception included, releases the engine first (declared in front of the network and the
    // tensors, so it goes last): the library's global device buffers must not be freed by static destructors, after the HIP runtime's own exit handlers have run
    struct Release { ~Release() { delParameters(); clearDeterministicSeed(); } } release;
    setDeterministicSeed(20240612);
    setup(dir);
    setSlotEncoding(in_bits, w_bits);
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkFromDescription(desc);
    const size_t px = (size_t)net.input_zd * net.input_xd * net.input_yd;
    vector<vector<float>> images(S, vector<float>(px));
    { ifstream f(dir + "/images.f32", ios::binary); if (!f) { fprintf(stderr, "missing images.f32\n"); return 2; }
      for (auto &im : images) f.read((char *)im.data(), px * 4);
      if (!f) { fprintf(stderr, "images.f32 is too short\n"); return 2; } }
    const ciphertext3D in = encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd);
    vector<int> at;
    for (int i = 0; i < net.getNumLayers(); i++) if (dynamic_pointer_cast<SlotRescaleLayer>(net.getLayers()[i])) at.push_back(i);
    if (at.empty()) { fprintf(stderr, "the description has no rescale layer\n"); return 2; }
    net.ntt_resident = true;
    const vector<vector<int64_t>> ref = decryptSlots(net.forward(in), S);
    // profiled, timed with events
    net.profile_budget = true; net.time_with_events = true;
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the profiled forward differs\n"); return 5; }
    if (net.last_reenc_ms != 0.0) { fprintf(stderr, "a rescale layer was timed as T_REENC\n"); return 5; }
    for (int i : at) {
        if (i == 0) continue;
        const int before = net.last_layer_budget_min[i - 1], after = net.last_layer_budget_min[i];
        printf("rescale layer %d: %.3f ms, budget %d -> %d, producer out_form %d\n", i, net.last_layer_ms[i], before, after, net.getLayers()[i - 1]->out_form);
        if (!(net.last_layer_ms[i] > 0.0) || net.last_layer_launches[i] != 1) { fprintf(stderr, "rescale layer %d was not timed as a layer\n", i); return 5; }
        if (net.getLayers()[i - 1]->out_form != CRC_NTT) { fprintf(stderr, "the producer of rescale layer %d does not hand over CRC_NTT\n", i); return 5; }
        if (before < 0 || after <= before) { fprintf(stderr, "rescale layer %d: budget %d -> %d\n", i, before, after); return 5; }
    }
    net.profile_budget = false; net.time_with_events = false;
    // two-level chunking: three tensors of the same images (fresh randomness each) as one batch, one image per chunk
    {
        vector<ciphertext3D> three = {in, encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd), encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd)};
        const ciphertext3D batch = stackImages(three);
        net.head_chunk = 1;
        const ciphertext3D out = net.forward(batch);
        net.head_chunk = 0;
        if (out.B != 3) { fprintf(stderr, "the chunked forward returned %d images\n", out.B); return 6; }
        const vector<vector<int64_t>> got = decryptSlots(out, S);
        const size_t no = ref[0].size();
        for (int s = 0; s < S; s++) for (int b = 0; b < 3; b++) for (size_t o = 0; o < no; o++)
            if (got[s][b * no + o] != ref[s][o]) { fprintf(stderr, "the chunked forward differs at slot %d image %d output %zu\n", s, b, o); return 6; }
    }
    net.ntt_resident = false;
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the layerwise (coefficient-form) forward differs\n"); return 7; }
    net.ntt_resident = true;
    for (int i : at) dynamic_pointer_cast<SlotRescaleLayer>(net.getLayers()[i])->symmetric = true;
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the forward with secret-key re-encryption differs\n"); return 8; }
    {
        SlotRescaleLayer r("r", 0);
        r.out_form = CRC_NTTP;
        bool thrown = false;
        try { r.forward(in); } catch (const invalid_argument &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "a rescale layer accepted a packed output form\n"); return 9; }
    }
    printf("slots_rescale_plan ok\n");
    return 0;
}

// slots_act_plan <description> <h5> <dir> <S> <input_bits> <weight_bits>: slots_rescale_plan for a slot-batched network with client-side activation layers
// (`client_relu` / `client_maxpool`: SlotReluLayer, SlotMaxPoolLayer) -- files as for slots_build.  The NTT-resident forward of one tensor is the yardstick; the same integers must come out of
//   a profiled forward timed with events (profile_budget, time_with_events): every client layer is timed as a layer (last_reenc_ms stays 0), its producer
//     hands over CRC_NTT, and its output has more noise budget than its input;
//   two-level chunking (three tensors stacked into a batch, head_chunk = 1): the layer works per ciphertext, so every image of the batch gives the yardstick;
//   a forward that is not NTT-resident; and one whose client layers re-encrypt under the secret key (their `symmetric`).
// A client layer asked for a form that is no ciphertext form throws std::invalid_argument.  Prints "slots_act_plan ok"
static int do_slots_act_plan(int argc, char **argv)
{
    if (argc < 8) return 1;
    const string desc = argv[2], h5 = argv[3], dir = argv[4]; const int S = atoi(argv[5]), in_bits = atoi(argv[6]), w_bits = atoi(argv[7]);
    // Every way out of this driver, a failed check's early return and an exception included, releases the engine first (declared in front of the network and the
    // tensors, so it goes last): the library's global device buffers must not be freed by static destructors, after the HIP runtime's own exit handlers have run
    struct Release { ~Release() { delParameters(); clearDeterministicSeed(); } } release;
    setDeterministicSeed(20240613);
    setup(dir);
    setSlotEncoding(in_bits, w_bits);
    CnnBuilder builder(h5);
    Network net = builder.buildNetworkFromDescription(desc);
    const size_t px = (size_t)net.input_zd * net.input_xd * net.input_yd;
    vector<vector<float>> images(S, vector<float>(px));
    { ifstream f(dir + "/images.f32", ios::binary); if (!f) { fprintf(stderr, "missing images.f32\n"); return 2; }
      for (auto &im : images) f.read((char *)im.data(), px * 4);
      if (!f) { fprintf(stderr, "images.f32 is too short\n"); return 2; } }
    const ciphertext3D in = encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd);
    vector<int> at;
    for (int i = 0; i < net.getNumLayers(); i++) if (dynamic_pointer_cast<SlotReluLayer>(net.getLayers()[i]) || dynamic_pointer_cast<SlotMaxPoolLayer>(net.getLayers()[i])) at.push_back(i);
    if (at.empty()) { fprintf(stderr, "the description has no client_relu or client_maxpool layer\n"); return 2; }
    net.ntt_resident = true;
    const vector<vector<int64_t>> ref = decryptSlots(net.forward(in), S);
    // profiled, timed with events
    net.profile_budget = true; net.time_with_events = true;
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the profiled forward differs\n"); return 5; }
    if (net.last_reenc_ms != 0.0) { fprintf(stderr, "a client layer was timed as T_REENC\n"); return 5; }
    for (int i : at) {
        if (i == 0) continue;
        const int before = net.last_layer_budget_min[i - 1], after = net.last_layer_budget_min[i];
        printf("client layer %d: %.3f ms, budget %d -> %d, producer out_form %d\n", i, net.last_layer_ms[i], before, after, net.getLayers()[i - 1]->out_form);
        if (!(net.last_layer_ms[i] > 0.0) || net.last_layer_launches[i] != 1) { fprintf(stderr, "client layer %d was not timed as a layer\n", i); return 5; }
        if (net.getLayers()[i - 1]->out_form != CRC_NTT) { fprintf(stderr, "the producer of client layer %d does not hand over CRC_NTT\n", i); return 5; }
        if (before < 0 || after <= before) { fprintf(stderr, "client layer %d: budget %d -> %d\n", i, before, after); return 5; }
    }
    net.profile_budget = false; net.time_with_events = false;
    // two-level chunking: three tensors of the same images (fresh randomness each) as one batch, one image per chunk
    {
        vector<ciphertext3D> three = {in, encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd), encryptImageSlots(images, net.input_zd, net.input_xd, net.input_yd)};
        const ciphertext3D batch = stackImages(three);
        net.head_chunk = 1;
        const ciphertext3D out = net.forward(batch);
        net.head_chunk = 0;
        if (out.B != 3) { fprintf(stderr, "the chunked forward returned %d images\n", out.B); return 6; }
        const vector<vector<int64_t>> got = decryptSlots(out, S);
        const size_t no = ref[0].size();
        for (int s = 0; s < S; s++) for (int b = 0; b < 3; b++) for (size_t o = 0; o < no; o++)
            if (got[s][b * no + o] != ref[s][o]) { fprintf(stderr, "the chunked forward differs at slot %d image %d output %zu\n", s, b, o); return 6; }
    }
    net.ntt_resident = false;
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the layerwise (coefficient-form) forward differs\n"); return 7; }
    net.ntt_resident = true;
    for (int i : at) {
        if (auto r = dynamic_pointer_cast<SlotReluLayer>(net.getLayers()[i])) r->symmetric = true;
        if (auto m = dynamic_pointer_cast<SlotMaxPoolLayer>(net.getLayers()[i])) m->symmetric = true;
    }
    if (decryptSlots(net.forward(in), S) != ref) { fprintf(stderr, "the forward with secret-key re-encryption differs\n"); return 8; }
    {
        SlotReluLayer r("r", 0);
        SlotMaxPoolLayer m("m", 1, 1, 1, 1, 0);
        r.out_form = m.out_form = CRC_NTTP;
        int thrown = 0;
        try { r.forward(in); } catch (const invalid_argument &) { thrown++; }
        try { m.forward(in); } catch (const invalid_argument &) { thrown++; }
        if (thrown != 2) { fprintf(stderr, "a client layer accepted a packed output form\n"); return 9; }
    }
    printf("slots_act_plan ok\n");
    return 0;
}

#define EXPECT_THROW(stmt, type) do { bool ok_ = false; try { stmt; } catch (const type &) { ok_ = true; } catch (...) {} if (!ok_) { fprintf(stderr, "expected " #type " from: " #stmt "\n"); return 3; } } while (0)

// plain_base <n> <S> <divisor> <cap> <t_0> [<t_1> ...]: S images of 1 x 2 x 2 pixels through the host classes over a residue base -- encryptImageSlotsCrt,
// decryptSlotsCrt, rescaleSlotsCrt (relu, cap) under the public and under the secret key, component / setComponent, the base of one modulus against
// encryptImageSlots -> decryptSlots, and the refusal of a stale base.  Pixel p of image s is ((4 s + p) 0x9E3779B97F4A7C15 mod 2^64 mod T) - (T - 1) / 2;
// image 0 is (T - 1) / 2, -(T - 1) / 2, 0, divisor / 2.  Prints the integers, one line per image.
static int do_plain_base(int argc, char **argv)
{
    if (argc < 7) return 1;
    const int n = atoi(argv[2]), S = atoi(argv[3]);
    const uint64_t D = strtoull(argv[4], 0, 0), cap = strtoull(argv[5], 0, 0);
    vector<uint64_t> ts;
    for (int i = 6; i < argc; i++) ts.push_back(strtoull(argv[i], 0, 0));
    setDeterministicSeed(1);
    setParameters(n, ts[0]);
    setSlotEncoding(4, 5);
    auto base = makePlainBase(ts);
    const int64_t half = (int64_t)((base->T - 1) / 2);
    vector<vector<int64_t>> images(S, vector<int64_t>(4));
    for (int s = 0; s < S; s++) for (int p = 0; p < 4; p++) images[s][p] = (int64_t)((uint64_t)(4 * s + p) * 0x9E3779B97F4A7C15ULL % base->T) - half;
    images[0] = {half, -half, 0, (int64_t)(D / 2)};
    auto show = [&](const char *what, const vector<vector<int64_t>> &v) {
        for (size_t s = 0; s < v.size(); s++) { printf("%s %zu", what, s); for (int64_t x : v[s]) printf(" %lld", (long long)x); printf("\n"); }
    };
    PlainBaseTensor enc = encryptImageSlotsCrt(images, 1, 2, 2, base, CRC_NTT);
    if (enc.parts.size() != ts.size() || enc.form() != CRC_NTT || enc.count() != 4) return 4;
    show("lifted", decryptSlotsCrt(enc, S));
    PlainBaseTensor act = rescaleSlotsCrt(enc, D, 1, cap, CRC_COEFF, false);
    show("act", decryptSlotsCrt(act, S));
    show("sym", decryptSlotsCrt(rescaleSlotsCrt(enc, D, 1, cap, CRC_NTT, true), S));
    show("rescale", decryptSlotsCrt(rescaleSlotsCrt(enc, D, 0, 0, CRC_COEFF, false), S));
    // member 0 is a tensor of the global context: its slots are the residues mod t_0; handed out and back, the tensor is what it was
    ciphertext3D part = component(act, 0);
    show("part0", decryptSlots(part, S));
    setComponent(act, 0, part);
    show("back", decryptSlotsCrt(act, S));
    int refused = 0;
    try { setComponent(act, 0, component(enc, 0)); } catch (const invalid_argument &) { refused++; }                  // another form
    try { component(act, (int)ts.size()); } catch (const invalid_argument &) { refused++; }
    try { rescaleSlotsCrt(enc, 0, 0, 0, CRC_COEFF); } catch (const invalid_argument &) { refused++; }
    try { rescaleSlotsCrt(enc, D, 0, (uint64_t)half + 1, CRC_COEFF); } catch (const invalid_argument &) { refused++; }
    try { makePlainBase({ts[0], ts[0]}); } catch (const invalid_argument &) { refused++; }
    if (ts.size() > 1) try { makePlainBase(vector<uint64_t>(ts.rbegin(), ts.rend())); } catch (const invalid_argument &) { refused++; }      // t_0 is not the parameters'
    // one modulus: encryptImageSlots -> decryptSlots
    auto one = makePlainBase({ts[0]});
    const bool same = decryptSlotsCrt(encryptImageSlotsCrt(images, 1, 2, 2, one), S) == decryptSlots(encryptImageSlots(images, 1, 2, 2), S);
    printf("one_modulus_equal %d\n", (int)same);
    printf("budget %d\n", minNoiseBudget(component(act, 0)));
    delParameters();
    setParameters(n, ts[0]);
    try { decryptSlotsCrt(enc, S); } catch (const invalid_argument &) { refused++; }                                 // a base of other parameters
    delParameters();
    printf("plain_base ok refused %d\n", refused);
    return 0;
}

static int do_api(int argc, char **argv)
{
    if (argc < 4) return 1;
    string h5 = argv[2], dir = argv[3];
    EXPECT_THROW(fraencode(1.0), logic_error);                         // context not set
    EXPECT_THROW(setParameters(4095, 1 << 20), invalid_argument);      // not a power of two
    setParameters(1024, {0x7fffffff380001ULL, 0x3fffffff000001ULL}, 1ULL << 20, 0);
    // client side round trip (encryptImage / decryptImage, globals.cpp:127-157,207-230)
    vector<float> img(28 * 28); for (int i = 0; i < 784; i++) img[i] = (float)((i % 17) - 8) / 4.0f;
    ciphertext3D ct = encryptImage(img, 1, 28, 28);
    floatCube back = decryptImage(ct);
    for (int i = 0; i < 28; i++) for (int j = 0; j < 28; j++) if (fabs(back[0][i][j] - img[i * 28 + j]) > 1e-6) { fprintf(stderr, "decrypt mismatch\n");
        return 4; }
    if (noiseBudget(ct) < 20) { fprintf(stderr, "budget too small\n"); return 4; }
    // a tiny layer stack: conv -> avgpool -> square -> fc, resident vs layerwise must give identical ciphertexts
    vector<float> w(2 * 1 * 3 * 3), b(2), fw(3 * 2 * 6 * 6), fb(3);
    for (size_t i = 0; i < w.size(); i++) w[i] = 0.05f * (float)((int)(i % 7) - 3);
    b[0] = 0.1f; b[1] = -0.2f;
    for (size_t i = 0; i < fw.size(); i++) fw[i] = 0.01f * (float)((int)(i % 11) - 5);
    fb = {0.5f, -0.25f, 0.125f};
    auto enc = [&](float v) { return fraencode((double)v); };
    plaintext4D ew(2, plaintext3D(1, plaintext2D(3, vector<Plaintext>(3)))); vector<Plaintext> eb(2);
    for (int f = 0; f < 2; f++) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) ew[f][0][i][j] = enc(w[(f * 3 + i) * 3 + j]); eb[f] = enc(b[f]); }
    plaintext2D efw(3, vector<Plaintext>(72)); vector<Plaintext> efb(3);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 72; j++) efw[i][j] = enc(fw[i * 72 + j]); efb[i] = enc(fb[i]); }
    vector<float> small(14 * 14); for (int i = 0; i < 196; i++) small[i] = (float)((i * 7) % 13 - 6) / 8.0f;
    ciphertext3D x = encryptImage(small, 1, 14, 14);
    Network net;
    net.getLayers().push_back(shared_ptr<Layer>(new ConvolutionalLayer("c", 14, 14, 1, 1, 1, 3, 3, 2, 4, ew, eb)));
    net.getLayers().push_back(shared_ptr<Layer>(new AvgPoolingLayer("p", 12, 12, 2, 2, 2, 2, 2)));
    net.getLayers().push_back(shared_ptr<Layer>(new SquareLayer("s", 2)));
    net.getLayers().push_back(shared_ptr<Layer>(new FullyConnectedLayer("f", 72, 3, 2, efw, efb)));
    net.ntt_resident = true;  vector<u64> r1 = net.forward(x).toHost();
    net.ntt_resident = false; ciphertext3D o2 = net.forward(x); vector<u64> r2 = o2.toHost();
    if (r1 != r2) { fprintf(stderr, "resident and layerwise outputs differ\n"); return 5; }
    // semantic check against float arithmetic
    floatCube dec = decryptImage(o2);
    double conv[2][12][12], pool[2][6][6];
    for (int f = 0; f < 2; f++) for (int i = 0; i < 12; i++) for (int j = 0; j < 12; j++) {
        double s = b[f];
        for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) s += (double)w[(f * 3 + a) * 3 + c] * small[(i + a) * 14 + j + c];
        conv[f][i][j] = s;
    }
    for (int f = 0; f < 2; f++) for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { double s = (conv[f][2*i][2*j] + conv[f][2*i][2*j+1] +
        conv[f][2*i+1][2*j] + conv[f][2*i+1][2*j+1]) / 4; pool[f][i][j] = s * s; }
    for (int o = 0; o < 3; o++) { double s = fb[o];
        for (int f = 0; f < 2; f++) for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) s += (double)fw[o * 72 + (f * 6 + i) * 6 + j] * pool[f][i][j];
        if (fabs(s - dec[0][o][0]) > 1e-4) { fprintf(stderr, "semantic mismatch %d: %f vs %f\n", o, s, dec[0][o][0]); return 6; } }
    // refresh path (network.cpp:30-34) keeps the result
    net.layer_before_reenc = 3; floatCube dec2 = decryptImage(net.forward(x)); net.layer_before_reenc = -1;
    for (int o = 0; o < 3; o++) if (fabs(dec2[0][o][0] - dec[0][o][0]) > 1e-4) { fprintf(stderr, "refresh changed the result\n"); return 7; }
    // fuse() and the refresh point: the refresh stays in front of the SAME layer when folds below it shift the indices, and no fold spans it.
    // [conv, avgpool, square, pool2, fc] with the refresh in front of pool2 (index 3): conv + avgpool fold (index 3 -> 2), square + pool2 must not pair up.
    {
        plaintext2D gw(3, vector<Plaintext>(50)); vector<Plaintext> gb(3);
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 50; j++) gw[i][j] = enc(fw[(i * 50 + j) % 216]); gb[i] = enc(fb[i]); }
        auto build = [&]() {
            Network nn;
            nn.getLayers().push_back(shared_ptr<Layer>(new ConvolutionalLayer("c", 14, 14, 1, 1, 1, 3, 3, 2, 4, ew, eb)));
            nn.getLayers().push_back(shared_ptr<Layer>(new AvgPoolingLayer("p", 12, 12, 2, 2, 2, 2, 2)));
            nn.getLayers().push_back(shared_ptr<Layer>(new SquareLayer("s", 2)));
            nn.getLayers().push_back(shared_ptr<Layer>(new PoolingLayer("p2", 6, 6, 2, 1, 1, 2, 2)));
            nn.getLayers().push_back(shared_ptr<Layer>(new FullyConnectedLayer("g", 50, 3, 2, gw, gb)));
            return nn;
        };
        Network plain = build(); plain.layer_before_reenc = 3;
        floatCube want = decryptImage(plain.forward(x));
        Network fusedn = build(); fusedn.layer_before_reenc = 3;
        const int removed = fusedn.fuse();
        const int at = fusedn.layer_before_reenc;
        if (at < 0 || at >= fusedn.getNumLayers() || fusedn.getLayer(at)->getName() != "p2") {
            fprintf(stderr, "fuse() moved the refresh point: %d layers removed, refresh now in front of index %d (%s)\n", removed, at,
                    at >= 0 && at < fusedn.getNumLayers() ? fusedn.getLayer(at)->getName().c_str() : "?");
            return 14;
        }
        if (at != 3 - removed) { fprintf(stderr, "refresh index %d after %d folds below it\n", at, removed); return 14; }
        floatCube got = decryptImage(fusedn.forward(x));
        for (int o = 0; o < 3; o++)
            if (fabs(got[0][o][0] - want[0][o][0]) > 1e-4) { fprintf(stderr, "fused network with a refresh differs: %f vs %f\n", got[0][o][0], want[0][o][0]);
                return 14; }
        // without a refresh the same network does pair square + pool2, bit-identically
        Network a = build(), b2 = build();
        const int removed2 = b2.fuse();
        if (removed2 <= removed) { fprintf(stderr, "square + pooling did not pair up without a refresh (%d vs %d)\n", removed2, removed); return 14; }
        if (a.forward(x).toHost() != b2.forward(x).toHost()) { fprintf(stderr, "fused network differs from the unfused one\n"); return 14; }
    }
    // save / load of the encoded parameters in SEAL's Plaintext wire format (savePlaintextParameters / istream ctor)
    { ofstream f(dir + "/enc_model.bin", ios::binary); for (int i = 0; i < net.getNumLayers(); i++) net.getLayer(i)->savePlaintextParameters(&f); }
    { ifstream f(dir + "/enc_model.bin", ios::binary);
      Network n2;
      n2.getLayers().push_back(shared_ptr<Layer>(new ConvolutionalLayer("c", 14, 14, 1, 1, 1, 3, 3, 2, 4, &f)));
      n2.getLayers().push_back(shared_ptr<Layer>(new AvgPoolingLayer("p", 12, 12, 2, 2, 2, 2, 2)));
      n2.getLayers().push_back(shared_ptr<Layer>(new SquareLayer("s", 2)));
      n2.getLayers().push_back(shared_ptr<Layer>(new FullyConnectedLayer("f", 72, 3, 2, &f)));
      if (n2.forward(x).toHost() != r1) { fprintf(stderr, "reloaded network differs\n"); return 8; } }
    // multi-GPU start-up path (Network::broadcastParameters over crc_comm / RCCL) on a one-rank communicator: the weights are unpacked,
    // "broadcast", checksummed and compared, and the network must still produce the same ciphertexts
    {
        uint8_t id[CRC_COMM_ID_BYTES]; crc_comm *comm = nullptr;
        if (crc_comm_unique_id(id) || crc_comm_create(context, 1, 0, id, &comm)) { fprintf(stderr, "crc_comm_create failed (rccl error %d)\n",
            crc_last_comm_error()); return 13; }
        const size_t bytes = net.broadcastParameters(comm, 0);
        fprintf(stderr, "broadcastParameters: %zu bytes on %d rank(s)\n", bytes, crc_comm_world(comm));
        net.ntt_resident = true;
        if (bytes == 0 || net.forward(x).toHost() != r1) { fprintf(stderr, "network differs after broadcastParameters\n"); return 13; }
        EXPECT_THROW(net.broadcastParameters(comm, 1), invalid_argument);
        crc_comm_destroy(comm);
    }
    // a dense layer with ONE input: crc_plan_mac may answer the one-channel matrix-core form for its (1, 1, 1, ...) geometry, which is a convolution's only --
    // the layer runs on the vector-ALU kernel with matrix_cores on as with it off, and gives the same words
    {
        plaintext2D ow(4, vector<Plaintext>(1)); vector<Plaintext> ob(4);
        for (int i = 0; i < 4; i++) { ow[i][0] = enc(0.25f * (float)(i - 2)); ob[i] = enc(0.125f * (float)i); }
        ciphertext3D one = encryptImage(vector<float>{0.75f}, 1, 1, 1);
        vector<u64> got[2];
        for (int on = 1; on >= 0; on--) {
            Network nn;
            nn.getLayers().push_back(shared_ptr<Layer>(new FullyConnectedLayer("one", 1, 4, 1, ow, ob)));
            nn.matrix_cores = on != 0;
            got[on] = nn.forward(one).toHost();
            const string kn = nn.getLayer(0)->kernelName();
            if (kn.find("mfma_conv1_kernel") != string::npos) { fprintf(stderr, "in_dim = 1 dense layer runs on %s\n", kn.c_str()); return 15; }
        }
        if (got[0].empty() || got[0] != got[1]) { fprintf(stderr, "in_dim = 1 dense layer: matrix_cores on and off differ\n"); return 15; }
    }
    // error behaviour mirrors the reference (std::invalid_argument on bad shapes / truncated streams)
    EXPECT_THROW(net.getLayer(0)->forward(ciphertext3D(1, 1, 10, 10)), invalid_argument);
    { istringstream empty(""); EXPECT_THROW(FullyConnectedLayer("f", 4, 2, 1, &empty), invalid_argument); }
    EXPECT_THROW(CnnBuilder("/nonexistent.h5").getPretrained("x"), runtime_error);
    // key / image files in SEAL's wire formats (setAndSaveParameters / initFromKeys / encryptAndSaveImage / loadEncryptedImage)
    {
        setDeterministicSeed(777);
        setAndSaveParameters(dir + "/pk.bin", dir + "/sk.bin", dir + "/evk.bin", 2048, 1ULL << 16);
        ciphertext3D saved = encryptAndSaveImage(small, 1, 14, 14, dir + "/img.bin");
        vector<u64> before = saved.toHost();
        setDeterministicSeed(999);                                    // a different key pair would be generated ...
        initFromKeys(dir + "/pk.bin", dir + "/sk.bin", dir + "/evk.bin", 2048, 1ULL << 16);       // ... but the files restore the first one
        ciphertext3D loaded = loadEncryptedImage(1, 14, 14, dir + "/img.bin");
        if (loaded.toHost() != before) { fprintf(stderr, "image file round trip differs\n"); return 11; }
        floatCube d3 = decryptImage(loaded);
        for (int i = 0; i < 196; i++) if (fabs(d3[0][i / 14][i % 14] - small[i]) > 1e-6) { fprintf(stderr, "decrypt after initFromKeys failed\n"); return 12; }
        EXPECT_THROW(initFromKeys(dir + "/pk.bin", dir + "/sk.bin", dir + "/evk.bin", 2048, 1ULL << 17), invalid_argument);   // hash mismatch
        setParameters(1024, {0x7fffffff380001ULL, 0x3fffffff000001ULL}, 1ULL << 20, 0);
    }
    // HDF5 loader through the builder
    CnnBuilder builder(h5);
    if (builder.getPretrained("pool1_features.conv1.weight").size() != 800) return 9;
    net.printNetworkStructure();
    delParameters();
    printf("api ok\n");
    return 0;
}

// test_host bcast <rank> <world> <rendezvous file> <out dir> [device]
//   Network::broadcastParameters across PROCESSES (one per rank; RCCL when every rank has its own GPU, the shared-memory rehearsal transport --
//   CRC_COMM_TRANSPORT=shm --
//   when they share one): rank 0 holds the real weights, every other rank builds the same topology from DIFFERENT weights, joins through the id rank 0 left in
//   the
//   file, receives -- and must then produce rank 0's output ciphertexts bit for bit (<out dir>/bcast_out_<rank>.u64)
static int do_bcast(int argc, char **argv)
{
    if (argc < 6) return 1;
    const int rank = atoi(argv[2]), world = atoi(argv[3]); const string rdv = argv[4], dir = argv[5]; const int device = argc > 6 ? atoi(argv[6]) : 0;
    setDeterministicSeed(4242);
    setParameters(1024, {0x7fffffff380001ULL, 0x3fffffff000001ULL}, 1ULL << 20, device);
    // the non-root ranks start from other weights: only the broadcast can make the outputs agree
    const float scale = rank == 0 ? 1.0f : -0.5f;
    auto enc = [&](float v) { return fraencode((double)(v * scale)); };
    plaintext4D ew(2, plaintext3D(1, plaintext2D(3, vector<Plaintext>(3)))); vector<Plaintext> eb(2);
    for (int f = 0; f < 2; f++) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) ew[f][0][i][j] = enc(0.05f * (float)(((f * 3 + i) * 3 + j) % 7 -
        3)); eb[f] = enc(f ? -0.2f : 0.1f); }
    plaintext2D efw(3, vector<Plaintext>(72)); vector<Plaintext> efb(3);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 72; j++) efw[i][j] = enc(0.01f * (float)((i * 72 + j) % 11 - 5)); efb[i] = enc(0.125f * (float)(i + 1)); }
    vector<float> small(14 * 14); for (int i = 0; i < 196; i++) small[i] = (float)((i * 7) % 13 - 6) / 8.0f;
    ciphertext3D x = encryptImage(small, 1, 14, 14);
    Network net;
    net.getLayers().push_back(shared_ptr<Layer>(new ConvolutionalLayer("c", 14, 14, 1, 1, 1, 3, 3, 2, 4, ew, eb)));
    net.getLayers().push_back(shared_ptr<Layer>(new AvgPoolingLayer("p", 12, 12, 2, 2, 2, 2, 2)));
    net.getLayers().push_back(shared_ptr<Layer>(new SquareLayer("s", 2)));
    net.getLayers().push_back(shared_ptr<Layer>(new FullyConnectedLayer("f", 72, 3, 2, efw, efb)));
    uint8_t id[CRC_COMM_ID_BYTES];
    if (rank == 0) {
        if (crc_comm_unique_id(id)) { fprintf(stderr, "crc_comm_unique_id failed (rccl error %d)\n", crc_last_comm_error()); return 13; }
        { ofstream o(rdv + ".tmp", ios::binary); o.write((const char *)id, sizeof id); }
        if (rename((rdv + ".tmp").c_str(), rdv.c_str())) return 13;
    } else {
        bool got = false;
        for (int tries = 0; tries < 1200 && !got; tries++) { ifstream f(rdv, ios::binary); got = f && f.read((char *)id, sizeof id); if (!got) usleep(100000); }
        if (!got) { fprintf(stderr, "no rendezvous id\n"); return 13; }
    }
    crc_comm *comm = nullptr;
    if (crc_comm_create(context, world, rank, id, &comm)) { fprintf(stderr, "crc_comm_create failed (rccl error %d)\n", crc_last_comm_error()); return 13; }
    const size_t bytes = net.broadcastParameters(comm, 0);
    net.ntt_resident = true;
    wr(dir + "/bcast_out_" + to_string(rank) + ".u64", net.forward(x).toHost());
    printf("bcast ok: rank %d of %d, %zu bytes\n", rank, crc_comm_world(comm), bytes);
    crc_comm_destroy(comm);
    delParameters();
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 1;
    try {
        if (!strcmp(argv[1], "bcast")) return do_bcast(argc, argv);
        if (!strcmp(argv[1], "net")) return do_net(argc, argv);
        if (!strcmp(argv[1], "netgeom")) return do_netgeom(argc, argv);
        if (!strcmp(argv[1], "net3")) return do_net3(argc, argv);
        if (!strcmp(argv[1], "netr")) return do_netr(argc, argv);
        if (!strcmp(argv[1], "plan")) return do_plan(argc, argv);
        if (!strcmp(argv[1], "encsym")) return do_encsym(argc, argv);
        if (!strcmp(argv[1], "budgetsym")) return do_budgetsym(argc, argv);
        if (!strcmp(argv[1], "seeded")) return do_seeded(argc, argv);
        if (!strcmp(argv[1], "netseeded")) return do_netseeded(argc, argv);
        if (!strcmp(argv[1], "api")) return do_api(argc, argv);
        if (!strcmp(argv[1], "files")) return do_files(argc, argv);
        if (!strcmp(argv[1], "searchlogic")) return do_searchlogic(argc, argv);
        if (!strcmp(argv[1], "search")) return do_search(argc, argv);
        if (!strcmp(argv[1], "describe")) return do_describe(argc, argv);
        if (!strcmp(argv[1], "labels")) return do_labels(argc, argv);
        if (!strcmp(argv[1], "build")) return do_build(argc, argv);
        if (!strcmp(argv[1], "multiply")) return do_multiply(argc, argv);
        if (!strcmp(argv[1], "slots_describe")) return do_slots_describe(argc, argv);
        if (!strcmp(argv[1], "slots_build")) return do_slots_build(argc, argv);
        if (!strcmp(argv[1], "slots_rescale_plan")) return do_slots_rescale_plan(argc, argv);
        if (!strcmp(argv[1], "slots_act_plan")) return do_slots_act_plan(argc, argv);
        if (!strcmp(argv[1], "build_plain")) return do_build_plain(argc, argv);
        if (!strcmp(argv[1], "plain_base")) return do_plain_base(argc, argv);
    } catch (const exception &e) { fprintf(stderr, "exception: %s\n", e.what()); return 10; }
    return 1;
}
