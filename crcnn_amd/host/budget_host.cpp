// budget_host.cpp -- the noise-budget profile of a real batch: one profiled Network::forward on seeded synthetic images, written as a small JSON file.
//
// usage: budget_host <model.h5> <n> <k> <t> <batch> <seed> <outdir> [description]
//   <model.h5>  the model file; its base name is the topology (PlainModelTiny | ApproxPlainModel | PlainModelWoPad) unless the path of a description file
//               follows as the last argument (28 x 28 one-channel inputs: the images are the synthetic digits)
//   <n> <k>     ring size and the first k primes of coeff_modulus_128(n); <t> the plain modulus
//   <batch>     seeded MNIST-like images (the generator of crcnn_amd/synth.py), encrypted under the deterministic seed <seed>
// Writes <outdir>/budget_<model>_n<n>_k<k>_b<batch>.json:
//   layers                    the layer names
//   layer_budget_min/_first   Network::last_layer_budget_min / _first of a forward with profile_budget (coefficient form between the layers, so every layer's
//                             tensor can be measured: the ciphertexts are those of the NTT-resident forward)
//   layer_budget_resident_*   the same from the NTT-resident forward (tensors measured in NTT form)
//   layer_budget_host_first   noiseBudget(output) -- the host routine on ciphertext 0 -- after every layer called one by one
//   output_budgets            noiseBudgets(output): every output ciphertext of every image; output_min / output_min_index: minNoiseBudget
//   scope                     the budget-checking forward (max_num_of_reencryptions = 1) with budget_scope 0 and 1: whether the two output tensors are the same
//                             bits and how many values each refreshed; and a copy of the output with ONE exhausted ciphertext (uniform residues) at index 5:
//                             minNoiseBudget and its index, noiseBudget(t) before and after
//   packed_forms_rejected     noiseBudgets / minNoiseBudget throw std::invalid_argument for CRC_NTTP and CRC_NTTL tensors
//   search_status             PlainModulusSearch::testPlainModulus at <t> on the first two images (exit_status_forward: 0 SUCCESS, 1 OUT_OF_BUDGET, 2 MISPREDICTED),
//                             with whole_batch_budget off and on
#include "crcnn_host.h"
#include "plain_modulus_search.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
using namespace std;

static uint64_t splitmix(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// synth.synth_image + synth.normalize: 81 % background, the rest uniform in 1..255; (p / 255 - 0.1307) / 0.3081 in float32
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
static string list(const vector<int> &v)
{
    ostringstream o; o << "[";
    for (size_t i = 0; i < v.size(); i++) o << (i ? ", " : "") << v[i];
    o << "]"; return o.str();
}

int main(int argc, char **argv)
{
    if (argc != 8 && argc != 9) { fprintf(stderr, "usage: %s <model.h5> <n> <k> <t> <batch> <seed> <outdir> [description]\n", argv[0]); return 1; }
    const string h5 = argv[1], outdir = argv[7];
    const int n = atoi(argv[2]), k = atoi(argv[3]), batch = atoi(argv[5]);
    const uint64_t t = strtoull(argv[4], 0, 0), seed = strtoull(argv[6], 0, 0);
    string model = h5.substr(h5.find_last_of('/') + 1);
    if (model.size() > 3 && model.substr(model.size() - 3) == ".h5") model.resize(model.size() - 3);
    const string label = model;                               // names the output file
    if (argc == 9) model = argv[8];
    try {
        if (n < 1 || k < 1 || batch < 1) throw invalid_argument("bad sizes");
        uint64_t q[16];
        if (crc_default_coeff_modulus_128(n, q, 16) < k) throw invalid_argument("coeff_modulus_128(n) has fewer primes than asked for");
        setDeterministicSeed(seed);
        setParameters(n, vector<uint64_t>(q, q + k), t, 0);
        CnnBuilder build(h5);
        ostringstream f;
        {                                                     // (every tensor and the network go before the search below sets the parameters again)
        Network net = build.buildNetworkByName(model);
        if (net.input_zd != 1 || net.input_xd != 28 || net.input_yd != 28) throw invalid_argument("the synthetic images are 1 x 28 x 28");
        vector<ciphertext3D> imgs;
        for (int b = 0; b < batch; b++) imgs.push_back(encryptImage(synthImage(b), 1, 28, 28));
        const ciphertext3D x = stackImages(imgs);
        imgs.clear();
        const int L = net.getNumLayers();

        // the profile: coefficient form between the layers (every tensor measurable), then NTT-resident (packed / limb hand-overs show as -1)
        net.profile_budget = true;
        net.ntt_resident = false;
        const ciphertext3D out = net.forward(x);
        const vector<int> lmin = net.last_layer_budget_min, lfirst = net.last_layer_budget_first;
        net.ntt_resident = true;
        const ciphertext3D out_res = net.forward(x);
        const vector<int> rmin = net.last_layer_budget_min, rfirst = net.last_layer_budget_first;
        net.profile_budget = false;
        const bool resident_same = out.toHost() == out_res.toHost();
        // the host routine on ciphertext 0 behind every layer
        vector<int> host_first;
        {
            ciphertext3D a = x;
            for (int i = 0; i < L; i++) { net.layers[i]->out_form = CRC_COEFF; a = net.layers[i]->forward(a); host_first.push_back(noiseBudget(a)); }
        }
        const vector<int> budgets = noiseBudgets(out);
        size_t where = 0;
        const int omin = minNoiseBudget(out, &where);

        // the two scopes of the budget-checking forward
        net.max_num_of_reencryptions = 1; net.keep_reenc_values = true;
        net.budget_scope = 0;
        const vector<uint64_t> s0 = net.forward(x).toHost(); const size_t refreshed0 = net.last_reenc_values.size();
        net.budget_scope = 1;
        const vector<uint64_t> s1 = net.forward(x).toHost(); const size_t refreshed1 = net.last_reenc_values.size();
        // one exhausted ciphertext where scope 0 does not look
        const size_t bad_index = 5, ctw = crc_ct_words(context, 2);
        vector<uint64_t> h = out.toHost();
        {
            uint64_t s = seed ^ 0xBADC0DEULL;
            for (int p = 0; p < 2; p++) for (int i = 0; i < k; i++) for (int c = 0; c < n; c++) h[bad_index * ctw + ((size_t)p * k + i) * n + c] = splitmix(s) % q[i];
        }
        const ciphertext3D spoiled = ciphertext3D::fromHost(h.data(), out.B, out.zd, out.xd, out.yd);
        size_t bad_where = 0;
        const int bad_min = minNoiseBudget(spoiled, &bad_where);
        const int nb_before = noiseBudget(out), nb_after = noiseBudget(spoiled);

        // the packed and limb forms cannot be measured: both whole-tensor calls refuse them
        bool rejected = true;
        for (int form : {CRC_NTTP, CRC_NTTL}) {
            const ciphertext3D p(1, 1, 1, 1, form);
            try { noiseBudgets(p); rejected = false; } catch (const invalid_argument &) {}
            try { minNoiseBudget(p); rejected = false; } catch (const invalid_argument &) {}
        }
        f << "{\"model\": \"" << label << "\", \"n\": " << n << ", \"k\": " << k << ", \"t\": " << t << ", \"batch\": " << batch << ", \"seed\": " << seed << ",\n";
        f << " \"layers\": [";
        for (int i = 0; i < L; i++) f << (i ? ", " : "") << "\"" << net.layers[i]->getName() << "\"";
        f << "],\n";
        f << " \"layer_budget_min\": " << list(lmin) << ",\n \"layer_budget_first\": " << list(lfirst) << ",\n";
        f << " \"layer_budget_resident_min\": " << list(rmin) << ",\n \"layer_budget_resident_first\": " << list(rfirst) << ",\n";
        f << " \"resident_output_identical\": " << (resident_same ? "true" : "false") << ",\n";
        f << " \"layer_budget_host_first\": " << list(host_first) << ",\n";
        f << " \"output_shape\": [" << out.B << ", " << out.zd << ", " << out.xd << ", " << out.yd << "],\n";
        f << " \"output_budgets\": " << list(budgets) << ",\n \"output_min\": " << omin << ", \"output_min_index\": " << where << ",\n";
        f << " \"scope\": {\"identical\": " << (s0 == s1 ? "true" : "false") << ", \"same_as_plain_forward\": " << (s0 == out.toHost() ? "true" : "false")
          << ", \"refreshed_values\": [" << refreshed0 << ", " << refreshed1 << "], \"exhausted_index\": " << bad_index << ", \"min\": " << bad_min
          << ", \"where\": " << bad_where << ", \"noise_budget_before\": " << nb_before << ", \"noise_budget_after\": " << nb_after << "},\n";
        f << " \"packed_forms_rejected\": " << (rejected ? "true" : "false") << ",\n";
        }
        // one candidate of the plain-modulus search on the first two images, with the reference's check and with the whole batch's
        {
            PlainModulusSearch s;
            s.model = model; s.max_poly_modulus = n; s.coeff_modulus.assign(q, q + k); s.seed = (unsigned)seed;
            for (int b = 0; b < min(batch, 2); b++) s.test_set.push_back(synthImage(b));
            s.predictWithPlainModel(h5);
            const int first = (int)s.testPlainModulus(build, t, (int)s.test_set.size());
            s.whole_batch_budget = true;
            const int whole = (int)s.testPlainModulus(build, t, (int)s.test_set.size());
            f << " \"search_status\": {\"first_ciphertext\": " << first << ", \"whole_batch\": " << whole << "}}\n";
        }
        const string path = outdir + "/budget_" + label + "_n" + to_string(n) + "_k" + to_string(k) + "_b" + to_string(batch) + ".json";
        ofstream o(path);
        o << f.str();
        o.close();
        if (!o) throw runtime_error("cannot write " + path);
        cout << "wrote " << path << endl;
        delParameters();
        return 0;
    } catch (const exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
