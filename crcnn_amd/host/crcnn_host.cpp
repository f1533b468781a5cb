// crcnn_host.cpp -- implementation of the CrCNN-compatible C++ host classes on top of the C ABI (include/crcnn_hip.h).
#include "crcnn_host.h"
#include "diag_plan.h"
#include "refresh_pass.h"
#include "../csrc/host_parallel.h"          // std::thread ranges (header only; no other csrc internals are used here: the engine is reached through the C ABI)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <list>
#include <mutex>
#include <sstream>

using namespace std;

crc_ctx *context = nullptr;
// The stream every ABI call of these classes is launched on.  NULL (the default stream) unless the caller installs its own (setStream): a driver that uploads
// the next chunk of encrypted images on a second stream while this one computes (bench_host's streamed inputs) needs a non-blocking one here -- the default
// stream would order itself against every other blocking stream of the process.  A global like the context, the keys and the work buffer
// (CrCNN/src/globals.h:18-26).
static void *g_stream = nullptr;
static uint64_t g_generation = 0;                          // counts delParameters(): what a Level (below) was made under
void setStream(void *s) { g_stream = s; }
void *getStream() { return g_stream; }
static inline void *stream() { return g_stream; }
vector<uint64_t> secret_key, public_key, ev_keys16_host;
shared_ptr<DeviceBuffer> ev_keys16;
vector<uint64_t> galois_elts, galois_keys_host;
static shared_ptr<DeviceBuffer> g_galois_keys;              // the key blobs of galois_elts, dbc g_galois_dbc, resident in HBM
static shared_ptr<DeviceBuffer> g_galois_ckeys;             // their conjugated blobs (crc_galois_conjugate_keys_dev): the keys of the hoisted rotations
static shared_ptr<DeviceBuffer> g_galois_pkeys;             // their prepared form (crc_galois_prepare_keys_dev), made by the first densePlanes that can use it
static int g_galois_dbc = 0;
static bool g_det = false;                                  // setDeterministicSeed(): tests / bench only
static uint64_t g_det_seed = 0;
static uint8_t g_master_key[CRC_KEY_BYTES];                 // fresh from the OS on every setParameters()
static uint64_t g_enc_counter = 0;                          // ciphertexts encrypted under g_master_key so far (= next keystream id)
// slot encoding (setSlotEncoding): scalar plaintexts instead of the fractional encoder
static bool g_slot_on = false;
static int g_slot_in_bits = 0, g_slot_w_bits = 0;
static uint64_t g_plain_modulus = 0;                        // t of the current context
static double g_enc_scale[2] = {0, 0};                      // slot encoding: scales of the first / second dataset of the layer CnnBuilder builds next
void setDeterministicSeed(uint64_t seed) { g_det = true; g_det_seed = seed; }
void clearDeterministicSeed() { g_det = false; }

// ---- status -> exception (the reference throws std::invalid_argument from SEAL, evaluator.cpp:1549-1556) ---------------
static void chk(int status, const char *what)
{
    if (status >= 0) return;
    string msg = string(what) + ": " + crc_strerror(status);
    if (status == CRC_ERR_INVALID_ARGUMENT || status == CRC_ERR_PARAMETERS) throw invalid_argument(msg);
    throw runtime_error(msg);
}
static crc_ctx *ctx()
{
    if (!context) throw logic_error("setParameters() must be called first");
    return context;
}
static int N() { return crc_ctx_n(ctx()); }
static int K() { return crc_ctx_k(ctx()); }
static size_t ctBytes() { return crc_ct_words(ctx(), 2) * 8; }
static uint64_t *ctAt(const ciphertext3D &t, size_t i) { return t.data() + i * crc_ct_words(ctx(), 2); }

// The randomness of `ids` keystream ids, drawn where they are spent.  Under setDeterministicSeed: a seed, fresh per draw.  Otherwise the master key from the
// counter: one keystream per ciphertext, never reused under this key.  Either way the counter moves past the ids
struct Randomness {
    bool det; uint64_t seed, stream_base;
    // one call of an entry point's seed / key pair: with(f, randomness...) puts the seed, or the key and its stream base, into f's argument list
    template <class Seeded, class Keyed, class With> void call(Seeded seeded, const char *seeded_name, Keyed keyed, const char *keyed_name, With &&with) const
    {
        if (det) chk(with(seeded, seed), seeded_name);
        else chk(with(keyed, (const uint8_t *)g_master_key, stream_base), keyed_name);
    }
};
#define ABI(f) f, #f
static Randomness drawRandomness(size_t ids)
{
    const Randomness r{g_det, g_det_seed + 1000003 * (g_enc_counter + 1), g_enc_counter};
    g_enc_counter += ids;
    return r;
}

// Device allocations are recycled by exact size: the reference passes its tensors by value and so do these classes -- every Layer::forward makes a new output
// tensor -- but a hipMalloc / hipFree pair per layer and chunk (the free synchronises the device) would cost more than some of the layers.  Freed buffers wait
// in a pool (bounded: beyond the cap they go back to the driver; an allocation that fails empties the pool and tries again); delParameters() empties it.
namespace {
bool windowOk(int xd, int yd, int xs, int ys, int xf, int yf);          // (with the description parser, below)
struct BufferPool {
    std::mutex mu;
    std::list<std::pair<size_t, void *>> lru;               // oldest first
    size_t pooled = 0;
    static constexpr size_t kCap = (size_t)128 << 30, kReserve = (size_t)16 << 30;
    void *take(size_t b)
    {
        std::lock_guard<std::mutex> g(mu);
        for (auto it = lru.begin(); it != lru.end(); ++it) if (it->first == b) { void *p = it->second; lru.erase(it); pooled -= b; return p; }
        return nullptr;
    }
    // the newest buffer stays; the least recently returned ones (the one-off scratch of model building, typically) make room for it
    bool give(size_t b, void *p)
    {
        std::lock_guard<std::mutex> g(mu);
        if (b > kCap) return false;
        while (pooled + b > kCap && !lru.empty()) { if (context) crc_free(context, lru.front().second); pooled -= lru.front().first; lru.pop_front(); }
        // ... and the device keeps kReserve free for allocations that do not come through here (the HIP runtime's scratch for spilling kernels, RCCL)
        size_t free_b = 0, total_b = 0;
        while (context && crc_mem_info(context, &free_b, &total_b) >= 0 && free_b < kReserve && !lru.empty()) { crc_free(context, lru.front().second);
            pooled -= lru.front().first; lru.pop_front(); }
        if (context && free_b < kReserve) return false;
        lru.emplace_back(b, p); pooled += b;
        return true;
    }
    void flush() { std::lock_guard<std::mutex> g(mu); for (auto &e : lru) if (context) crc_free(context, e.second); lru.clear(); pooled = 0; }
};
BufferPool g_pool;
}
DeviceBuffer::DeviceBuffer(size_t b) : bytes(b)
{
    const size_t want = b ? b : 8;
    if ((ptr = g_pool.take(want))) return;
    static const bool trace = getenv("CRC_HOST_TRACE") != nullptr;
    if (trace) fprintf(stderr, "[host] hipMalloc %.3f GiB (pool miss)\n", want / 1073741824.0);
    if (crc_malloc(ctx(), want, &ptr) >= 0) return;
    g_pool.flush();
    chk(crc_malloc(ctx(), want, &ptr), "crc_malloc");
}
DeviceBuffer::~DeviceBuffer()
{
    if (!ptr || !context) return;
    if (g_pool.give(bytes ? bytes : 8, ptr)) return;
    if (getenv("CRC_HOST_TRACE")) fprintf(stderr, "[host] hipFree %.3f GiB (pool full)\n", bytes / 1073741824.0);
    crc_free(context, ptr);
}

// ---- Plaintext ------------------------------------------------------------------------------------------------------
void Plaintext::dense(uint64_t *out, int n) const
{
    memset(out, 0, 8 * (size_t)n);
    for (auto &p : nz) if (p.first < n) out[p.first] = p.second;
}
void Plaintext::save(ostream &stream) const
{
    int32_t cc = coeff_count_;
    vector<uint64_t> d((size_t)max(cc, 0), 0);
    for (auto &p : nz) if (p.first < cc) d[p.first] = p.second;
    stream.write(reinterpret_cast<const char *>(&cc), sizeof cc);
    stream.write(reinterpret_cast<const char *>(d.data()), (streamsize)d.size() * 8);
}
void Plaintext::load(istream &stream)
{
    int32_t cc = 0;
    stream.read(reinterpret_cast<char *>(&cc), sizeof cc);
    if (!stream || cc < 0 || cc > N() + 1) throw invalid_argument("plain is not valid for encryption parameters");
    vector<uint64_t> d((size_t)cc);
    stream.read(reinterpret_cast<char *>(d.data()), (streamsize)cc * 8);
    if (!stream) throw invalid_argument("truncated plaintext stream");
    coeff_count_ = cc; nz.clear();
    for (int i = 0; i < cc; i++) if (d[i]) nz.emplace_back(i, d[i]);
}
static Plaintext fromDense(const uint64_t *co, int n, int cc)
{
    Plaintext p; p.coeff_count_ = cc;
    for (int i = 0; i < n; i++) if (co[i]) p.nz.emplace_back(i, co[i]);
    return p;
}
// slot encoding: the constant polynomial nearbyint(value * scale) mod t -- the same number in every slot
static Plaintext scalarPlain(double value, double scale)
{
    const double r = nearbyint(value * scale);
    if (!(fabs(r) < 9.2e18)) throw invalid_argument("slot encoding: value * scale does not fit an int64");
    long long v = (long long)r % (long long)g_plain_modulus;
    if (v < 0) v += (long long)g_plain_modulus;
    Plaintext p; p.coeff_count_ = 1;
    if (v) p.nz.emplace_back(0, (uint64_t)v);
    return p;
}
// the one switch between the two encodings: scale 0 = the fractional encoder
static Plaintext encodeScaled(double value, double scale) { return scale != 0 ? scalarPlain(value, scale) : fraencode(value); }
void setSlotEncoding(int input_bits, int weight_bits)
{
    if (!crc_slots_supported(ctx())) throw invalid_argument("setSlotEncoding: the plain modulus must be a prime that is 1 mod 2n and none of the engine's moduli");
    if (input_bits < 0 || input_bits > 30 || weight_bits < 0 || weight_bits > 30) throw invalid_argument("setSlotEncoding: bit counts must be in 0..30");
    g_slot_on = true; g_slot_in_bits = input_bits; g_slot_w_bits = weight_bits;
}
void clearSlotEncoding() { g_slot_on = false; g_enc_scale[0] = g_enc_scale[1] = 0; }
bool slotEncoding() { return g_slot_on; }
Plaintext fraencode(double value)
{
    vector<uint64_t> co((size_t)N()); int32_t cc = 0;
    chk(crc_encode_f64(ctx(), &value, 1, co.data(), &cc), "crc_encode_f64");
    return fromDense(co.data(), N(), cc);
}
double fradecode(const vector<uint64_t> &plain) { return crc_decode(ctx(), plain.data()); }

// plaintext list -> device buffer of [count][k][n]: mode 0 = NTT-form weights, 1 = delta coefficient form, 2 = delta NTT form; mode 3 = the plaintext
// coefficients themselves, [count][n] (streamed layers)
static shared_ptr<DeviceBuffer> uploadPlain(const vector<const Plaintext *> &pl, int mode)
{
    const int n = N(), k = mode == 3 ? 1 : K();
    auto out = make_shared<DeviceBuffer>(pl.size() * (size_t)k * n * 8);
    const size_t chunk = max<size_t>(1, min<size_t>(pl.size(), (64u << 20) / ((size_t)n * 8)));
    DeviceBuffer stage(chunk * (size_t)n * 8), cstage(chunk * (size_t)CRC_PLAIN_COMPACT_WORDS * 8);
    vector<uint64_t> host, chost(chunk * (size_t)CRC_PLAIN_COMPACT_WORDS);
    for (size_t o = 0; o < pl.size(); o += chunk) {
        const size_t c = min(chunk, pl.size() - o);
        // what the fractional encoder produces has non-zero coefficients only at 0..63 and n-32..n-1: such plaintexts travel in compact form (96 words each,
        // crc_plain_expand zero-extends them on the device); anything else -- a plaintext loaded from a file may be arbitrary -- goes down dense
        atomic<bool> compact{true};
        crc_host::parallel_for(c, 64, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; i++) {
                uint64_t *row = chost.data() + i * CRC_PLAIN_COMPACT_WORDS;
                memset(row, 0, sizeof(uint64_t) * CRC_PLAIN_COMPACT_WORDS);
                for (auto &z : pl[o + i]->nz) {
                    if (z.first < CRC_PLAIN_COMPACT_LOW) row[z.first] = z.second;
                    else if (z.first >= n - CRC_PLAIN_COMPACT_HIGH && z.first < n) row[CRC_PLAIN_COMPACT_LOW + z.first - (n - CRC_PLAIN_COMPACT_HIGH)] =
                        z.second;
                    else { compact = false; return; }
                }
            }
        });
        if (compact) {
            chk(crc_memcpy_h2d(ctx(), cstage.ptr, chost.data(), c * (size_t)CRC_PLAIN_COMPACT_WORDS * 8, stream()), "crc_memcpy_h2d");
            chk(crc_plain_expand(ctx(), (const uint64_t *)cstage.ptr, c, (uint64_t *)stage.ptr, stream()), "crc_plain_expand");
        } else {
            host.resize(chunk * (size_t)n);
            crc_host::parallel_for(c, 64, [&](size_t b, size_t e) { for (size_t i = b; i < e; i++) pl[o + i]->dense(host.data() + i * n, n); });
            chk(crc_memcpy_h2d(ctx(), stage.ptr, host.data(), c * (size_t)n * 8, stream()), "crc_memcpy_h2d");
        }
        uint64_t *dst = (uint64_t *)out->ptr + o * (size_t)k * n;
        if (mode == 3) chk(crc_memcpy_d2d(ctx(), dst, stage.ptr, c * (size_t)n * 8, stream()), "crc_memcpy_d2d");
        else if (mode == 0) chk(crc_plain_to_ntt(ctx(), (const uint64_t *)stage.ptr, c, dst, stream()), "crc_plain_to_ntt");
        else chk(crc_plain_to_delta(ctx(), (const uint64_t *)stage.ptr, c, mode == 2 ? CRC_NTT : CRC_COEFF, dst, stream()), "crc_plain_to_delta");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    }
    return out;
}

// ---- tensors ---------------------------------------------------------------------------------------------------------- Network::forward's two ping-pong
// activation slots: the NEXT tensor constructed on this thread takes (and, if it is too small, replaces) the slot the hint points at instead of a buffer of its
// own -- every layer constructs its output tensor first.  With 200 GiB of weights resident there is no room for a recycling pool, and a hipMalloc / hipFree
// pair per layer costs more than most layers (PlainModelWoPad at n = 16384: 113 ms instead of 3.8 ms per image for conv1).
static thread_local shared_ptr<DeviceBuffer> *g_out_hint = nullptr;
// arms the hint for ONE layer call and disarms it when the scope ends, however it ends: a layer that throws before it has constructed its output must not leave
// the hint pointing at the network's slot for whatever tensor the caller constructs next (an encryptImage in a retry, or a slot of a Network that no longer
// exists)
struct OutHint {
    explicit OutHint(shared_ptr<DeviceBuffer> *slot) { g_out_hint = slot; }
    ~OutHint() { g_out_hint = nullptr; }
    OutHint(const OutHint &) = delete; OutHint &operator=(const OutHint &) = delete;
};

ciphertext3D::ciphertext3D(int B, int zd, int xd, int yd, int form) : B(B), zd(zd), xd(xd), yd(yd), form(form)
{
    size_t bytes = count() * ctBytes();
    if (form == CRC_NTTLC) { const size_t lb = crc_limb_tensor_bytes(ctx(), B, zd, xd, yd); if (lb > bytes) bytes = lb; }      // channels padded to 32
    // a dense consumer's limb tensor: every output a channel of ONE position, rounded up to 32 (7 bytes per residue: larger than the ciphertexts below 217
    // channels)
    if (form == CRC_NTTL || form == CRC_NTTLS) { const size_t lb = crc_limb_tensor_bytes(ctx(), B, zd * xd * yd, 1, 1); if (lb > bytes) bytes = lb; }
    if (g_out_hint) {
        shared_ptr<DeviceBuffer> *slot = g_out_hint; g_out_hint = nullptr;
        if (!*slot || (*slot)->bytes < bytes) { slot->reset(); *slot = make_shared<DeviceBuffer>(bytes); }
        buf = *slot;
        return;
    }
    buf = make_shared<DeviceBuffer>(bytes);
}
ciphertext3D ciphertext3D::images(int b0, int count) const
{
    if (!buf || b0 < 0 || count < 1 || b0 + count > B) throw invalid_argument("ciphertext3D::images: range outside the batch");
    if (form == CRC_NTTL || form == CRC_NTTLC || form == CRC_NTTLS) throw invalid_argument("ciphertext3D::images: a limb tensor is laid out for its whole batch");
    ciphertext3D v; v.B = count; v.zd = zd; v.xd = xd; v.yd = yd; v.form = form; v.buf = buf;
    v.offset = offset + (size_t)b0 * zd * xd * yd * ctBytes();
    return v;
}
ciphertext3D ciphertext3D::fromHost(const uint64_t *h, int B, int zd, int xd, int yd)
{
    ciphertext3D t(B, zd, xd, yd);
    chk(crc_memcpy_h2d(ctx(), t.buf->ptr, h, t.count() * ctBytes(), stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return t;
}
vector<uint64_t> ciphertext3D::toHost() const
{
    vector<uint64_t> h(count() * ctBytes() / 8);
    chk(crc_memcpy_d2h(ctx(), h.data(), data(), h.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return h;
}
ciphertext3D stackImages(const vector<ciphertext3D> &images)
{
    if (images.empty()) throw invalid_argument("no images");
    const ciphertext3D &f = images[0];
    int B = 0;
    for (auto &im : images) {
        if (im.zd != f.zd || im.xd != f.xd || im.yd != f.yd || im.form != f.form) throw invalid_argument("image shapes differ");
        B += im.B;
    }
    ciphertext3D t(B, f.zd, f.xd, f.yd, f.form);
    size_t off = 0;
    for (auto &im : images) { chk(crc_memcpy_d2d(ctx(), (char *)t.data() + off, im.data(), im.count() * ctBytes(), stream()), "crc_memcpy_d2d");
        off += im.count() * ctBytes(); }
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return t;
}
ciphertext3D deepCopyImage(const ciphertext3D &image)
{
    ciphertext3D t(image.B, image.zd, image.xd, image.yd, image.form);
    chk(crc_memcpy_d2d(ctx(), t.data(), image.data(), image.count() * ctBytes(), stream()), "crc_memcpy_d2d");
    return t;
}

// ---- globals ----------------------------------------------------------------------------------------------------------
void setParameters(int poly_modulus, uint64_t plain_modulus)
{
    uint64_t q[16];
    int k = crc_default_coeff_modulus_128(poly_modulus, q, 16);            // parms->set_coeff_modulus(coeff_modulus_128(n)), globals.cpp:30
    if (k < 0) throw invalid_argument("no default coeff_modulus for this poly_modulus");
    setParameters(poly_modulus, vector<uint64_t>(q, q + k), plain_modulus, 0);
}
void setParameters(int poly_modulus, const vector<uint64_t> &coeff_modulus, uint64_t plain_modulus, int device)
{
    delParameters();
    chk(crc_ctx_create(poly_modulus, coeff_modulus.data(), (int)coeff_modulus.size(), plain_modulus, device, &context),
        "encryption parameters are not set correctly");
    g_plain_modulus = plain_modulus;
    const int n = N(), k = K();
    secret_key.assign((size_t)k * n, 0); public_key.assign((size_t)2 * k * n, 0);
    ev_keys16_host.assign(crc_evk_words(context, 16), 0);                  // keygen->generate_evaluation_keys(16, *ev_keys16), globals.cpp:54
    g_enc_counter = 0;
    if (g_det) {
        chk(crc_keygen(context, g_det_seed, secret_key.data(), public_key.data()), "crc_keygen");
        chk(crc_gen_evk(context, g_det_seed + 1, secret_key.data(), 16, ev_keys16_host.data()), "crc_gen_evk");
    } else {
        chk(crc_random_key(g_master_key), "crc_random_key");
        chk(crc_keygen_key(context, g_master_key, secret_key.data(), public_key.data()), "crc_keygen_key");
        chk(crc_gen_evk_key(context, g_master_key, secret_key.data(), 16, ev_keys16_host.data()), "crc_gen_evk_key");
    }
    ev_keys16 = make_shared<DeviceBuffer>(ev_keys16_host.size() * 8);
    chk(crc_memcpy_h2d(context, ev_keys16->ptr, ev_keys16_host.data(), ev_keys16_host.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(context, stream()), "crc_stream_sync");
}
// One kernel scratch area for every layer of the process: layers run one after another on one stream, so their scratch never overlaps in
// time, and the largest request decides the size (a per-layer buffer summed to ~40 GiB at WoPad 16384 beside the 182 GiB limb weights).
static shared_ptr<DeviceBuffer> g_scratch;
// limb-form tile buffers of the streamed layers (one set serves every streamed layer: they run one after the other)
static shared_ptr<DeviceBuffer> g_wltile, g_xltile;
// device copies of the client's keys (secret key for the refresh, public key for every encryption); uploaded on first use, dropped with the parameters
// (the host vectors are public globals, as in the reference: a caller may assign them -- a fingerprint of the words decides whether the copy is current)
static shared_ptr<DeviceBuffer> g_d_sk, g_d_pk;
static uint64_t g_d_sk_fp = 0, g_d_pk_fp = 0;
static const uint64_t *deviceKey(shared_ptr<DeviceBuffer> &d, uint64_t &fp, const vector<uint64_t> &h, const char *what)
{
    if (h.empty()) throw logic_error(string("setParameters() or initFromKeys() must be called first (") + what + ")");
    uint64_t f = 0x9e3779b97f4a7c15ULL ^ h.size();
    for (uint64_t w : h) f = (f ^ w) * 0xff51afd7ed558ccdULL + (f >> 29);
    if (!d || d->bytes != h.size() * 8 || f != fp) {
        fp = f;
        d = make_shared<DeviceBuffer>(h.size() * 8);
        chk(crc_memcpy_h2d(ctx(), d->ptr, h.data(), h.size() * 8, stream()), "crc_memcpy_h2d");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // the host vector may change after this call returns
    }
    return (const uint64_t *)d->ptr;
}

void delParameters()
{
    g_generation++;                                         // levels made under these parameters are stale from here on
    ev_keys16.reset();
    g_galois_keys.reset(); g_galois_ckeys.reset(); g_galois_pkeys.reset(); galois_elts.clear(); galois_keys_host.clear(); g_galois_dbc = 0;
    g_d_sk.reset(); g_d_pk.reset();
    g_scratch.reset(); g_wltile.reset(); g_xltile.reset();
    g_pool.flush();
    clearSlotEncoding();
    if (context) { crc_ctx_destroy(context); context = nullptr; }
}
static void writeFile(const string &path, const vector<uint8_t> &b) { ofstream f(path, ofstream::binary); if (!f) throw runtime_error("cannot write " + path);
    f.write((const char *)b.data(), (streamsize)b.size()); }
static vector<uint8_t> readFile(const string &path)
{
    ifstream f(path, ifstream::binary); if (!f) throw runtime_error("cannot open " + path);
    f.seekg(0, ios::end); size_t sz = (size_t)f.tellg(); f.seekg(0); vector<uint8_t> b(sz); f.read((char *)b.data(), (streamsize)sz); return b;
}
void setAndSaveParameters(string public_key_path, string secret_key_path, string evaluation_key_path, int poly_modulus, uint64_t plain_modulus)
{   // globals.cpp:58-74
    setParameters(poly_modulus, plain_modulus);
    size_t w = 0;
    vector<uint8_t> b(crc_seal_pk_bytes(context)); chk(crc_seal_pk_save(context, public_key.data(), b.data(), b.size(), &w), "crc_seal_pk_save");
        writeFile(public_key_path, b);
    b.assign(crc_seal_sk_bytes(context), 0); chk(crc_seal_sk_save(context, secret_key.data(), b.data(), b.size(), &w), "crc_seal_sk_save");
        writeFile(secret_key_path, b);
    b.assign(crc_seal_evk_bytes(context, 16), 0); chk(crc_seal_evk_save(context, ev_keys16_host.data(), 16, b.data(), b.size(), &w), "crc_seal_evk_save");
        writeFile(evaluation_key_path, b);
}
void initFromKeys(string public_key_path, string secret_key_path, string evaluation_key_path, int poly_modulus, uint64_t plain_modulus)
{   // globals.cpp:77-111
    setParameters(poly_modulus, plain_modulus);
    vector<uint8_t> b = readFile(public_key_path); chk(crc_seal_pk_load(context, b.data(), b.size(), public_key.data()),
        "public_key is not valid for encryption parameters");
    b = readFile(secret_key_path); chk(crc_seal_sk_load(context, b.data(), b.size(), secret_key.data()), "secret_key is not valid for encryption parameters");
    b = readFile(evaluation_key_path); int dbc = 0;
    chk(crc_seal_evk_load(context, b.data(), b.size(), ev_keys16_host.data(), &dbc), "evaluation_keys is not valid for encryption parameters");
    if (dbc != 16) throw invalid_argument("evaluation keys must have decomposition_bit_count 16");
    chk(crc_memcpy_h2d(context, ev_keys16->ptr, ev_keys16_host.data(), ev_keys16_host.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(context, stream()), "crc_stream_sync");
    g_d_sk.reset(); g_d_pk.reset();
}
ciphertext3D encryptAndSaveImage(vector<float> image, int zd, int xd, int yd, string file_name)
{   // globals.cpp:174-190: the ciphertexts back to back in Ciphertext::save format
    ciphertext3D t = encryptImage(image, zd, xd, yd);
    vector<uint64_t> h = t.toHost();
    const size_t one = crc_seal_ct_bytes(ctx(), 2), ctw = crc_ct_words(ctx(), 2);
    vector<uint8_t> b(one * t.count()); size_t w = 0;
    for (size_t i = 0; i < t.count(); i++) chk(crc_seal_ct_save(ctx(), h.data() + i * ctw, 2, b.data() + i * one, one, &w), "crc_seal_ct_save");
    writeFile(file_name, b);
    return t;
}
ciphertext3D loadEncryptedImage(int zd, int xd, int yd, string file_name)
{   // globals.cpp:193-205
    vector<uint8_t> b = readFile(file_name);
    const size_t cnt = (size_t)zd * xd * yd, ctw = crc_ct_words(ctx(), 2);
    vector<uint64_t> h(cnt * ctw); size_t off = 0;
    for (size_t i = 0; i < cnt; i++) { int size = 0; size_t used = 0;
        chk(crc_seal_ct_load(ctx(), b.data() + off, b.size() - off, h.data() + i * ctw, 2, &size, &used), "encrypted is not valid for encryption parameters");
        if (size != 2) throw invalid_argument("expected size-2 ciphertexts");
        off += used; }
    return ciphertext3D::fromHost(h.data(), 1, zd, xd, yd);
}
// encode on the host, encrypt on the device (crc_encrypt_dev: Encryptor::encrypt, encryptor.cpp:71-134)
static ciphertext3D encryptPixels(const vector<float> &px, int zd, int xd, int yd)
{
    const int n = N();
    vector<uint64_t> pl(px.size() * n);
    chk(crc_encode_f32(ctx(), px.data(), px.size(), pl.data(), nullptr), "crc_encode_f32");
    DeviceBuffer d_pl(pl.size() * 8), d_work(crc_encrypt_dev_work_bytes(ctx(), px.size()));
    const uint64_t *d_pk = deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    chk(crc_memcpy_h2d(ctx(), d_pl.ptr, pl.data(), pl.size() * 8, stream()), "crc_memcpy_h2d");
    ciphertext3D out(1, zd, xd, yd, CRC_COEFF);
    drawRandomness(px.size()).call(ABI(crc_encrypt_dev), ABI(crc_encrypt_dev_key), [&](auto f, auto... rnd) {
        return f(ctx(), d_pk, (const uint64_t *)d_pl.ptr, px.size(), rnd..., (uint64_t *)out.buf->ptr, d_work.ptr, stream()); });
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return out;
}
ciphertext3D encryptImage(vector<float> image, int zd, int xd, int yd)
{
    if ((int)image.size() < xd * yd) throw invalid_argument("image too small");
    // the reference indexes image[i*xd+j] for every z (globals.cpp:133): one plane replicated over zd
    vector<float> px((size_t)zd * xd * yd);
    for (int z = 0; z < zd; z++) for (int i = 0; i < xd; i++) for (int j = 0; j < yd; j++) px[((size_t)z * xd + i) * yd + j] = image[(size_t)i * xd + j];
    return encryptPixels(px, zd, xd, yd);
}
ciphertext3D encryptImage(floatCube image)
{
    const int zd = (int)image.size(), xd = (int)image[0].size(), yd = (int)image[0][0].size();
    vector<float> px; px.reserve((size_t)zd * xd * yd);
    for (auto &a : image) for (auto &b : a) for (float v : b) px.push_back(v);
    return encryptPixels(px, zd, xd, yd);
}
// encode on the host, encrypt under the secret key on the device (crc_encrypt_sym_dev); one keystream id per ciphertext from the counter encryptImage uses
ciphertext3D encryptImageSymmetric(const vector<float> &px, int zd, int xd, int yd, int out_form)
{
    const size_t per = (size_t)zd * xd * yd;
    if (zd < 1 || xd < 1 || yd < 1 || px.empty() || px.size() % per) throw invalid_argument("encryptImageSymmetric: pixels must be [B][zd][xd][yd]");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("encryptImageSymmetric: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    const int n = N();
    vector<uint64_t> pl(px.size() * n);
    chk(crc_encode_f32(ctx(), px.data(), px.size(), pl.data(), nullptr), "crc_encode_f32");
    DeviceBuffer d_pl(pl.size() * 8), d_work(crc_encrypt_sym_dev_work_bytes(ctx(), px.size()));
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    chk(crc_memcpy_h2d(ctx(), d_pl.ptr, pl.data(), pl.size() * 8, stream()), "crc_memcpy_h2d");
    ciphertext3D out((int)(px.size() / per), zd, xd, yd, out_form);
    drawRandomness(px.size()).call(ABI(crc_encrypt_sym_dev_forms), ABI(crc_encrypt_sym_dev_key_forms), [&](auto f, auto... rnd) {
        return f(ctx(), d_sk, (const uint64_t *)d_pl.ptr, px.size(), rnd..., out_form, (uint64_t *)out.buf->ptr, d_work.ptr, stream()); });
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return out;
}
ciphertext3D encryptImageSymmetric(floatCube image, int out_form)
{
    const int zd = (int)image.size(), xd = (int)image[0].size(), yd = (int)image[0][0].size();
    vector<float> px; px.reserve((size_t)zd * xd * yd);
    for (auto &a : image) for (auto &b : a) for (float v : b) px.push_back(v);
    return encryptImageSymmetric(px, zd, xd, yd, out_form);
}
// ---- seeded images: the c0 rows and a public seed (encryption on the host threads or on the device; the server expands on the device) ----
// pixels up at 4 bytes each, encoded and encrypted on the installed stream (crc_encrypt_f32_seeded_dev[_key]), the packed rows down: the host path's seeds
static void encryptSeededOnDevice(const vector<float> &px, SeededImages &out)
{
    DeviceBuffer d_px(px.size() * 4), d_c0(out.c0.size() * 8), d_work(crc_encrypt_f32_seeded_dev_work_bytes(ctx(), px.size()));
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    chk(crc_memcpy_h2d(ctx(), d_px.ptr, px.data(), px.size() * 4, stream()), "crc_memcpy_h2d");
    const Randomness r = drawRandomness(px.size());
    if (r.det) {
        chk(crc_seeded_public_seed(r.seed, out.seed), "crc_seeded_public_seed");
        out.stream_base = 0;
        chk(crc_encrypt_f32_seeded_dev(ctx(), d_sk, (const float *)d_px.ptr, px.size(), r.seed, (uint64_t *)d_c0.ptr, d_work.ptr, stream()),
            "crc_encrypt_f32_seeded_dev");
    } else {
        chk(crc_random_key(out.seed), "crc_random_key");
        out.stream_base = r.stream_base;
        chk(crc_encrypt_f32_seeded_dev_key(ctx(), d_sk, (const float *)d_px.ptr, px.size(), g_master_key, out.seed, out.stream_base, (uint64_t *)d_c0.ptr,
                                           d_work.ptr, stream()), "crc_encrypt_f32_seeded_dev_key");
    }
    chk(crc_memcpy_d2h(ctx(), out.c0.data(), d_c0.ptr, out.c0.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
}
SeededImages encryptImageSeeded(const vector<float> &px, int zd, int xd, int yd, bool on_device)
{
    const size_t per = (size_t)zd * xd * yd;
    if (zd < 1 || xd < 1 || yd < 1 || px.empty() || px.size() % per) throw invalid_argument("encryptImageSeeded: pixels must be [B][zd][xd][yd]");
    const int n = N();
    SeededImages out;
    out.B = (int)(px.size() / per); out.zd = zd; out.xd = xd; out.yd = yd;
    out.c0.resize(px.size() * (size_t)K() * n);
    if (on_device) {
        encryptSeededOnDevice(px, out);
        return out;
    }
    vector<uint64_t> pl(px.size() * n);
    chk(crc_encode_f32(ctx(), px.data(), px.size(), pl.data(), nullptr), "crc_encode_f32");
    const Randomness r = drawRandomness(px.size());
    if (r.det) {
        chk(crc_seeded_public_seed(r.seed, out.seed), "crc_seeded_public_seed");
        out.stream_base = 0;
        chk(crc_encrypt_sym_seeded(ctx(), secret_key.data(), pl.data(), px.size(), r.seed, out.c0.data()), "crc_encrypt_sym_seeded");
    } else {
        chk(crc_random_key(out.seed), "crc_random_key");
        out.stream_base = r.stream_base;
        chk(crc_encrypt_sym_seeded_key(ctx(), secret_key.data(), pl.data(), px.size(), g_master_key, out.seed, out.stream_base, out.c0.data()),
            "crc_encrypt_sym_seeded_key");
    }
    return out;
}
SeededImages encryptImageSeeded(floatCube image, bool on_device)
{
    const int zd = (int)image.size(), xd = (int)image[0].size(), yd = (int)image[0][0].size();
    vector<float> px; px.reserve((size_t)zd * xd * yd);
    for (auto &a : image) for (auto &b : a) for (float v : b) px.push_back(v);
    return encryptImageSeeded(px, zd, xd, yd, on_device);
}
void SeededImages::save(ostream &os) const
{
    if (c0.size() != count() * (size_t)K() * N()) throw invalid_argument("SeededImages::save: rows do not match the dimensions");
    const int32_t dims[4] = {B, zd, xd, yd};
    vector<uint8_t> b(crc_seeded_ct_bytes(ctx(), count())); size_t w = 0;
    chk(crc_seeded_ct_save(ctx(), c0.data(), count(), seed, stream_base, b.data(), b.size(), &w), "crc_seeded_ct_save");
    os.write((const char *)dims, sizeof dims); os.write((const char *)b.data(), (streamsize)b.size());
    if (!os) throw runtime_error("SeededImages::save: write failed");
}
void SeededImages::load(istream &is)
{
    int32_t dims[4] = {0, 0, 0, 0};
    is.read((char *)dims, sizeof dims);
    if (!is || dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[3] < 1) throw invalid_argument("SeededImages::load: not a seeded image file");
    const size_t cnt = (size_t)dims[0] * dims[1] * dims[2] * dims[3];
    vector<uint8_t> b(crc_seeded_ct_bytes(ctx(), cnt));
    is.read((char *)b.data(), (streamsize)b.size());
    if (!is) throw invalid_argument("SeededImages::load: file shorter than its dimensions say");
    vector<uint64_t> rows(cnt * (size_t)K() * N()); size_t got = 0; uint8_t sd[32]; uint64_t base = 0;
    chk(crc_seeded_ct_load(ctx(), b.data(), b.size(), rows.data(), cnt, &got, sd, &base), "seeded images are not valid for encryption parameters");
    if (got != cnt) throw invalid_argument("SeededImages::load: count does not match the dimensions");
    B = dims[0]; zd = dims[1]; xd = dims[2]; yd = dims[3]; c0.swap(rows); memcpy(seed, sd, 32); stream_base = base;
}
void expandSeeded(const uint64_t *d_c0, int B, int zd, int xd, int yd, const uint8_t *seed, uint64_t stream_base, ciphertext3D &dst)
{
    if (!d_c0 || !seed || !dst.buf || dst.B != B || dst.zd != zd || dst.xd != xd || dst.yd != yd)
        throw invalid_argument("expandSeeded: destination tensor does not match the dimensions");
    if (dst.form != CRC_COEFF && dst.form != CRC_NTT) throw invalid_argument("expandSeeded: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    chk(crc_seeded_expand_dev(ctx(), d_c0, dst.count(), seed, stream_base, dst.form, dst.data(), stream()), "crc_seeded_expand_dev");
}
ciphertext3D expandSeeded(const SeededImages &im, int out_form)
{
    if (im.count() == 0 || im.c0.size() != im.count() * (size_t)K() * N()) throw invalid_argument("expandSeeded: rows do not match the dimensions");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("expandSeeded: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    DeviceBuffer d_c0(im.c0.size() * 8);
    chk(crc_memcpy_h2d(ctx(), d_c0.ptr, im.c0.data(), im.c0.size() * 8, stream()), "crc_memcpy_h2d");
    ciphertext3D out(im.B, im.zd, im.xd, im.yd, out_form);
    expandSeeded((const uint64_t *)d_c0.ptr, im.B, im.zd, im.xd, im.yd, im.seed, im.stream_base, out);
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");     // the packed rows and the host vector are released here
    return out;
}
// ---- slot-batched client side ------------------------------------------------------------------------------------------------
ciphertext3D encryptImageSlots(const vector<vector<int64_t>> &images, int zd, int xd, int yd, int out_form)
{
    if (!g_slot_on) throw logic_error("encryptImageSlots: setSlotEncoding() must be called first");
    const size_t per = (size_t)zd * xd * yd, S = images.size();
    if (zd < 1 || xd < 1 || yd < 1 || S < 1 || S > (size_t)N()) throw invalid_argument("encryptImageSlots: 1 to n images of [zd][xd][yd] pixels");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("encryptImageSlots: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    vector<int64_t> h(S * per);
    for (size_t j = 0; j < S; j++) {
        if (images[j].size() != per) throw invalid_argument("encryptImageSlots: every image must have zd xd yd pixels");
        memcpy(h.data() + j * per, images[j].data(), per * 8);
    }
    DeviceBuffer d_v(h.size() * 8), d_pl(per * (size_t)N() * 8), d_work(crc_encrypt_dev_work_bytes(ctx(), per));
    const uint64_t *d_pk = deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    chk(crc_memcpy_h2d(ctx(), d_v.ptr, h.data(), h.size() * 8, stream()), "crc_memcpy_h2d");
    // image-major: pixel c of image j at h[j per + c]
    chk(crc_slots_compose_dev(ctx(), (const int64_t *)d_v.ptr, per, (int)S, 1, per, (uint64_t *)d_pl.ptr, stream()), "crc_slots_compose_dev");
    ciphertext3D out(1, zd, xd, yd, out_form);
    drawRandomness(per).call(ABI(crc_encrypt_dev_forms), ABI(crc_encrypt_dev_key_forms), [&](auto f, auto... rnd) {
        return f(ctx(), d_pk, (const uint64_t *)d_pl.ptr, per, rnd..., out_form, out.data(), d_work.ptr, stream()); });
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return out;
}
ciphertext3D encryptImageSlots(const vector<vector<float>> &images, int zd, int xd, int yd, int out_form)
{
    if (!g_slot_on) throw logic_error("encryptImageSlots: setSlotEncoding() must be called first");
    const double scale = ldexp(1.0, g_slot_in_bits);
    vector<vector<int64_t>> q(images.size());
    for (size_t j = 0; j < images.size(); j++) {
        q[j].resize(images[j].size());
        for (size_t i = 0; i < images[j].size(); i++) {
            const double r = nearbyint((double)images[j][i] * scale);
            if (!(fabs(r) < 9.2e18)) throw invalid_argument("encryptImageSlots: a pixel does not fit an int64 at this scale");
            q[j][i] = (int64_t)r;
        }
    }
    return encryptImageSlots(q, zd, xd, yd, out_form);
}
vector<vector<int64_t>> decryptSlots(const ciphertext3D &t, int S)
{
    if (!t.buf || t.count() == 0) throw invalid_argument("decryptSlots: empty tensor");
    if (t.form != CRC_COEFF && t.form != CRC_NTT) throw invalid_argument("decryptSlots: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (S < 1 || S > N()) throw invalid_argument("decryptSlots: 1 to n slots");
    const size_t cnt = t.count();
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    DeviceBuffer d_pl(cnt * (size_t)N() * 8), d_v(cnt * (size_t)S * 8), d_work(crc_decrypt_dev_work_bytes(ctx(), cnt, 2, t.form));
    chk(crc_decrypt_dev(ctx(), d_sk, t.data(), cnt, 2, t.form, (uint64_t *)d_pl.ptr, d_work.ptr, stream()), "crc_decrypt_dev");
    chk(crc_slots_decompose_dev(ctx(), (const uint64_t *)d_pl.ptr, cnt, S, (int64_t *)d_v.ptr, 1, cnt, stream()), "crc_slots_decompose_dev");
    vector<int64_t> h(cnt * (size_t)S);
    chk(crc_memcpy_d2h(ctx(), h.data(), d_v.ptr, h.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    vector<vector<int64_t>> out(S);
    for (int j = 0; j < S; j++) out[j].assign(h.begin() + (size_t)j * cnt, h.begin() + (size_t)(j + 1) * cnt);
    return out;
}
vector<vector<double>> decryptImageSlots(const ciphertext3D &t, int S, double scale)
{
    if (!(scale > 0)) throw invalid_argument("decryptImageSlots: the scale must be positive (Network::slot_scale())");
    const vector<vector<int64_t>> v = decryptSlots(t, S);
    vector<vector<double>> out(v.size());
    for (size_t j = 0; j < v.size(); j++) { out[j].resize(v[j].size()); for (size_t i = 0; i < v[j].size(); i++) out[j][i] = (double)v[j][i] / scale; }
    return out;
}
// ---- Galois keys, rotations, slot sums ------------------------------------------------------------------------------------
static shared_ptr<DeviceBuffer> &ensure(shared_ptr<DeviceBuffer> &b, size_t bytes);
void generateGaloisKeys(int dbc, vector<uint64_t> elts)
{
    if (secret_key.empty()) throw logic_error("cannot generate galois keys for unspecified secret key");
    if (dbc < 1 || dbc > 60) throw invalid_argument("decomposition_bit_count is not in the valid range");
    for (uint64_t g : elts) if (!crc_galois_elt_valid(ctx(), g)) throw invalid_argument("galois element is not valid");
    vector<uint64_t> keys(elts.size() * crc_evk_words(ctx(), dbc));
    // a domain of its own in the key generator's streams (the element in the nonce): the master key, or the deterministic seed next to the evaluation keys'
    if (g_det) chk(crc_gen_galois_keys(ctx(), g_det_seed + 2, secret_key.data(), dbc, elts.data(), (int)elts.size(), keys.data()), "crc_gen_galois_keys");
    else chk(crc_gen_galois_keys_key(ctx(), g_master_key, secret_key.data(), dbc, elts.data(), (int)elts.size(), keys.data()), "crc_gen_galois_keys_key");
    g_galois_keys = make_shared<DeviceBuffer>(keys.size() * 8 + 8);
    chk(crc_memcpy_h2d(ctx(), g_galois_keys->ptr, keys.data(), keys.size() * 8, stream()), "crc_memcpy_h2d");
    // the conjugated blobs beside them, made on the device element by element (g = 1 has no key to conjugate: its blob is never read)
    g_galois_ckeys = make_shared<DeviceBuffer>(keys.size() * 8 + 8);
    const size_t kw = crc_evk_words(ctx(), dbc);
    for (size_t e = 0; e < elts.size(); e++)
        if (elts[e] != 1) chk(crc_galois_conjugate_keys_dev(ctx(), &elts[e], 1, dbc, (const uint64_t *)g_galois_keys->ptr + e * kw,
                                                            (uint64_t *)g_galois_ckeys->ptr + e * kw, stream()), "crc_galois_conjugate_keys_dev");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    galois_elts = std::move(elts); galois_keys_host = std::move(keys); g_galois_dbc = dbc;
    g_galois_pkeys.reset();
}
void generateGaloisKeys(int dbc)
{
    vector<uint64_t> elts(crc_galois_default_elts(ctx(), nullptr, 0));
    chk(crc_galois_default_elts(ctx(), elts.data(), (int)elts.size()), "crc_galois_default_elts");
    generateGaloisKeys(dbc, elts);
}
// ---- seeded Galois keys: the client makes the first rows, the server expands them on the device ----
SeededKeys generateGaloisKeysSeeded(int dbc, vector<uint64_t> elts, bool on_device)
{
    if (secret_key.empty()) throw logic_error("cannot generate galois keys for unspecified secret key");
    if (dbc < 1 || dbc > 60) throw invalid_argument("decomposition_bit_count is not in the valid range");
    for (uint64_t g : elts) if (!crc_galois_elt_valid(ctx(), g)) throw invalid_argument("galois element is not valid");
    SeededKeys out;
    out.dbc = dbc; out.rows.resize(elts.size() * crc_seeded_key_words(ctx(), dbc));
    const int ne = (int)elts.size();
    // the streams carry the element, dbc and k in their nonce (chacha.h) and nothing per call: the PUBLIC seed must be the same whenever the master key serves an
    // element again (a rotation set, then a layer's elements that share 3), or two sets would hold equal e around different A and first - first' = -(A - A') s
    // is the secret key.  So the seed is a function of the master key -- the first half of its keystream block under CHACHA_DOM_KSK_SEED, a PRF output that says
    // nothing about the key -- and a repeated element is the same key byte for byte, as it is under generateGaloisKeys.  (Deterministic mode: the seed's own.)
    if (g_det) chk(crc_seeded_public_seed(g_det_seed + 2, out.seed), "crc_seeded_public_seed");
    else {
        const uint8_t nonce[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 11 /* CHACHA_DOM_KSK_SEED << 24, little-endian */};
        uint8_t block[64];
        chk(crc_chacha20_block(g_master_key, 0, nonce, block), "crc_chacha20_block");
        memcpy(out.seed, block, 32);
    }
    if (on_device) {
        DeviceBuffer d_first(out.rows.size() * 8 + 16);
        const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
        if (g_det) chk(crc_gen_keys_seeded_dev(ctx(), g_det_seed + 2, d_sk, dbc, elts.data(), ne, (uint64_t *)d_first.ptr, stream()), "crc_gen_keys_seeded_dev");
        else chk(crc_gen_keys_seeded_dev_key(ctx(), g_master_key, out.seed, d_sk, dbc, elts.data(), ne, (uint64_t *)d_first.ptr, stream()), "crc_gen_keys_seeded_dev_key");
        if (!out.rows.empty()) chk(crc_memcpy_d2h(ctx(), out.rows.data(), d_first.ptr, out.rows.size() * 8, stream()), "crc_memcpy_d2h");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    } else if (g_det) chk(crc_gen_keys_seeded(ctx(), g_det_seed + 2, secret_key.data(), dbc, elts.data(), ne, out.rows.data()), "crc_gen_keys_seeded");
    else chk(crc_gen_keys_seeded_key(ctx(), g_master_key, out.seed, secret_key.data(), dbc, elts.data(), ne, out.rows.data()), "crc_gen_keys_seeded_key");
    out.ids = std::move(elts);
    return out;
}
void installGaloisKeys(const SeededKeys &keys)
{
    if (keys.dbc < 1 || keys.dbc > 60) throw invalid_argument("decomposition_bit_count is not in the valid range");
    for (uint64_t g : keys.ids) if (!crc_galois_elt_valid(ctx(), g)) throw invalid_argument("galois element is not valid");
    const size_t ne = keys.ids.size(), rw = crc_seeded_key_words(ctx(), keys.dbc), kw = crc_evk_words(ctx(), keys.dbc);
    if (keys.rows.size() != ne * rw) throw invalid_argument("installGaloisKeys: rows do not match the elements");
    DeviceBuffer d_rows(ne * rw * 8 + 16);
    if (ne) chk(crc_memcpy_h2d(ctx(), d_rows.ptr, keys.rows.data(), ne * rw * 8, stream()), "crc_memcpy_h2d");
    auto plain = make_shared<DeviceBuffer>(ne * kw * 8 + 8), conj = make_shared<DeviceBuffer>(ne * kw * 8 + 8);
    chk(crc_seeded_keys_expand_dev(ctx(), (const uint64_t *)d_rows.ptr, keys.ids.data(), (int)ne, keys.dbc, keys.seed, 0, (uint64_t *)plain->ptr, stream()),
        "crc_seeded_keys_expand_dev");
    // the conjugated blobs beside them, run by run between the elements 1 (g = 1 has no key to conjugate: its blob is never read)
    for (size_t e0 = 0; e0 < ne;) {
        if (keys.ids[e0] == 1) { e0++; continue; }
        size_t e1 = e0; while (e1 < ne && keys.ids[e1] != 1) e1++;
        chk(crc_seeded_keys_expand_dev(ctx(), (const uint64_t *)d_rows.ptr + e0 * rw, keys.ids.data() + e0, (int)(e1 - e0), keys.dbc, keys.seed, 1,
                                       (uint64_t *)conj->ptr + e0 * kw, stream()), "crc_seeded_keys_expand_dev");
        e0 = e1;
    }
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    g_galois_keys = plain; g_galois_ckeys = conj; g_galois_pkeys.reset();
    galois_elts = keys.ids; galois_keys_host.clear(); g_galois_dbc = keys.dbc;
}
void SeededKeys::save(ostream &os) const
{
    if (dbc < 1 || dbc > 60 || rows.size() != ids.size() * crc_seeded_key_words(ctx(), dbc)) throw invalid_argument("SeededKeys::save: rows do not match the elements");
    vector<uint8_t> b(crc_seeded_keys_bytes(ctx(), dbc, (int)ids.size())); size_t w = 0;
    chk(crc_seeded_keys_save(ctx(), rows.data(), ids.data(), (int)ids.size(), dbc, seed, b.data(), b.size(), &w), "crc_seeded_keys_save");
    os.write((const char *)b.data(), (streamsize)b.size());
    if (!os) throw runtime_error("SeededKeys::save: write failed");
}
void SeededKeys::load(istream &is)
{
    // the header says how long the container is (uint32 dbc at offset 12, uint64 n_ids at offset 48 of its 88 bytes), and it is not trusted: magic, version and
    // parameter hash are checked before its count sizes anything, and the payload is read in bounded pieces, so memory follows the bytes that really arrive
    vector<uint8_t> b(88);
    is.read((char *)b.data(), 88);
    if (!is) throw invalid_argument("SeededKeys::load: not a seeded key file");
    uint32_t version = 0, d = 0; uint64_t cnt = 0, hash[4];
    memcpy(&version, b.data() + 8, 4); memcpy(&d, b.data() + 12, 4); memcpy(&cnt, b.data() + 48, 8);
    chk(crc_params_hash(ctx(), hash), "crc_params_hash");
    if (memcmp(b.data(), "CRCSKEY\0", 8) || version != 1) throw invalid_argument("SeededKeys::load: not a seeded key file");
    if (memcmp(b.data() + 16, hash, 32)) throw invalid_argument("seeded keys are not valid for encryption parameters");
    const size_t total = cnt <= (1u << 24) ? crc_seeded_keys_bytes(ctx(), (int)d, (int)cnt) : 0;
    if (total < 88) throw invalid_argument("SeededKeys::load: not a seeded key file");
    for (size_t at = 88; at < total;) {
        const size_t piece = min<size_t>(total - at, (size_t)64 << 20);
        b.resize(at + piece);
        is.read((char *)b.data() + at, (streamsize)piece);
        if (!is) throw invalid_argument("SeededKeys::load: file shorter than its header says");
        at += piece;
    }
    vector<uint64_t> r(cnt * crc_seeded_key_words(ctx(), (int)d)), id(cnt); int got = 0, gd = 0; uint8_t sd[32];
    // (the size query first: an empty set has no rows to point at)
    chk(crc_seeded_keys_load(ctx(), b.data(), b.size(), nullptr, nullptr, 0, &got, &gd, nullptr), "seeded keys are not valid for encryption parameters");
    if (cnt) chk(crc_seeded_keys_load(ctx(), b.data(), b.size(), r.data(), id.data(), (int)cnt, &got, &gd, sd), "seeded keys are not valid for encryption parameters");
    else memcpy(sd, b.data() + 56, 32);
    dbc = gd; ids.swap(id); rows.swap(r); memcpy(seed, sd, 32);
}
// what the three operations share: the checks in the reference's order, the result tensor, the scratch.  mode 0 rotate_rows(steps), 1 rotate_columns, 2 the slot sum
static ciphertext3D galoisOp(const char *what, const ciphertext3D &t, int mode, int steps, int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    if (!t.buf) throw invalid_argument(string(what) + ": empty tensor");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument(string(what) + ": ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (mode == 0 && !crc_galois_elt_rows(ctx(), steps)) throw invalid_argument("step count too large");
    const uint64_t *d_gk = g_galois_keys ? (const uint64_t *)g_galois_keys->ptr : nullptr;
    const int dbc = g_galois_dbc ? g_galois_dbc : 16, ne = (int)galois_elts.size();
    if (mode == 0 || mode == 1) {                           // (the planner on the host: a missing key is the reference's exception, not a status)
        int plan[64];
        const uint64_t g = mode == 0 ? crc_galois_elt_rows(ctx(), steps) : crc_galois_elt_columns(ctx());
        if (crc_galois_plan(ctx(), g, galois_elts.data(), ne, plan, 64) < 0) throw invalid_argument("galois key not present");
    }
    ciphertext3D out(t.B, t.zd, t.xd, t.yd, out_form);
    const size_t cnt = t.count();
    ensure(g_scratch, mode == 2 ? crc_sum_slots_work_bytes(ctx(), cnt, dbc) : crc_apply_galois_work_bytes(ctx(), cnt, dbc));
    int rc;
    if (mode == 0) rc = crc_rotate_rows_forms(ctx(), t.data(), t.form, cnt, steps, d_gk, galois_elts.data(), ne, dbc, out.data(), out_form, g_scratch->ptr, stream());
    else if (mode == 1) rc = crc_rotate_columns_forms(ctx(), t.data(), t.form, cnt, d_gk, galois_elts.data(), ne, dbc, out.data(), out_form, g_scratch->ptr, stream());
    else rc = crc_sum_slots_forms(ctx(), t.data(), t.form, cnt, d_gk, galois_elts.data(), ne, dbc, out.data(), out_form, g_scratch->ptr, stream());
    if (mode == 2 && rc == CRC_ERR_INVALID_ARGUMENT) throw invalid_argument("galois key not present");      // (every other argument was checked above)
    chk(rc, what);
    return out;
}
ciphertext3D rotateRows(const ciphertext3D &t, int steps, int out_form) { return galoisOp("rotateRows", t, 0, steps, out_form); }
ciphertext3D rotateColumns(const ciphertext3D &t, int out_form) { return galoisOp("rotateColumns", t, 1, 0, out_form); }
ciphertext3D sumSlots(const ciphertext3D &t, int out_form) { return galoisOp("sumSlots", t, 2, 0, out_form); }
// ---- hoisted rotations and the matrix-vector product over slots ------------------------------------------------------------
// the conjugated keys of the set on the device (null before generateGaloisKeys), and the digit width they were made with
static const uint64_t *galoisCkeys() { return g_galois_ckeys ? (const uint64_t *)g_galois_ckeys->ptr : nullptr; }
static int galoisDbc() { return g_galois_dbc ? g_galois_dbc : 16; }
// what the two share: the reference's checks in rotateRows' order, then every step's element with its own conjugated key in the set
static vector<uint64_t> hoistedElements(const char *what, const ciphertext3D &t, const vector<int> &steps, int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    if (!t.buf) throw invalid_argument(string(what) + ": empty tensor");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument(string(what) + ": ciphertext forms only (CRC_COEFF / CRC_NTT)");
    vector<uint64_t> gs;
    for (int s : steps) {
        const uint64_t g = crc_galois_elt_rows(ctx(), s);
        if (!g) throw invalid_argument("step count too large");
        if (g != 1 && find(galois_elts.begin(), galois_elts.end(), g) == galois_elts.end()) throw invalid_argument("galois key not present");
        gs.push_back(g);
    }
    return gs;
}
vector<ciphertext3D> rotateRowsMany(const ciphertext3D &t, const vector<int> &steps, int out_form)
{
    const vector<uint64_t> gs = hoistedElements("rotateRowsMany", t, steps, out_form);
    if (gs.empty()) return {};
    const int R = (int)gs.size(), dbc = galoisDbc();
    if ((long long)R * t.B > 0x7fffffffLL) throw invalid_argument("rotateRowsMany: too many results");
    ciphertext3D all(R * t.B, t.zd, t.xd, t.yd, out_form);              // [R][count]: one buffer, handed out as R views
    const size_t cnt = t.count();
    ensure(g_scratch, crc_rotate_hoisted_work_bytes(ctx(), cnt, R, dbc));
    chk(crc_rotate_hoisted_forms(ctx(), t.data(), t.form, cnt, gs.data(), R, galoisCkeys(), galois_elts.data(), (int)galois_elts.size(), dbc,
                                 all.data(), out_form, g_scratch->ptr, stream()), "rotateRowsMany");
    vector<ciphertext3D> out;
    for (int r = 0; r < R; r++) out.push_back(all.images(r * t.B, t.B));
    return out;
}
void diagMatvecPlan(const vector<vector<int64_t>> &W, int M, int n, vector<int> &steps, vector<int64_t> &rows)
{
    if (!crc_diag_plan(W, M, n, steps, rows)) throw invalid_argument("matvecSlots: M must be a power of two <= n/2 and W at most M x M");
}
// R rows of n slot values each -> their NTT-form plaintexts [R][k][n] on the device: compose, upload, transform
static shared_ptr<DeviceBuffer> plainRowsNtt(const vector<int64_t> &rows, int R)
{
    const int n = N(), k = crc_ctx_k(ctx());
    vector<uint64_t> plain((size_t)R * n);
    chk(crc_slots_compose(ctx(), rows.data(), R, n, n, 1, plain.data()), "crc_slots_compose");
    DeviceBuffer d_plain(plain.size() * 8);
    auto d_p = make_shared<DeviceBuffer>((size_t)R * k * n * 8);
    chk(crc_memcpy_h2d(ctx(), d_plain.ptr, plain.data(), plain.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_plain_to_ntt(ctx(), (const uint64_t *)d_plain.ptr, R, (uint64_t *)d_p->ptr, stream()), "crc_plain_to_ntt");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // (the composed rows and their upload go out of scope here)
    return d_p;
}
ciphertext3D matvecSlots(const ciphertext3D &t, const vector<vector<int64_t>> &W, int M, int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    const int n = N();
    vector<int> steps; vector<int64_t> rows;
    diagMatvecPlan(W, M, n, steps, rows);
    const vector<uint64_t> gs = hoistedElements("matvecSlots", t, steps, out_form);
    ciphertext3D out(t.B, t.zd, t.xd, t.yd, out_form);
    const size_t cnt = t.count(), ctb = crc_ct_words(ctx(), 2) * 8;
    if (gs.empty()) {                                                   // W = 0: the transparent zero ciphertext, as the sum of no terms
        chk(crc_memset(ctx(), out.data(), 0, cnt * ctb, stream()), "crc_memset");
        return out;
    }
    const int R = (int)gs.size(), dbc = galoisDbc();
    const shared_ptr<DeviceBuffer> d_p = plainRowsNtt(rows, R);
    ensure(g_scratch, crc_diag_mac_work_bytes(ctx(), cnt, R, dbc));
    chk(crc_diag_mac_forms(ctx(), t.data(), t.form, cnt, gs.data(), R, (const uint64_t *)d_p->ptr, galoisCkeys(), galois_elts.data(),
                           (int)galois_elts.size(), dbc, out.data(), out_form, g_scratch->ptr, stream()), "matvecSlots");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // (the diagonals' buffers go out of scope here)
    return out;
}
// baby-step / giant-step: the same product with B + M/B rotations instead of M (crc_diag_mac_bsgs_forms).  The default split is the power of two B >= M/B nearest
// the square root: the fewest keys, and the fastest of sqrt(M) / 2, sqrt(M), 2 sqrt(M) at every shape of profiles/matvec_bsgs.md
void bsgsMatvecPlan(const vector<vector<int64_t>> &W, int M, int n, int B, vector<int> &baby_steps, vector<int> &giant_steps, vector<int64_t> &rows)
{
    if (!crc_bsgs_plan(W, M, n, B, baby_steps, giant_steps, rows))
        throw invalid_argument("matvecSlotsBsgs: M must be a power of two <= n/2, B a power of two <= M and W at most M x M");
}
int bsgsDefaultSplit(int M)
{
    int B = 1;
    while ((long long)B * B < M) B *= 2;
    return B;
}
ciphertext3D matvecSlotsBsgs(const ciphertext3D &t, const vector<vector<int64_t>> &W, int M, int B, int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    const int n = N();
    vector<int> baby, giant; vector<int64_t> rows;
    bsgsMatvecPlan(W, M, n, B ? B : bsgsDefaultSplit(M), baby, giant, rows);
    const vector<uint64_t> gb = hoistedElements("matvecSlotsBsgs", t, baby, out_form), gg = hoistedElements("matvecSlotsBsgs", t, giant, out_form);
    ciphertext3D out(t.B, t.zd, t.xd, t.yd, out_form);
    const size_t cnt = t.count(), ctb = crc_ct_words(ctx(), 2) * 8;
    if (gg.empty()) {                                                   // W = 0: the transparent zero ciphertext, as the sum of no terms
        chk(crc_memset(ctx(), out.data(), 0, cnt * ctb, stream()), "crc_memset");
        return out;
    }
    const int nb = (int)gb.size(), ng = (int)gg.size(), dbc = galoisDbc();
    const shared_ptr<DeviceBuffer> d_p = plainRowsNtt(rows, nb * ng);
    ensure(g_scratch, crc_diag_mac_bsgs_work_bytes(ctx(), cnt, nb, ng, dbc));
    chk(crc_diag_mac_bsgs_forms(ctx(), t.data(), t.form, cnt, gb.data(), nb, gg.data(), ng, (const uint64_t *)d_p->ptr, galoisCkeys(),
                                galois_elts.data(), (int)galois_elts.size(), dbc, out.data(), out_form, g_scratch->ptr, stream()), "matvecSlotsBsgs");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // (the rows' buffers go out of scope here)
    return out;
}
// ---- the packed convolution: one channel plane per ciphertext ---------------------------------------------------------------
// (the general planner: at origin = 0, pad = 0, stride = 1, pool_stride = pool it is crc_conv_slots_plan field for field)
static ConvSlotsGeomPlan convSlotsPlan(const SlotPlanes &g)
{
    ConvSlotsGeomPlan P;
    if (!crc_conv_slots_plan_geom(N(), g.M, g.pitch, g.origin, g.H, g.W, g.fh, g.fw, g.dil, g.pad, g.stride, g.pool, g.pool_stride, P))
        throw invalid_argument("convSlots: M must be a power of two <= n/2, the plane must fit it with the margin its pad needs and the window must leave an output");
    return P;
}
SlotPlanes planesOf(int xd, int yd, int M, int margin)
{
    SlotPlanes g;
    g.M = M; g.pitch = yd + margin; g.H = xd; g.W = yd; g.origin = margin * (g.pitch + 1);
    return g;
}
SlotPlanes planesOf(int xd, int yd, int M) { return planesOf(xd, yd, M, 0); }
ciphertext3D encryptImagePlanes(const vector<int64_t> &pixels, int zd, int xd, int yd, int M, int margin, int out_form)
{
    if (!g_slot_on) throw logic_error("encryptImagePlanes: setSlotEncoding() must be called first");
    const int n = N();
    if (zd < 1 || xd < 1 || yd < 1 || pixels.size() != (size_t)zd * xd * yd) throw invalid_argument("encryptImagePlanes: [zd][xd][yd] pixels");
    if (M < 1 || (M & (M - 1)) || M > n / 2 || margin < 0 || margin > M || ((long long)xd + margin) * ((long long)yd + margin) + margin > M)
        throw invalid_argument("encryptImagePlanes: M must be a power of two <= n/2 that holds a plane and its margin");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("encryptImagePlanes: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    const size_t per = (size_t)xd * yd;
    const int pitch = yd + margin, origin = margin * (pitch + 1);       // (the last pixel at origin + (xd - 1) pitch + yd - 1 < (xd + margin)(yd + margin) + margin)
    vector<int64_t> h((size_t)zd * n, 0);                               // plane-major: slot i of plane z at h[z n + i]
    for (int z = 0; z < zd; z++)
        for (int base = 0; base < n; base += M)
            for (int r = 0; r < xd; r++)
                for (int c = 0; c < yd; c++) h[(size_t)z * n + base + origin + r * pitch + c] = pixels[(size_t)z * per + (size_t)r * yd + c];
    DeviceBuffer d_v(h.size() * 8), d_pl(h.size() * 8), d_work(crc_encrypt_dev_work_bytes(ctx(), zd));
    const uint64_t *d_pk = deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    chk(crc_memcpy_h2d(ctx(), d_v.ptr, h.data(), h.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_slots_compose_dev(ctx(), (const int64_t *)d_v.ptr, zd, n, n, 1, (uint64_t *)d_pl.ptr, stream()), "crc_slots_compose_dev");
    ciphertext3D out(1, zd, 1, 1, out_form);
    drawRandomness(zd).call(ABI(crc_encrypt_dev_forms), ABI(crc_encrypt_dev_key_forms), [&](auto f, auto... rnd) {
        return f(ctx(), d_pk, (const uint64_t *)d_pl.ptr, zd, rnd..., out_form, out.data(), d_work.ptr, stream()); });
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return out;
}
ciphertext3D encryptImagePlanes(const vector<float> &pixels, int zd, int xd, int yd, int M, int margin, int out_form)
{
    if (!g_slot_on) throw logic_error("encryptImagePlanes: setSlotEncoding() must be called first");
    const double scale = ldexp(1.0, g_slot_in_bits);
    vector<int64_t> q(pixels.size());
    for (size_t i = 0; i < pixels.size(); i++) {
        const double r = nearbyint((double)pixels[i] * scale);
        if (!(fabs(r) < 9.2e18)) throw invalid_argument("encryptImagePlanes: a pixel does not fit an int64 at this scale");
        q[i] = (int64_t)r;
    }
    return encryptImagePlanes(q, zd, xd, yd, M, margin, out_form);
}
ciphertext3D encryptImagePlanes(const vector<int64_t> &pixels, int zd, int xd, int yd, int M, int out_form) { return encryptImagePlanes(pixels, zd, xd, yd, M, 0, out_form); }
ciphertext3D encryptImagePlanes(const vector<float> &pixels, int zd, int xd, int yd, int M, int out_form) { return encryptImagePlanes(pixels, zd, xd, yd, M, 0, out_form); }
vector<vector<int64_t>> decryptPlanes(const ciphertext3D &t, const SlotPlanes &g)
{
    if (g.M < 1 || g.M > N() || g.pitch < 1 || g.H < 1 || g.W < 1 || g.dil < 1 || g.W > g.pitch || g.origin < 0 ||
        g.origin + (long long)g.dil * ((long long)(g.H - 1) * g.pitch + g.W - 1) >= g.M)
        throw invalid_argument("decryptPlanes: the plane does not fit its period");
    const vector<vector<int64_t>> v = decryptSlots(t, g.M);            // [M][count]
    vector<vector<int64_t>> out(t.count());
    for (size_t z = 0; z < out.size(); z++)
        for (int r = 0; r < g.H; r++) for (int c = 0; c < g.W; c++) out[z].push_back(v[(size_t)g.origin + (size_t)g.dil * (r * g.pitch + c)][z]);
    return out;
}
vector<uint64_t> convSlotsElements(const SlotPlanes &g)
{
    const ConvSlotsGeomPlan P = convSlotsPlan(g);
    vector<uint64_t> out;
    for (uint64_t e : P.elements) if (e != 1 && find(out.begin(), out.end(), e) == out.end()) out.push_back(e);
    return out;
}
ciphertext3D convSlots(const ciphertext3D &t, const vector<int64_t> &weights, int Cout, const SlotPlanes &g, SlotPlanes *og, int out_form)
{
    return convSlots(t, weights, Cout, g, {}, false, og, out_form);
}
ciphertext3D convSlots(const ciphertext3D &t, const vector<int64_t> &weights, int Cout, const SlotPlanes &g, const vector<int64_t> &bias, bool mask, SlotPlanes *og,
                       int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    const ConvSlotsGeomPlan P = convSlotsPlan(g);
    const vector<uint64_t> gs = hoistedElements("convSlots", t, P.steps, out_form);
    if (t.B != 1 || t.xd != 1 || t.yd != 1) throw invalid_argument("convSlots: a tensor [1][zd][1][1] of channel planes (encryptImagePlanes)");
    const int Cin = (int)t.count(), T = (int)P.steps.size(), k = crc_ctx_k(ctx()), dbc = galoisDbc();
    vector<int64_t> folded;
    if (Cout < 1 || !crc_conv_slots_fold_geom(P, weights, Cout, Cin, (int64_t)g_plain_modulus, folded)) throw invalid_argument("convSlots: weights must be [Cout][Cin][fh][fw]");
    if (!bias.empty() && bias.size() != (size_t)Cout) throw invalid_argument("convSlots: the bias must be [Cout]");
    vector<uint64_t> packed((size_t)k * folded.size());
    chk(crc_conv_slots_pack_weights(ctx(), folded.data(), folded.size(), packed.data()), "crc_conv_slots_pack_weights");
    if (!crc_conv_slots_work_bytes(ctx(), 1, Cin, Cout, T, dbc)) throw invalid_argument("convSlots: too many channels or taps");
    DeviceBuffer d_w(packed.size() * 8);
    chk(crc_memcpy_h2d(ctx(), d_w.ptr, packed.data(), packed.size() * 8, stream()), "crc_memcpy_h2d");
    shared_ptr<DeviceBuffer> d_b, d_m;                                  // the packed bias [k][Cout]; the mask's NTT-form row [k][n]
    if (!bias.empty()) {
        vector<uint64_t> pb((size_t)k * Cout);
        chk(crc_conv_slots_pack_bias(ctx(), bias.data(), bias.size(), pb.data()), "crc_conv_slots_pack_bias");
        d_b = make_shared<DeviceBuffer>(pb.size() * 8);
        chk(crc_memcpy_h2d(ctx(), d_b->ptr, pb.data(), pb.size() * 8, stream()), "crc_memcpy_h2d");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");       // (pb goes out of scope here)
    }
    if (mask) d_m = plainRowsNtt(crc_conv_slots_mask_slots(P), 1);
    ciphertext3D out(1, Cout, 1, 1, out_form);
    ensure(g_scratch, crc_conv_slots_work_bytes(ctx(), 1, Cin, Cout, T, dbc));
    chk(crc_conv_slots_bias_mask_forms(ctx(), t.data(), t.form, 1, Cin, gs.data(), T, (const uint64_t *)d_w.ptr, Cout, d_b ? (const uint64_t *)d_b->ptr : nullptr,
                                       d_m ? (const uint64_t *)d_m->ptr : nullptr, galoisCkeys(), galois_elts.data(), (int)galois_elts.size(), dbc, out.data(),
                                       out_form, g_scratch->ptr, stream()), "convSlots");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // (the weights', the bias' and the mask's buffers go out of scope here)
    if (og) { *og = SlotPlanes(); og->M = g.M; og->pitch = g.pitch; og->origin = g.origin; og->H = P.out_h; og->W = P.out_w; og->dil = P.out_dil; }
    return out;
}
// ---- the dense layer over channel planes: the outputs are rotated, one batched key switch with one key per step ------------
static DensePlanesPlan densePlanesPlan(int M, const vector<int> &in_slots, int O, const vector<int> &out_slots)
{
    vector<int> outs = out_slots;
    if (outs.empty()) for (int o = 0; o < O; o++) outs.push_back(o);    // the default: output o at slot o
    DensePlanesPlan P;
    if (O < 1 || (int)outs.size() != O || !crc_dense_planes_plan(N(), M, in_slots, outs, P))
        throw invalid_argument("densePlanes: M must be a power of two <= n/2, both slot lists distinct slots of [0, M), O of them for the outputs");
    return P;
}
vector<int> densePlanesInSlots(const SlotPlanes &g)
{
    if (g.M < 1 || g.pitch < 1 || g.H < 1 || g.W < 1 || g.dil < 1 || g.W > g.pitch || g.origin < 0 ||
        g.origin + (long long)g.dil * ((long long)(g.H - 1) * g.pitch + g.W - 1) >= g.M)
        throw invalid_argument("densePlanes: the plane does not fit its period");
    vector<int> out;
    for (int r = 0; r < g.H; r++) for (int c = 0; c < g.W; c++) out.push_back(g.origin + g.dil * (r * g.pitch + c));
    return out;
}
vector<uint64_t> densePlanesElements(int M, const vector<int> &in_slots, int O, const vector<int> &out_slots)
{
    const DensePlanesPlan P = densePlanesPlan(M, in_slots, O, out_slots);
    vector<uint64_t> out;
    for (uint64_t e : P.elements) if (e != 1) out.push_back(e);         // (distinct steps below n/2: distinct elements)
    return out;
}
vector<uint64_t> densePlanesElements(const SlotPlanes &g, int O, const vector<int> &out_slots) { return densePlanesElements(g.M, densePlanesInSlots(g), O, out_slots); }
// the prepared form of the keys of the set, one slot per key of the set (crc_dense_planes_forms indexes d_pk as it does elts), kept until the keys change.  A slot
// is filled when a layer first asks for its element `gs`: the keys of other layers (the convolution's) are never prepared.  Null where the fp64 key switch does not
// take these parameters
static const uint64_t *preparedGaloisKeys(int dbc, const vector<uint64_t> &gs)
{
    static vector<char> done;                                           // per key of the set: its slot is filled
    const size_t pkw = crc_galois_prepared_key_words(ctx(), dbc), kw = crc_evk_words(ctx(), dbc);
    if (!pkw || !g_galois_ckeys || galois_elts.empty()) return nullptr;
    if (!g_galois_pkeys) {
        g_galois_pkeys = make_shared<DeviceBuffer>(galois_elts.size() * pkw * 8 + 8);
        done.assign(galois_elts.size(), 0);
    }
    shared_ptr<DeviceBuffer> scratch;
    for (uint64_t g : gs) {
        const size_t e = find(galois_elts.begin(), galois_elts.end(), g) - galois_elts.begin();
        if (g == 1 || e == galois_elts.size() || done[e]) continue;      // (a missing key is the entry point's refusal)
        if (!scratch) scratch = make_shared<DeviceBuffer>(kw * 8);
        chk(crc_galois_prepare_keys_dev(ctx(), (const uint64_t *)g_galois_ckeys->ptr + e * kw, &galois_elts[e], 1, dbc, (uint64_t *)g_galois_pkeys->ptr + e * pkw,
                                        (uint64_t *)scratch->ptr, stream()), "crc_galois_prepare_keys_dev");
        done[e] = 1;
    }
    if (scratch) chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");     // (the scratch goes out of scope here)
    return (const uint64_t *)g_galois_pkeys->ptr;
}
size_t preparedGaloisKeyBytes() { return g_galois_pkeys ? g_galois_pkeys->bytes : 0; }
ciphertext3D densePlanes(const ciphertext3D &t, const vector<int64_t> &W, int O, int M, const vector<int> &in_slots, const vector<int> &out_slots, int out_form)
{
    if (!crc_slots_supported(ctx())) throw logic_error("encryption parameters do not support batching");
    const DensePlanesPlan P = densePlanesPlan(M, in_slots, O, out_slots);
    const vector<uint64_t> gs = hoistedElements("densePlanes", t, P.steps, out_form);
    if (t.B != 1 || t.xd != 1 || t.yd != 1) throw invalid_argument("densePlanes: a tensor [1][zd][1][1] of channel planes (convSlots' result, or a vector)");
    const int Cin = (int)t.count(), R = (int)P.steps.size(), n = N(), k = crc_ctx_k(ctx()), dbc = galoisDbc();
    if (W.size() != (size_t)O * Cin * in_slots.size()) throw invalid_argument("densePlanes: weights must be [O][Cin][P]");
    const uint64_t *d_pk = preparedGaloisKeys(dbc, gs);
    if (!crc_dense_planes_work_bytes(ctx(), 1, Cin, R, dbc, d_pk != nullptr)) throw invalid_argument("densePlanes: too many channels or steps");
    // the rows a step at a time: fold, compose on the device, transform -- the R Cin n integers never exist at once on the host
    const size_t rowp = (size_t)k * n;
    DeviceBuffer d_v((size_t)Cin * n * 8), d_pl((size_t)Cin * n * 8), d_p((size_t)R * Cin * rowp * 8);
    vector<int64_t> rows;
    for (int j = 0; j < R; j++) {
        if (!crc_dense_planes_fold_step(P, W, Cin, (int64_t)g_plain_modulus, j, rows)) throw invalid_argument("densePlanes: weights must be [O][Cin][P]");
        chk(crc_memcpy_h2d(ctx(), d_v.ptr, rows.data(), rows.size() * 8, stream()), "crc_memcpy_h2d");
        chk(crc_slots_compose_dev(ctx(), (const int64_t *)d_v.ptr, Cin, n, n, 1, (uint64_t *)d_pl.ptr, stream()), "crc_slots_compose_dev");
        chk(crc_plain_to_ntt(ctx(), (const uint64_t *)d_pl.ptr, Cin, (uint64_t *)d_p.ptr + (size_t)j * Cin * rowp, stream()), "crc_plain_to_ntt");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");       // (the next step writes `rows` again)
    }
    ciphertext3D out(1, 1, 1, 1, out_form);
    ensure(g_scratch, crc_dense_planes_work_bytes(ctx(), 1, Cin, R, dbc, d_pk != nullptr));
    chk(crc_dense_planes_forms(ctx(), t.data(), t.form, 1, Cin, gs.data(), R, (const uint64_t *)d_p.ptr, galoisCkeys(),
                               galois_elts.data(), (int)galois_elts.size(), d_pk, dbc, out.data(), out_form, g_scratch->ptr, stream()), "densePlanes");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");           // (the rows' buffer goes out of scope here)
    return out;
}
ciphertext3D densePlanes(const ciphertext3D &t, const vector<int64_t> &W, int O, const SlotPlanes &g, const vector<int> &out_slots, int out_form)
{
    return densePlanes(t, W, O, g.M, densePlanesInSlots(g), out_slots, out_form);
}
vector<vector<int64_t>> decryptVector(const ciphertext3D &t, const vector<int> &out_slots)
{
    int top = 0;
    for (int s : out_slots) { if (s < 0 || s >= N()) throw invalid_argument("decryptVector: a slot outside the ring"); top = s > top ? s : top; }
    if (out_slots.empty()) throw invalid_argument("decryptVector: no slots");
    const vector<vector<int64_t>> v = decryptSlots(t, top + 1);        // [slots][count]
    vector<vector<int64_t>> out(t.count());
    for (size_t z = 0; z < out.size(); z++) for (int s : out_slots) out[z].push_back(v[(size_t)s][z]);
    return out;
}
vector<floatCube> decryptImages(const ciphertext3D &t)
{
    const int n = N();
    if (t.form != CRC_COEFF) throw invalid_argument("tensor is in NTT form");
    vector<uint64_t> h = t.toHost(), pl(t.count() * n);
    chk(crc_decrypt(ctx(), secret_key.data(), h.data(), t.count(), 2, pl.data()), "crc_decrypt");
    vector<floatCube> out(t.B, floatCube(t.zd, vector<vector<float>>(t.xd, vector<float>(t.yd))));
    size_t i = 0;
    for (int b = 0; b < t.B; b++) for (int z = 0; z < t.zd; z++) for (int x = 0; x < t.xd; x++) for (int y = 0; y < t.yd; y++, i++)
        out[b][z][x][y] = (float)crc_decode(ctx(), pl.data() + i * n);
    return out;
}
floatCube decryptImage(const ciphertext3D &t)
{
    if (t.B != 1) throw invalid_argument("decryptImage expects a single image; use decryptImages for a batch");
    return decryptImages(t)[0];
}
int noiseBudget(const ciphertext3D &t, size_t index)
{
    vector<uint64_t> h(ctBytes() / 8);
    chk(crc_memcpy_d2h(ctx(), h.data(), (char *)t.data() + index * ctBytes(), ctBytes(), stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return crc_noise_budget(ctx(), secret_key.data(), h.data(), 2);
}

// ---- Layer ------------------------------------------------------------------------------------------------------------
void Layer::computeBoundaries(int xd, int yd, int xs, int ys, int xf, int yf, int *xl, int *yl)
{
    *xl = xf > xs ? xd - xf + 1 : xd - xs + 1;
    *yl = yf > ys ? yd - yf + 1 : yd - ys + 1;
}
static void checkInput(const ciphertext3D &in, int zd, int xd, int yd, const char *who)
{
    if (!in.buf || in.zd != zd || in.xd != xd || in.yd != yd) throw invalid_argument(string(who) + ": input tensor shape does not match the layer");
}
static shared_ptr<DeviceBuffer> &ensure(shared_ptr<DeviceBuffer> &b, size_t bytes)
{
    if (!b || b->bytes < bytes) b = make_shared<DeviceBuffer>(bytes);
    return b;
}
// a form-preserving layer's output converted to the form the network asked for: CRC_COEFF <-> CRC_NTT, nothing when the tensor is in it already
static void toForm(ciphertext3D &t, int form, const char *who)
{
    if (t.form == form) return;
    if (t.form == CRC_COEFF && form == CRC_NTT) chk(crc_ntt_fwd(ctx(), t.data(), t.count(), 2, stream()), "crc_ntt_fwd");
    else if (t.form == CRC_NTT && form == CRC_COEFF) chk(crc_ntt_inv(ctx(), t.data(), t.count(), 2, stream()), "crc_ntt_inv");
    else throw invalid_argument(string(who) + ": cannot convert form " + to_string(t.form) + " to out_form " + to_string(form) + " (CRC_COEFF and CRC_NTT only)");
    t.form = form;
}

// The pass driver of the client-side refreshes.  `items` items (ciphertexts, or whole planes) of in_cts input ciphertexts and `ids` keystream ids each go through
// launch(first item, items, randomness) in passes of refresh_pass_len items, which share the layers' scratch area; every pass draws its randomness as it starts
template <class WorkBytes, class Launch> static void refreshPasses(size_t items, size_t in_cts, size_t ids, WorkBytes &&work_bytes, Launch &&launch)
{
    const size_t pass = refresh_pass_len(work_bytes(1), items, in_cts);
    ensure(g_scratch, work_bytes(pass));
    for (size_t o = 0; o < items; o += pass) {
        const size_t c = min(pass, items - o);
        launch(o, c, drawRandomness(c * ids));
    }
}

// The client-side refresh of network.cpp:30-34 -- `floatCube image = decryptImage(input); input = encryptImage(image);` -- for a whole batch on the launch
// stream (crc_refresh_dev: decrypt, decode, round to float, encode, encrypt; nothing crosses PCIe and the host does not wait).  Passes of bounded size share the
// layers' scratch area.  Fresh randomness per ciphertext exactly as encryptImage draws it (deterministic only under setDeterministicSeed)
ciphertext3D refreshImages(const ciphertext3D &t, int out_form, vector<float> *values, bool symmetric)
{
    if (!t.buf) throw invalid_argument("refreshImages: empty tensor");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument("refreshImages: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    const uint64_t *d_pk = symmetric ? nullptr : deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    auto work_bytes = [&](size_t c) { return symmetric ? crc_refresh_sym_dev_work_bytes(ctx(), c, t.form) : crc_refresh_dev_work_bytes(ctx(), c, t.form); };
    ciphertext3D out(t.B, t.zd, t.xd, t.yd, out_form);
    const size_t cnt = t.count();
    shared_ptr<DeviceBuffer> d_vals;
    if (values) d_vals = make_shared<DeviceBuffer>(cnt * sizeof(float));
    refreshPasses(cnt, 1, 1, work_bytes, [&](size_t o, size_t c, const Randomness &rnd) {
        float *dv = d_vals ? (float *)d_vals->ptr + o : nullptr;
        if (symmetric) rnd.call(ABI(crc_refresh_sym_dev), ABI(crc_refresh_sym_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, ctAt(t, o), c, t.form, r..., out_form, ctAt(out, o), dv, g_scratch->ptr, stream()); });
        else rnd.call(ABI(crc_refresh_dev), ABI(crc_refresh_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, d_pk, ctAt(t, o), c, t.form, r..., out_form, ctAt(out, o), dv, g_scratch->ptr, stream()); });
    });
    if (values) {
        values->assign(cnt, 0.f);
        chk(crc_memcpy_d2h(ctx(), values->data(), d_vals->ptr, cnt * sizeof(float), stream()), "crc_memcpy_d2h");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    }
    return out;
}

// The refresh of a slot-batched tensor (crc_slots_refresh_dev: decrypt, every slot divided by `divisor` and rounded, encrypt), on the launch stream, in passes
// of bounded size on the layers' scratch area; seed / key and counter exactly as refreshImages draws them
ciphertext3D rescaleSlots(const ciphertext3D &t, uint64_t divisor, int out_form, bool symmetric)
{
    if (!t.buf) throw invalid_argument("rescaleSlots: empty tensor");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument("rescaleSlots: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (divisor < 1 || divisor > ((uint64_t)1 << 62)) throw invalid_argument("rescaleSlots: the divisor must be in 1..2^62");
    if (!crc_slots_supported(ctx())) throw invalid_argument("rescaleSlots: the plain modulus must be a prime that is 1 mod 2n and none of the engine's moduli");
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    const uint64_t *d_pk = symmetric ? nullptr : deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    auto work_bytes = [&](size_t c) { return symmetric ? crc_slots_refresh_sym_dev_work_bytes(ctx(), c, t.form) : crc_slots_refresh_dev_work_bytes(ctx(), c, t.form); };
    ciphertext3D out(t.B, t.zd, t.xd, t.yd, out_form);
    refreshPasses(t.count(), 1, 1, work_bytes, [&](size_t o, size_t c, const Randomness &rnd) {
        if (symmetric) rnd.call(ABI(crc_slots_refresh_sym_dev), ABI(crc_slots_refresh_sym_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, ctAt(t, o), c, t.form, divisor, r..., out_form, ctAt(out, o), g_scratch->ptr, stream()); });
        else rnd.call(ABI(crc_slots_refresh_dev), ABI(crc_slots_refresh_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, d_pk, ctAt(t, o), c, t.form, divisor, r..., out_form, ctAt(out, o), g_scratch->ptr, stream()); });
    });
    return out;
}
ciphertext3D SlotRescaleLayer::forward(ciphertext3D input)
{
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("SlotRescaleLayer: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    return rescaleSlots(input, divisor, out_form, symmetric);
}
void SlotRescaleLayer::printLayerStructure() { cerr << "SlotRescaleLayer " << name << " :bits " << bits << " divisor " << divisor << endl; }

// rescaleSlots with the client-side activation between decrypt and encrypt (crc_slots_refresh_act_dev); a pass is a run of whole [xd][yd] planes
ciphertext3D actSlots(const ciphertext3D &t, int xs, int ys, int xf, int yf, uint64_t divisor, int relu, uint64_t cap, int out_form, bool symmetric)
{
    if (!t.buf) throw invalid_argument("actSlots: empty tensor");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument("actSlots: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (divisor < 1 || divisor > ((uint64_t)1 << 62)) throw invalid_argument("actSlots: the divisor must be in 1..2^62");
    if (!crc_slots_supported(ctx())) throw invalid_argument("actSlots: the plain modulus must be a prime that is 1 mod 2n and none of the engine's moduli");
    if (!windowOk(t.xd, t.yd, xs, ys, xf, yf)) throw invalid_argument("actSlots: the window does not fit the tensor");
    if (relu != 0 && relu != 1) throw invalid_argument("actSlots: relu must be 0 or 1");
    if (cap > (g_plain_modulus - 1) / 2) throw invalid_argument("actSlots: the cap must be at most (t - 1) / 2");
    const uint64_t *d_sk = deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key");
    const uint64_t *d_pk = symmetric ? nullptr : deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key");
    const int xd = t.xd, yd = t.yd, xo = (xd - xf) / xs + 1, yo = (yd - yf) / ys + 1;
    auto work_bytes = [&](size_t p) { return symmetric ? crc_slots_refresh_act_sym_dev_work_bytes(ctx(), p, xd, yd, xs, ys, xf, yf, t.form)
                                                      : crc_slots_refresh_act_dev_work_bytes(ctx(), p, xd, yd, xs, ys, xf, yf, t.form); };
    ciphertext3D out(t.B, t.zd, xo, yo, out_form);
    const size_t in_cts = (size_t)xd * yd, out_cts = (size_t)xo * yo;
    refreshPasses((size_t)t.B * t.zd, in_cts, out_cts, work_bytes, [&](size_t o, size_t p, const Randomness &rnd) {
        if (symmetric) rnd.call(ABI(crc_slots_refresh_act_sym_dev), ABI(crc_slots_refresh_act_sym_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, ctAt(t, o * in_cts), p, xd, yd, xs, ys, xf, yf, t.form, divisor, relu, cap, r..., out_form, ctAt(out, o * out_cts), g_scratch->ptr,
                     stream()); });
        else rnd.call(ABI(crc_slots_refresh_act_dev), ABI(crc_slots_refresh_act_dev_key), [&](auto f, auto... r) {
            return f(ctx(), d_sk, d_pk, ctAt(t, o * in_cts), p, xd, yd, xs, ys, xf, yf, t.form, divisor, relu, cap, r..., out_form, ctAt(out, o * out_cts), g_scratch->ptr,
                     stream()); });
    });
    return out;
}
ciphertext3D SlotReluLayer::forward(ciphertext3D input)
{
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("SlotReluLayer: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    return actSlots(input, 1, 1, 1, 1, divisor, 1, cap, out_form, symmetric);
}
void SlotReluLayer::printLayerStructure() { cerr << "SlotReluLayer " << name << " :bits " << bits << " divisor " << divisor << " cap " << cap << endl; }
ciphertext3D SlotMaxPoolLayer::forward(ciphertext3D input)
{
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("SlotMaxPoolLayer: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    return actSlots(input, xs, ys, xf, yf, divisor, relu ? 1 : 0, cap, out_form, symmetric);
}
void SlotMaxPoolLayer::printLayerStructure()
{
    cerr << "SlotMaxPoolLayer " << name << " :stride " << xs << " " << ys << " window " << xf << " " << yf << " bits " << bits << " divisor " << divisor << " relu "
         << relu << " cap " << cap << endl;
}

// Decryptor::invariant_noise_budget of a whole tensor on the launch stream (crc_noise_budget_dev), in passes of bounded work that share the layers' scratch
// area.  The result buffer: one {min, first index} pair per pass, then the budgets -- so the pairs and the first ciphertext's budget are one small copy
struct DeviceBudgets { shared_ptr<DeviceBuffer> buf; size_t passes = 0, pass = 0, count = 0;
    int32_t *pairs() const { return (int32_t *)buf->ptr; } int32_t *bits() const { return pairs() + 2 * passes; } };
// what the measurement reads: a tensor of the global context under the global secret key, or a LevelTensor under its level's
struct BudgetView { crc_ctx *c; const uint64_t *d_sk; const uint64_t *data; size_t count; int form; };
static BudgetView budgetView(const ciphertext3D &t, const char *who)
{
    if (!t.buf || t.count() == 0) throw invalid_argument(string(who) + ": empty tensor");
    return BudgetView{ctx(), deviceKey(g_d_sk, g_d_sk_fp, secret_key, "secret key"), t.data(), t.count(), t.form};
}
static DeviceBudgets deviceBudgets(const BudgetView &t, const char *who)
{
    if (t.form != CRC_COEFF && t.form != CRC_NTT) throw invalid_argument(string(who) + ": ciphertext forms only (CRC_COEFF / CRC_NTT)");
    const size_t ctb = crc_ct_words(t.c, 2) * 8;
    DeviceBudgets r;
    r.count = t.count;
    const size_t one = crc_noise_budget_dev_work_bytes(t.c, 1, 2, t.form);
    r.pass = ((size_t)4 << 30) / (one ? one : 1);
    if (r.pass < 1024) r.pass = 1024;
    if (r.pass > r.count) r.pass = r.count;
    r.passes = (r.count + r.pass - 1) / r.pass;
    ensure(g_scratch, crc_noise_budget_dev_work_bytes(t.c, r.pass, 2, t.form));
    r.buf = make_shared<DeviceBuffer>((2 * r.passes + r.count) * sizeof(int32_t));
    for (size_t o = 0, pi = 0; o < r.count; o += r.pass, pi++) {
        const size_t c = min(r.pass, r.count - o);
        chk(crc_noise_budget_dev(t.c, t.d_sk, (const uint64_t *)((const char *)t.data + o * ctb), c, 2, t.form, r.bits() + o, r.pairs() + 2 * pi,
                                 g_scratch->ptr, stream()), "crc_noise_budget_dev");
    }
    return r;
}
static vector<int> allBudgets(const BudgetView &t, const char *who)
{
    const DeviceBudgets r = deviceBudgets(t, who);
    vector<int32_t> h(r.count);
    chk(crc_memcpy_d2h(t.c, h.data(), r.bits(), r.count * sizeof(int32_t), stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(t.c, stream()), "crc_stream_sync");
    return vector<int>(h.begin(), h.end());
}
vector<int> noiseBudgets(const ciphertext3D &t) { return allBudgets(budgetView(t, "noiseBudgets"), "noiseBudgets"); }
// {min, first index} of the tensor and the budget of its ciphertext 0
static int minAndFirstBudget(const BudgetView &t, const char *who, size_t *where, int *first)
{
    const DeviceBudgets r = deviceBudgets(t, who);
    vector<int32_t> h(2 * r.passes + 1);
    chk(crc_memcpy_d2h(t.c, h.data(), r.pairs(), h.size() * sizeof(int32_t), stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(t.c, stream()), "crc_stream_sync");
    int best = h[0]; size_t at = (size_t)h[1];
    for (size_t pi = 1; pi < r.passes; pi++) if (h[2 * pi] < best) { best = h[2 * pi]; at = pi * r.pass + (size_t)h[2 * pi + 1]; }
    if (where) *where = at;
    if (first) *first = h[2 * r.passes];
    return best;
}
static int minAndFirstBudget(const ciphertext3D &t, const char *who, size_t *where, int *first) { return minAndFirstBudget(budgetView(t, who), who, where, first); }
int minNoiseBudget(const ciphertext3D &t, size_t *where) { return minAndFirstBudget(t, "minNoiseBudget", where, nullptr); }

// ---- levels: a tensor continues over the first `kept` moduli (crc_mod_switch_forms) --------------------------------------
// A Level belongs to the parameters it was made under: setParameters() / delParameters() start a new generation, and a level of an older one is refused.
Level::~Level() { if (ctx) crc_ctx_destroy(ctx); }
shared_ptr<Level> makeLevel(int kept, bool derive_keys)
{
    const int k = K(), n = N();
    if (kept < 1 || kept >= k) throw invalid_argument("makeLevel: a level keeps 1 .. k - 1 of the " + to_string(k) + " coefficient moduli");
    if (secret_key.size() != (size_t)k * n || public_key.size() != (size_t)2 * k * n) throw logic_error("makeLevel: the keys do not match the parameters");
    vector<uint64_t> q(k);
    chk(crc_ctx_table(ctx(), "q", q.data(), k), "crc_ctx_table");
    auto L = make_shared<Level>();
    if (derive_keys) chk(crc_ctx_create_level(ctx(), kept, crc_ctx_device(ctx()), &L->ctx), "makeLevel: crc_ctx_create_level");
    else chk(crc_ctx_create(n, q.data(), kept, g_plain_modulus, crc_ctx_device(ctx()), &L->ctx), "makeLevel: crc_ctx_create");
    if (!crc_mod_switch_supported(ctx(), L->ctx)) throw logic_error("makeLevel: the prefix context is not a level of the parameters");
    L->kept = kept; L->generation = g_generation;
    L->secret_key.assign(secret_key.begin(), secret_key.begin() + (size_t)kept * n);
    for (int p = 0; p < 2; p++) L->public_key.insert(L->public_key.end(), public_key.begin() + (size_t)p * k * n, public_key.begin() + ((size_t)p * k + kept) * n);
    L->d_secret_key = make_shared<DeviceBuffer>(L->secret_key.size() * 8);
    chk(crc_memcpy_h2d(L->ctx, L->d_secret_key->ptr, L->secret_key.data(), L->secret_key.size() * 8, stream()), "crc_memcpy_h2d");
    if (derive_keys) {
        // the global keys, which are public material, become the level's on the device: no secret key is read
        if (!crc_keys_restrict_supported(ctx(), L->ctx)) throw logic_error("makeLevel: the derived context is not a level of the parameters");
        L->derived = true;
        auto restricted = [&](const shared_ptr<DeviceBuffer> &from, size_t n_keys, int dbc, const char *what) {
            auto to = make_shared<DeviceBuffer>(n_keys * crc_evk_words(L->ctx, dbc) * 8 + 16);
            chk(crc_keys_restrict_dev(ctx(), L->ctx, (const uint64_t *)from->ptr, (int)n_keys, dbc, (uint64_t *)to->ptr, stream()), what);
            return to;
        };
        if (ev_keys16) L->d_ev_keys16 = restricted(ev_keys16, 1, 16, "makeLevel: crc_keys_restrict_dev (evaluation keys)");
        if (g_galois_keys && !galois_elts.empty()) {
            L->galois_elts = galois_elts; L->galois_dbc = g_galois_dbc ? g_galois_dbc : 16;
            L->d_galois_keys = restricted(g_galois_keys, galois_elts.size(), L->galois_dbc, "makeLevel: crc_keys_restrict_dev (Galois keys)");
            if (g_galois_ckeys) L->d_galois_ckeys = restricted(g_galois_ckeys, galois_elts.size(), L->galois_dbc, "makeLevel: crc_keys_restrict_dev (conjugated keys)");
        }
    }
    chk(crc_stream_sync(L->ctx, stream()), "crc_stream_sync");
    return L;
}
static const Level &levelOf(const shared_ptr<Level> &L, const char *who)
{
    if (!L || !L->ctx) throw invalid_argument(string(who) + ": no level");
    if (!context || L->generation != g_generation) throw invalid_argument(string(who) + ": the level was made under other parameters");
    return *L;
}
static const Level &levelOf(const LevelTensor &t, const char *who)
{
    const Level &L = levelOf(t.level, who);
    if (!t.buf || t.count() == 0) throw invalid_argument(string(who) + ": empty tensor");
    if (t.buf->bytes < t.count() * crc_ct_words(L.ctx, 2) * 8) throw invalid_argument(string(who) + ": the tensor does not have this level's ciphertext size");
    return L;
}
vector<uint64_t> LevelTensor::toHost() const
{
    const Level &L = levelOf(*this, "LevelTensor::toHost");
    vector<uint64_t> h(count() * crc_ct_words(L.ctx, 2));
    chk(crc_memcpy_d2h(L.ctx, h.data(), data(), h.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(L.ctx, stream()), "crc_stream_sync");
    return h;
}
void LevelTensor::save(const string &path) const
{
    const Level &L = levelOf(*this, "LevelTensor::save");
    if (form != CRC_COEFF) throw invalid_argument("LevelTensor::save: tensor is in NTT form");
    const vector<uint64_t> h = toHost();
    const size_t one = crc_seal_ct_bytes(L.ctx, 2), ctw = crc_ct_words(L.ctx, 2);
    vector<uint8_t> b(one * count()); size_t w = 0;
    for (size_t i = 0; i < count(); i++) chk(crc_seal_ct_save(L.ctx, h.data() + i * ctw, 2, b.data() + i * one, one, &w), "crc_seal_ct_save");
    writeFile(path, b);
}
LevelTensor LevelTensor::load(const shared_ptr<Level> &level, int B, int zd, int xd, int yd, const string &path)
{
    const Level &L = levelOf(level, "LevelTensor::load");
    if (B < 1 || zd < 1 || xd < 1 || yd < 1) throw invalid_argument("LevelTensor::load: empty shape");
    const vector<uint8_t> b = readFile(path);
    LevelTensor t; t.B = B; t.zd = zd; t.xd = xd; t.yd = yd; t.form = CRC_COEFF; t.level = level;
    const size_t cnt = t.count(), ctw = crc_ct_words(L.ctx, 2);
    vector<uint64_t> h(cnt * ctw); size_t off = 0;
    for (size_t i = 0; i < cnt; i++) { int size = 0; size_t used = 0;
        chk(crc_seal_ct_load(L.ctx, b.data() + off, b.size() - off, h.data() + i * ctw, 2, &size, &used), "encrypted is not valid for the level's encryption parameters");
        if (size != 2) throw invalid_argument("expected size-2 ciphertexts");
        off += used; }
    if (off != b.size()) throw invalid_argument("LevelTensor::load: the file holds more than the tensor");
    t.buf = make_shared<DeviceBuffer>(h.size() * 8);
    chk(crc_memcpy_h2d(L.ctx, t.buf->ptr, h.data(), h.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(L.ctx, stream()), "crc_stream_sync");
    return t;
}
LevelTensor modSwitch(const ciphertext3D &t, const shared_ptr<Level> &to, int out_form)
{
    const Level &L = levelOf(to, "modSwitch");
    if (!t.buf || t.count() == 0) throw invalid_argument("modSwitch: empty tensor");
    if (t.form != CRC_COEFF && t.form != CRC_NTT) throw invalid_argument("modSwitch: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("modSwitch: out_form must be CRC_COEFF or CRC_NTT");
    LevelTensor out; out.B = t.B; out.zd = t.zd; out.xd = t.xd; out.yd = t.yd; out.form = out_form; out.level = to;
    out.buf = make_shared<DeviceBuffer>(t.count() * crc_ct_words(L.ctx, 2) * 8);
    ensure(g_scratch, crc_mod_switch_work_bytes(ctx(), L.ctx, t.count(), 2, t.form, out_form));
    chk(crc_mod_switch_forms(ctx(), L.ctx, t.data(), t.form, t.count(), 2, out.data(), out_form, g_scratch->ptr, stream()), "crc_mod_switch_forms");
    return out;
}
// ---- noise flooding ---------------------------------------------------------------------------------------------------------------------------------------------
int floodBits(int budget_in, int lambda)
{
    const int B = crc_flood_bits(ctx(), budget_in, lambda);
    if (B < 0) throw invalid_argument("floodBits: no admissible flood width for this budget and lambda");
    return B;
}
// count ciphertexts of context c under the device public key d_pk, in place; the keystream ids g_enc_counter .. + count - 1 are spent
static void floodOn(crc_ctx *c, const uint64_t *d_pk, uint64_t *d_ct, size_t count, int form, int flood_bits, const char *who)
{
    if (form != CRC_COEFF && form != CRC_NTT) throw invalid_argument(string(who) + ": ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (!crc_flood_supported(c, flood_bits)) throw invalid_argument(string(who) + ": flood_bits is not admissible for the encryption parameters");
    ensure(g_scratch, crc_flood_dev_work_bytes(c, count, form));
    drawRandomness(count).call(ABI(crc_flood_dev), ABI(crc_flood_dev_key), [&](auto f, auto... rnd) {
        return f(c, d_pk, d_ct, count, form, flood_bits, rnd..., g_scratch->ptr, stream()); });
}
void floodImages(ciphertext3D &t, int flood_bits)
{
    if (!t.buf || t.count() == 0) throw invalid_argument("floodImages: empty tensor");
    floodOn(ctx(), deviceKey(g_d_pk, g_d_pk_fp, public_key, "public key"), t.data(), t.count(), t.form, flood_bits, "floodImages");
}
void floodImages(LevelTensor &t, int flood_bits)
{
    const Level &L = levelOf(t, "floodImages");
    if (!t.level->d_public_key) {
        t.level->d_public_key = make_shared<DeviceBuffer>(L.public_key.size() * 8);
        chk(crc_memcpy_h2d(L.ctx, t.level->d_public_key->ptr, L.public_key.data(), L.public_key.size() * 8, stream()), "crc_memcpy_h2d");
    }
    floodOn(L.ctx, (const uint64_t *)t.level->d_public_key->ptr, t.data(), t.count(), t.form, flood_bits, "floodImages");
}
LevelTensor sanitizeResponse(const ciphertext3D &t, int flood_bits, const shared_ptr<Level> &to, int out_form)
{
    levelOf(to, "sanitizeResponse");
    if (!t.buf || t.count() == 0) throw invalid_argument("sanitizeResponse: empty tensor");
    ciphertext3D own(t.B, t.zd, t.xd, t.yd, t.form);
    chk(crc_memcpy_d2d(ctx(), own.data(), t.data(), t.count() * ctBytes(), stream()), "crc_memcpy_d2d");
    floodImages(own, flood_bits);
    LevelTensor out = modSwitch(own, to, out_form);
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");       // (the flooded copy goes out of scope here)
    return out;
}
static LevelTensor levelResult(const LevelTensor &t, const Level &L, int out_form)
{
    LevelTensor out; out.B = t.B; out.zd = t.zd; out.xd = t.xd; out.yd = t.yd; out.form = out_form; out.level = t.level;
    out.buf = make_shared<DeviceBuffer>(t.count() * crc_ct_words(L.ctx, 2) * 8);
    return out;
}
LevelTensor squareRelin(const LevelTensor &t, int out_form)
{
    const Level &L = levelOf(t, "squareRelin");
    if (!L.derived || !L.d_ev_keys16) throw logic_error("squareRelin: the level holds no evaluation keys (makeLevel(kept, true))");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument("squareRelin: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    LevelTensor out = levelResult(t, L, out_form);
    ensure(g_scratch, crc_square_relin_work_bytes(L.ctx, t.count(), 16));
    chk(crc_square_relin_forms(L.ctx, t.data(), t.form, t.count(), (const uint64_t *)L.d_ev_keys16->ptr, 16, out.data(), out_form, g_scratch->ptr, stream()),
        "crc_square_relin_forms");
    return out;
}
LevelTensor rotateRows(const LevelTensor &t, int steps, int out_form)
{
    const Level &L = levelOf(t, "rotateRows");
    if (!crc_slots_supported(L.ctx)) throw logic_error("encryption parameters do not support batching");
    if (!L.derived) throw logic_error("rotateRows: the level holds no Galois keys (makeLevel(kept, true))");
    if ((t.form != CRC_COEFF && t.form != CRC_NTT) || (out_form != CRC_COEFF && out_form != CRC_NTT))
        throw invalid_argument("rotateRows: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    const uint64_t g = crc_galois_elt_rows(L.ctx, steps);
    if (!g) throw invalid_argument("step count too large");
    const int ne = (int)L.galois_elts.size(), dbc = L.galois_dbc ? L.galois_dbc : 16;
    int plan[64];
    if (crc_galois_plan(L.ctx, g, L.galois_elts.data(), ne, plan, 64) < 0) throw invalid_argument("galois key not present");
    LevelTensor out = levelResult(t, L, out_form);
    ensure(g_scratch, crc_apply_galois_work_bytes(L.ctx, t.count(), dbc));
    chk(crc_rotate_rows_forms(L.ctx, t.data(), t.form, t.count(), steps, L.d_galois_keys ? (const uint64_t *)L.d_galois_keys->ptr : nullptr, L.galois_elts.data(), ne,
                              dbc, out.data(), out_form, g_scratch->ptr, stream()), "crc_rotate_rows_forms");
    return out;
}
vector<floatCube> decryptImages(const LevelTensor &t)
{
    const Level &L = levelOf(t, "decryptImages");
    const int n = N();
    if (t.form != CRC_COEFF) throw invalid_argument("tensor is in NTT form");
    vector<uint64_t> h = t.toHost(), pl(t.count() * n);
    chk(crc_decrypt(L.ctx, L.secret_key.data(), h.data(), t.count(), 2, pl.data()), "crc_decrypt");
    vector<floatCube> out(t.B, floatCube(t.zd, vector<vector<float>>(t.xd, vector<float>(t.yd))));
    size_t i = 0;
    for (int b = 0; b < t.B; b++) for (int z = 0; z < t.zd; z++) for (int x = 0; x < t.xd; x++) for (int y = 0; y < t.yd; y++, i++)
        out[b][z][x][y] = (float)crc_decode(L.ctx, pl.data() + i * n);
    return out;
}
vector<vector<int64_t>> decryptSlots(const LevelTensor &t, int S)
{
    const Level &L = levelOf(t, "decryptSlots");
    if (t.form != CRC_COEFF && t.form != CRC_NTT) throw invalid_argument("decryptSlots: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (S < 1 || S > N()) throw invalid_argument("decryptSlots: 1 to n slots");
    const size_t cnt = t.count();
    DeviceBuffer d_pl(cnt * (size_t)N() * 8), d_v(cnt * (size_t)S * 8), d_work(crc_decrypt_dev_work_bytes(L.ctx, cnt, 2, t.form));
    chk(crc_decrypt_dev(L.ctx, (const uint64_t *)L.d_secret_key->ptr, t.data(), cnt, 2, t.form, (uint64_t *)d_pl.ptr, d_work.ptr, stream()), "crc_decrypt_dev");
    chk(crc_slots_decompose_dev(L.ctx, (const uint64_t *)d_pl.ptr, cnt, S, (int64_t *)d_v.ptr, 1, cnt, stream()), "crc_slots_decompose_dev");
    vector<int64_t> h(cnt * (size_t)S);
    chk(crc_memcpy_d2h(L.ctx, h.data(), d_v.ptr, h.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(L.ctx, stream()), "crc_stream_sync");
    vector<vector<int64_t>> out(S);
    for (int j = 0; j < S; j++) out[j].assign(h.begin() + (size_t)j * cnt, h.begin() + (size_t)(j + 1) * cnt);
    return out;
}
static BudgetView budgetView(const LevelTensor &t, const char *who)
{
    const Level &L = levelOf(t, who);
    return BudgetView{L.ctx, (const uint64_t *)L.d_secret_key->ptr, t.data(), t.count(), t.form};
}
vector<int> noiseBudgets(const LevelTensor &t) { return allBudgets(budgetView(t, "noiseBudgets"), "noiseBudgets"); }
int minNoiseBudget(const LevelTensor &t, size_t *where) { return minAndFirstBudget(budgetView(t, "minNoiseBudget"), "minNoiseBudget", where, nullptr); }

// ---- several plain moduli: r sibling contexts over the parameters' n, q and device, the slots recombined by the CRT (crc_slots_crt_*) ----
// Like a Level, a PlainBase belongs to the parameters it was made under.
PlainBase::~PlainBase() { for (size_t j = 1; j < ctxs.size(); j++) if (ctxs[j]) crc_ctx_destroy(ctxs[j]); }
shared_ptr<PlainBase> makePlainBase(const vector<uint64_t> &ts)
{
    const int k = K(), n = N();
    if (ts.empty() || ts.size() > CRC_SLOTS_CRT_MAX) throw invalid_argument("makePlainBase: a base has 1 .. " + to_string(CRC_SLOTS_CRT_MAX) + " plain moduli");
    if (ts[0] != g_plain_modulus) throw invalid_argument("makePlainBase: the first modulus must be the plain modulus of the parameters");
    if (secret_key.size() != (size_t)k * n || public_key.size() != (size_t)2 * k * n) throw logic_error("makePlainBase: the keys do not match the parameters");
    vector<uint64_t> q(k);
    chk(crc_ctx_table(ctx(), "q", q.data(), k), "crc_ctx_table");
    auto B = make_shared<PlainBase>();
    B->ts = ts; B->generation = g_generation;
    B->ctxs.assign(ts.size(), nullptr);
    B->ctxs[0] = ctx();
    for (size_t j = 1; j < ts.size(); j++) chk(crc_ctx_create(n, q.data(), k, ts[j], crc_ctx_device(ctx()), &B->ctxs[j]), "makePlainBase: crc_ctx_create");
    if (!crc_slots_crt_supported(B->ctxs.data(), (int)ts.size()))
        throw invalid_argument("makePlainBase: the moduli must be pairwise distinct primes that are 1 mod 2n, none of the engine's moduli, with a product below 2^63");
    B->T = 1;
    for (uint64_t t : ts) B->T *= t;
    // the keys live mod q alone: one device copy of each serves every member
    B->d_secret_key = make_shared<DeviceBuffer>(secret_key.size() * 8);
    B->d_public_key = make_shared<DeviceBuffer>(public_key.size() * 8);
    chk(crc_memcpy_h2d(ctx(), B->d_secret_key->ptr, secret_key.data(), secret_key.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_memcpy_h2d(ctx(), B->d_public_key->ptr, public_key.data(), public_key.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return B;
}
static const PlainBase &baseOf(const shared_ptr<PlainBase> &B, const char *who)
{
    if (!B || B->ctxs.empty()) throw invalid_argument(string(who) + ": no plain base");
    if (!context || B->generation != g_generation || B->ctxs[0] != context) throw invalid_argument(string(who) + ": the plain base was made under other parameters");
    return *B;
}
// the base of a tensor whose r parts have one shape and one ciphertext form
static const PlainBase &baseOf(const PlainBaseTensor &t, const char *who)
{
    const PlainBase &B = baseOf(t.base, who);
    if (t.parts.size() != B.ts.size() || t.count() == 0) throw invalid_argument(string(who) + ": the tensor does not have one part per modulus");
    for (const ciphertext3D &p : t.parts) {
        if (!p.buf || p.B != t.parts[0].B || p.zd != t.parts[0].zd || p.xd != t.parts[0].xd || p.yd != t.parts[0].yd || p.form != t.parts[0].form)
            throw invalid_argument(string(who) + ": the parts differ in shape or form");
    }
    if (t.form() != CRC_COEFF && t.form() != CRC_NTT) throw invalid_argument(string(who) + ": ciphertext forms only (CRC_COEFF / CRC_NTT)");
    return B;
}
// under setDeterministicSeed: the public expansion of the seed encryptImage would have used (NOT secure, as every seeded run)
static void crtKey(const Randomness &r, uint8_t key[CRC_KEY_BYTES], uint64_t &stream_base)
{
    if (r.det) { chk(crc_seeded_public_seed(r.seed, key), "crc_seeded_public_seed"); stream_base = 0; }
    else { memcpy(key, g_master_key, CRC_KEY_BYTES); stream_base = r.stream_base; }
}
PlainBaseTensor encryptImageSlotsCrt(const vector<vector<int64_t>> &images, int zd, int xd, int yd, const shared_ptr<PlainBase> &base, int out_form)
{
    const PlainBase &B = baseOf(base, "encryptImageSlotsCrt");
    if (!g_slot_on) throw logic_error("encryptImageSlotsCrt: setSlotEncoding() must be called first");
    const size_t per = (size_t)zd * xd * yd, S = images.size();
    if (zd < 1 || xd < 1 || yd < 1 || S < 1 || S > (size_t)N()) throw invalid_argument("encryptImageSlotsCrt: 1 to n images of [zd][xd][yd] pixels");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("encryptImageSlotsCrt: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    vector<int64_t> h(S * per);
    for (size_t j = 0; j < S; j++) {
        if (images[j].size() != per) throw invalid_argument("encryptImageSlotsCrt: every image must have zd xd yd pixels");
        memcpy(h.data() + j * per, images[j].data(), per * 8);
    }
    DeviceBuffer d_v(h.size() * 8), d_pl(per * (size_t)N() * 8), d_work(crc_encrypt_dev_work_bytes(ctx(), per));
    chk(crc_memcpy_h2d(ctx(), d_v.ptr, h.data(), h.size() * 8, stream()), "crc_memcpy_h2d");
    PlainBaseTensor out;
    out.base = base;
    for (size_t j = 0; j < B.ts.size(); j++) {
        crc_ctx *c = B.ctxs[j];
        chk(crc_slots_compose_dev(c, (const int64_t *)d_v.ptr, per, (int)S, 1, per, (uint64_t *)d_pl.ptr, stream()), "crc_slots_compose_dev");
        ciphertext3D part(1, zd, xd, yd, out_form);
        uint8_t key[CRC_KEY_BYTES]; uint64_t stream_base;
        crtKey(drawRandomness(per), key, stream_base);
        chk(crc_encrypt_dev_key_forms(c, (const uint64_t *)B.d_public_key->ptr, (const uint64_t *)d_pl.ptr, per, key, stream_base, out_form, part.data(), d_work.ptr,
                                      stream()), "crc_encrypt_dev_key_forms");
        out.parts.push_back(part);
    }
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return out;
}
vector<vector<int64_t>> decryptSlotsCrt(const PlainBaseTensor &t, int S)
{
    const PlainBase &B = baseOf(t, "decryptSlotsCrt");
    if (S < 1 || S > N()) throw invalid_argument("decryptSlotsCrt: 1 to n slots");
    const size_t cnt = t.count(), r = B.ts.size();
    DeviceBuffer d_pl(r * cnt * (size_t)N() * 8), d_v(cnt * (size_t)S * 8), d_work(crc_decrypt_dev_work_bytes(ctx(), cnt, 2, t.form()));
    const uint64_t *rows[CRC_SLOTS_CRT_MAX];
    for (size_t j = 0; j < r; j++) {
        uint64_t *pl = (uint64_t *)d_pl.ptr + j * cnt * (size_t)N();
        chk(crc_decrypt_dev(B.ctxs[j], (const uint64_t *)B.d_secret_key->ptr, t.parts[j].data(), cnt, 2, t.form(), pl, d_work.ptr, stream()), "crc_decrypt_dev");
        rows[j] = pl;
    }
    chk(crc_slots_crt_decompose_dev(B.ctxs.data(), (int)r, rows, cnt, S, (int64_t *)d_v.ptr, 1, cnt, stream()), "crc_slots_crt_decompose_dev");
    vector<int64_t> h(cnt * (size_t)S);
    chk(crc_memcpy_d2h(ctx(), h.data(), d_v.ptr, h.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    vector<vector<int64_t>> out(S);
    for (int j = 0; j < S; j++) out[j].assign(h.begin() + (size_t)j * cnt, h.begin() + (size_t)(j + 1) * cnt);
    return out;
}
PlainBaseTensor rescaleSlotsCrt(const PlainBaseTensor &t, uint64_t divisor, int relu, uint64_t cap, int out_form, bool symmetric)
{
    const PlainBase &B = baseOf(t, "rescaleSlotsCrt");
    if (out_form != CRC_COEFF && out_form != CRC_NTT) throw invalid_argument("rescaleSlotsCrt: ciphertext forms only (CRC_COEFF / CRC_NTT)");
    if (divisor < 1 || divisor > ((uint64_t)1 << 62)) throw invalid_argument("rescaleSlotsCrt: the divisor must be in 1..2^62");
    if (relu != 0 && relu != 1) throw invalid_argument("rescaleSlotsCrt: relu must be 0 or 1");
    if (cap > (B.T - 1) / 2) throw invalid_argument("rescaleSlotsCrt: the cap must be at most (T - 1) / 2");
    const int r = (int)B.ts.size();
    const ciphertext3D &p0 = t.parts[0];
    PlainBaseTensor out;
    out.base = t.base;
    for (int j = 0; j < r; j++) out.parts.push_back(ciphertext3D(p0.B, p0.zd, p0.xd, p0.yd, out_form));
    auto work_bytes = [&](size_t c) { return crc_slots_crt_refresh_dev_work_bytes(B.ctxs.data(), r, c, t.form()); };
    const uint64_t *d_sk = (const uint64_t *)B.d_secret_key->ptr, *d_pk = (const uint64_t *)B.d_public_key->ptr;
    // member j takes the stream ids stream_base + j c .. + c of its pass's r c
    refreshPasses(t.count(), 1, r, work_bytes, [&](size_t o, size_t c, const Randomness &rnd) {
        const uint64_t *in[CRC_SLOTS_CRT_MAX]; uint64_t *dst[CRC_SLOTS_CRT_MAX];
        for (int j = 0; j < r; j++) { in[j] = ctAt(t.parts[j], o); dst[j] = ctAt(out.parts[j], o); }
        uint8_t key[CRC_KEY_BYTES]; uint64_t stream_base;
        crtKey(rnd, key, stream_base);
        if (symmetric)
            chk(crc_slots_crt_refresh_sym_dev_key(B.ctxs.data(), r, d_sk, in, c, t.form(), divisor, relu, cap, key, stream_base, out_form, dst, g_scratch->ptr, stream()),
                "crc_slots_crt_refresh_sym_dev_key");
        else
            chk(crc_slots_crt_refresh_dev_key(B.ctxs.data(), r, d_sk, d_pk, in, c, t.form(), divisor, relu, cap, key, stream_base, out_form, dst, g_scratch->ptr,
                                              stream()), "crc_slots_crt_refresh_dev_key");
    });
    return out;
}
ciphertext3D component(const PlainBaseTensor &t, int j)
{
    const PlainBase &B = baseOf(t, "component");
    if (j < 0 || j >= (int)B.ts.size()) throw invalid_argument("component: no such member");
    return t.parts[j];
}
void setComponent(PlainBaseTensor &t, int j, const ciphertext3D &part)
{
    const PlainBase &B = baseOf(t, "setComponent");
    if (j < 0 || j >= (int)B.ts.size()) throw invalid_argument("setComponent: no such member");
    const ciphertext3D &p = t.parts[j];
    if (!part.buf || part.B != p.B || part.zd != p.zd || part.xd != p.xd || part.yd != p.yd || part.form != p.form)
        throw invalid_argument("setComponent: the part must have the tensor's shape and form");
    t.parts[j] = part;
}

static int g_expected_batch = 0;                            // images per Network::forward the caller announced (0: unknown)
void setExpectedBatch(int images_per_forward) { g_expected_batch = images_per_forward > 0 ? images_per_forward : 0; }
static bool tooLargeForHbm(size_t weights)
{
    size_t free_b = 0, total_b = 0;
    chk(crc_mem_info(ctx(), &free_b, &total_b), "crc_mem_info");
    const char *e = getenv("CRC_STREAM_SHARE");                 // (tests force streaming on small rings with a tiny share, as netrun.py does)
    const double share = e ? atof(e) : 0.75;
    return (double)weights * K() * N() * 8 > share * (double)total_b;
}
static size_t bytesOf(const shared_ptr<DeviceBuffer> &b) { return b ? b->bytes : 0; }
static shared_ptr<DeviceBuffer> inttCopy(const shared_ptr<DeviceBuffer> &ntt_rows, size_t rows)       // coefficient-form twin of NTT-form delta rows
{
    const size_t rowb = (size_t)K() * N() * 8;
    auto out = make_shared<DeviceBuffer>(rows * rowb);
    chk(crc_memcpy_d2d(ctx(), out->ptr, ntt_rows->ptr, rows * rowb, stream()), "crc_memcpy_d2d");
    chk(crc_ntt_inv(ctx(), (uint64_t *)out->ptr, rows, 1, stream()), "crc_ntt_inv");
    return out;
}

// A batch-norm layer folded into the conv / dense layer behind it (Network::fuse), on canonical NTT-form weight rows [f][T] -- the whole layer, or one tile
// of output rows while a tile-wise layer's limb weights are built: w'[f][z][tap] = w (*) s[z], b'[f] = b[f] - sum_t w'[f][t] (*) M[z(t)]
struct BnFold {
    BatchNormLayer &bn;
    const int T, per_ch;                                    // weights per output row, and per batch-norm channel
    DeviceBuffer fake, outc, wk;
    vector<uint64_t> corr, q;
    // (the correction is the dense kernel on one pseudo-image whose ciphertexts are (M[z(t)], 0), built here once for calls on up to max_rows output rows)
    BnFold(BatchNormLayer &bn, int T, int per_ch, int max_rows) : bn(bn), T(T), per_ch(per_ch), fake((size_t)T * 2 * K() * N() * 8),
        outc((size_t)max_rows * 2 * K() * N() * 8), wk(max<size_t>(crc_dense_work_bytes(ctx(), 1, T, max_rows, CRC_NTT), 256)),
        corr((size_t)max_rows * 2 * K() * N()), q(K())
    {
        const size_t rowb = (size_t)K() * N() * 8;
        chk(crc_memset(ctx(), fake.ptr, 0, fake.bytes, stream()), "crc_memset");
        for (int z = 0; z < T / per_ch; z++) for (int t = 0; t < per_ch; t++)
            chk(crc_memcpy_d2d(ctx(), (char *)fake.ptr + ((size_t)z * per_ch + t) * 2 * rowb, (char *)bn.d_mean[1]->ptr + (size_t)z * rowb, rowb, stream()),
                "crc_memcpy_d2d");
        chk(crc_ctx_table(ctx(), "q", q.data(), K()) < 0 ? CRC_ERR_INVALID_ARGUMENT : CRC_OK, "crc_ctx_table");
    }
    // d_w: fn output rows, scaled in place; bias: their NTT-form rows [fn][k][n] on the host, corrected in place.  Waits for the stream
    void apply(uint64_t *d_w, int fn, uint64_t *bias)
    {
        const int n = N(), k = K();
        for (int f = 0; f < fn; f++)
            chk(crc_multiply_plain_ntt(ctx(), d_w + (size_t)f * T * k * n, (const uint64_t *)bn.d_invstd->ptr, T, per_ch, 1, stream()),
                "crc_multiply_plain_ntt");
        chk(crc_dense(ctx(), (const uint64_t *)fake.ptr, d_w, nullptr, 1, T, fn, CRC_NTT, CRC_NTT, (uint64_t *)outc.ptr, wk.ptr, stream()), "crc_dense");
        chk(crc_memcpy_d2h(ctx(), corr.data(), outc.ptr, (size_t)fn * 2 * k * n * 8, stream()), "crc_memcpy_d2h");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
        for (int f = 0; f < fn; f++) for (int m = 0; m < k; m++) for (int s2 = 0; s2 < n; s2++) {
            uint64_t &b = bias[((size_t)f * k + m) * n + s2]; const uint64_t c = corr[(((size_t)f * 2) * k + m) * n + s2];
            b = b >= c ? b - c : b + q[m] - c;
        }
    }
};

// ---- MacLayer: what ConvolutionalLayer and FullyConnectedLayer share ------------------------------------------------------------------
static bool g_matrix_cores = true;                  // Network::matrix_cores of the forward in progress (layers called directly plan with the default)
// (the one statement of the policy, shared with netrun.py)
int MacLayer::plannedForm(int B) const
{
    int wf = CRC_NTT;
    // (a boxed layer is planned as what it runs: the base window over the summed image)
    const int xdi = xd - (bxf - 1) * xs, ydi = yd - (byf - 1) * ys;
    if (slot_weights && g_matrix_cores) chk(crc_plan_mac_scalar(ctx(), zd, xdi, ydi, xs, ys, wxf(), wyf(), nf, B, &wf), "crc_plan_mac_scalar");
    else chk(crc_plan_mac(ctx(), zd, xdi, ydi, xs, ys, wxf(), wyf(), nf, B, g_matrix_cores ? 1 : 0, &wf), "crc_plan_mac");
    return wf;
}
// a boxed layer's weights back to the enlarged window W * box (crc_conv2d_fold_pool makes exactly that; its bias output -- the box's multiple of a bias that already
// is one -- is dropped)
void MacLayer::unbox()
{
    if (!boxed()) return;
    packWeights(true);
    const size_t rowb = (size_t)K() * N() * 8;
    auto w2 = make_shared<DeviceBuffer>((size_t)nf * zd * xf * yf * rowb), b2 = make_shared<DeviceBuffer>((size_t)nf * rowb);
    chk(crc_conv2d_fold_pool(ctx(), (const uint64_t *)d_w->ptr, (const uint64_t *)d_b[1]->ptr, nullptr, nf, zd, wxf(), wyf(), xs, ys, bxf, byf,
        (uint64_t *)w2->ptr, (uint64_t *)b2->ptr, stream()), "crc_conv2d_fold_pool");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    d_w = w2; bxf = byf = 1;
}
// room for the limb copy (CRC_NTTL) beside the canonical weights it is made from
bool MacLayer::limbFits() const
{
    size_t free_b = 0, total_b = 0;
    chk(crc_mem_info(ctx(), &free_b, &total_b), "crc_mem_info");
    return free_b >= crc_limb_weights_bytes(ctx(), nf, zd, xf, yf) + ((size_t)24 << 30);
}
void MacLayer::upload()
{
    if (alreadyNtt()) return;
    vector<const Plaintext *> w, b;
    plaintexts(0, nf, w, &b);
    streamed = forced_placement >= 0 ? forced_placement == 1 : tooLargeForHbm(w.size());
    // Tile-wise limb weights are a dense layer's only: the root's placement 2, or decided here.
    if (forced_placement >= 0) tilewise = forcedTilewise();
    // (g_expected_batch: a deployment that evaluates one image at a time -- setExpectedBatch(1) -- never takes the limb GEMM for a dense layer, so its canonical
    // weights stay resident and the layer runs as a weight stream (mac_stream_kernel) instead of being built tile-wise in limb form)
    else if (dense && !streamed && plannedForm(g_expected_batch) == CRC_NTTL) {
        // canonical + limb copy beyond what HBM has left, the limb copy alone within it: build the limb weights tile by tile at the first forward
        // (buildTilewise)
        size_t free_b = 0, total_b = 0;
        chk(crc_mem_info(ctx(), &free_b, &total_b), "crc_mem_info");
        const size_t canon = w.size() * (size_t)K() * N() * 8, limb = crc_limb_weights_bytes(ctx(), nf, zd, xf, yf), reserve = (size_t)24 << 30;
        // (the tests force it on small rings)
        tilewise = (canon + limb + reserve > free_b && limb + reserve + ((size_t)8 << 30) <= free_b) || getenv("CRC_FORCE_TILEWISE") != nullptr;
    }
    if (streamed) d_plain = uploadPlain(w, 3); else if (!tilewise) d_w = uploadPlain(w, 0);
    d_b[0] = uploadPlain(b, 1); d_b[1] = uploadPlain(b, 2);
    alreadyNtt() = true;                   // transform_kernel_to_ntt, convolutionalLayer.cpp:151-156 (done once)
}
vector<uint64_t> MacLayer::hostBias()
{
    vector<uint64_t> bias((size_t)nf * K() * N());
    chk(crc_memcpy_d2h(ctx(), bias.data(), d_b[1]->ptr, bias.size() * 8, stream()), "crc_memcpy_d2h");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return bias;
}
void MacLayer::setBias(const vector<uint64_t> &ntt_rows)
{
    d_b[1] = make_shared<DeviceBuffer>(ntt_rows.size() * 8);
    chk(crc_memcpy_h2d(ctx(), d_b[1]->ptr, ntt_rows.data(), ntt_rows.size() * 8, stream()), "crc_memcpy_h2d");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    d_b[0] = inttCopy(d_b[1], nf);
}
void MacLayer::buildTilewise()
{
    if (tile_built) return;
    const size_t rowb = (size_t)K() * N() * 8, T = taps();
    d_w = make_shared<DeviceBuffer>(crc_limb_weights_bytes(ctx(), nf, zd, xf, yf));
    const int ft = (int)max<size_t>(1, min<size_t>((size_t)nf, ((size_t)4 << 30) / (T * rowb)));
    unique_ptr<BnFold> fold;
    vector<uint64_t> bias;
    if (fold_bn) { fold.reset(new BnFold(*fold_bn, (int)T, (int)T / fold_bn->num_channels, ft)); bias = hostBias(); }
    for (int f0 = 0; f0 < nf; f0 += ft) {
        const int fn = min(ft, nf - f0);
        vector<const Plaintext *> w;
        plaintexts(f0, fn, w, nullptr);
        shared_ptr<DeviceBuffer> wt = uploadPlain(w, 0);                                   // lift + NTT of the tile's plaintexts (canonical, scratch)
        if (fold) fold->apply((uint64_t *)wt->ptr, fn, bias.data() + (size_t)f0 * K() * N());
        chk(crc_limb_pack_weights_tile(ctx(), (const uint64_t *)wt->ptr, nf, f0, fn, zd, xf, yf, d_w->ptr, stream()), "crc_limb_pack_weights_tile");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    }
    if (fold) { setBias(bias); chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync"); }
    w_form = CRC_NTTL; tile_built = true;
}
size_t MacLayer::deviceBytes() const { return bytesOf(d_w) + bytesOf(d_b[0]) + bytesOf(d_b[1]) + bytesOf(d_plain) + bytesOf(d_wtile) + bytesOf(d_ytile) +
    bytesOf(d_w_canon); }
string MacLayer::kernelName() const
{
    // one image through a resident dense layer runs as a weight stream
    if (dense && last_B == 1 && !streamed && (w_form == CRC_NTTP || w_form == CRC_NTT)) return w_form == CRC_NTTP ?
        "mac_stream_kernel (weight stream: one image, two rows per weight; v_mad_u64_u32, CRC_NTTP)" :
        "mac_stream_kernel (weight stream: one image; canonical residues)";
    const int wf = streamed ? stream_form : w_form;
    const string k = wf == CRC_NTTLS ? "mfma_mac2w_kernel (int8 limb GEMM over all slots, scalar weights, CRC_NTTLS)" :
                     wf == CRC_NTTL ? "mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL)" : wf == CRC_NTTL1 ?
        "mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1)"
                   : wf == CRC_NTTP ? "mac3_kernel (v_mad_u64_u32, CRC_NTTP)" : "mac3_kernel (v_mad_u64_u32, canonical residues)";
    return k + (!streamed ? "" : wf == CRC_NTTL ? ", streamed weights (64-filter limb tiles built inside the forward)" : ", streamed weights") +
        (tilewise ? ", limb weights built tile by tile" : "");
}
int MacLayer::placement() { upload(); return streamed ? 1 : tilewise ? 2 : 0; }
bool MacLayer::streamsOnMatrixCores(int B) { upload(); return streamed && plannedForm(B) == CRC_NTTL; }
void MacLayer::restoreCanonical()
{
    if (w_form == CRC_NTTP || (w_form == CRC_NTTL1 && d_w_canon)) { packWeights(true); return; }
    if (w_form != CRC_NTTL && w_form != CRC_NTTL1 && w_form != CRC_NTTLS) return;
    if (!hasPlaintexts()) throw logic_error(dense ? "FullyConnectedLayer " + name + ": weights are in limb form and there are no plaintexts to rebuild them from" :
        "ConvolutionalLayer " + name + ": a folded layer's weights are in limb form and it has no plaintexts to rebuild them from");
    // (a tile-wise layer goes back to "not built": the next forward builds its limb tensor again, with whatever batch-norm layer fuse() folds into it)
    d_w.reset(); w_form = CRC_NTT; alreadyNtt() = false; tile_built = false;
    upload();
}
void MacLayer::deviceParameters(vector<shared_ptr<DeviceBuffer>> &out, bool allocate_only)
{
    if (allocate_only && !alreadyNtt() && forcedTilewise()) {
        // a tile-wise layer is never on the wire (its only device copy is the limb tensor -- 182 GiB for PlainModelWoPad's fc3 at n = 16384, k = 4 -- which
        // every rank builds from its own plaintexts, deterministically): a receiving rank needs the model's plaintexts like the root
        if (!hasPlaintexts()) throw logic_error("FullyConnectedLayer " + name +
            ": tile-wise weights are built on every rank -- a receiving rank must load the model too");
    } else if (allocate_only && !alreadyNtt()) {            // a receiving rank sizes the buffers without encoding anything
        const size_t rowb = (size_t)K() * N() * 8;
        streamed = forced_placement >= 0 ? forced_placement == 1 : tooLargeForHbm(nf * taps());
        if (!streamed) d_w = make_shared<DeviceBuffer>(nf * taps() * rowb);
        d_b[0] = make_shared<DeviceBuffer>(nf * rowb); d_b[1] = make_shared<DeviceBuffer>(nf * rowb);
        alreadyNtt() = true;
    }
    upload();
    if (tilewise) { buildTilewise(); return; }              // nothing to send or receive (see above)
    packWeights(true);                                      // canonical residues on the wire
    if (streamed && !d_plain) d_plain = make_shared<DeviceBuffer>(nf * taps() * N() * 8);
    out.push_back(streamed ? d_plain : d_w); out.push_back(d_b[0]); out.push_back(d_b[1]);
}
bool MacLayer::limbWeights(int B)
{
    upload();
    if (streamed) return false;
    if (tilewise) { buildTilewise(); return true; }
    if (w_form == CRC_NTTL || w_form == CRC_NTTL1 || w_form == CRC_NTTLS) return true;
    int planned = plannedForm(B);
    if (planned == CRC_NTTLS) {
        // the scalar form of a slot-batched layer: packed from the (possibly fused) canonical rows, which are dropped like the limb GEMM's.  Kilobytes to a few
        // megabytes: no look at the free memory.  A row that is not a constant polynomial (the pack says so) keeps the layer on the row path, silently
        if (w_form == CRC_NTTP) packWeights(true);
        auto ws = make_shared<DeviceBuffer>(crc_scalar_weights_bytes(ctx(), nf, zd, xf, yf));
        int constant = 1;
        const int rc = crc_scalar_pack_weights(ctx(), (const uint64_t *)d_w->ptr, N(), nf, zd, xf, yf, ws->ptr, &constant, stream());
        if (rc == CRC_OK) { d_w = ws; w_form = CRC_NTTLS; return true; }
        if (constant) chk(rc, "crc_scalar_pack_weights");
        slot_weights = false;
        planned = plannedForm(B);
    }
    // The one-channel matrix-core kernel (kernels_mfma1.hip) is a convolution's only: crc_plan_mac answers CRC_NTTL1 for a dense layer with in_dim == 1 as
    // well, which stays on the vector-ALU kernel
    const bool conv1 = !dense && planned == CRC_NTTL1;
    // (a boxed layer that does not get the one-channel kernel -- matrix cores off, a forced form -- takes its enlarged window back and is planned again)
    if (boxed() && !(conv1 && crc_limb_conv1_box_supported(ctx(), zd, xd, yd, xs, ys, wxf(), wyf(), nf, bxf, byf))) { unbox(); return limbWeights(B); }
    // (decided BEFORE the weights are touched: a layer that stays on the vector-ALU kernel keeps its 28-bit packed weights -- unpacking and re-packing them on
    // every forward() is a read-modify-write of the whole layer.  Nothing is allocated between this look at the free memory and the limb copy below)
    if (!conv1 && !(planned == CRC_NTTL && limbFits())) return false;
    if (w_form == CRC_NTTP) packWeights(true);
    auto wl = make_shared<DeviceBuffer>(conv1 ? crc_limb_conv1_weights_bytes_for(ctx(), nf, wxf(), wyf()) : crc_limb_weights_bytes(ctx(), nf, zd, xf, yf));
    if (conv1) chk(crc_limb_conv1_pack_weights(ctx(), (const uint64_t *)d_w->ptr, nf, wxf(), wyf(), wl->ptr, stream()), "crc_limb_conv1_pack_weights");
    else chk(crc_limb_pack_weights(ctx(), (const uint64_t *)d_w->ptr, nf, zd, xf, yf, wl->ptr, stream()), "crc_limb_pack_weights");
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    // (the canonical copy of a one-channel layer is small: kept, so that the weights can go back on the wire; the limb GEMM's is dropped)
    if (conv1) d_w_canon = d_w;
    d_w = wl; w_form = conv1 ? CRC_NTTL1 : CRC_NTTL;
    return true;
}
void MacLayer::packWeights(bool unpack)
{
    upload();
    if (streamed || (tilewise && !tile_built)) return;
    if (w_form == CRC_NTTL1 && unpack) { d_w = d_w_canon; d_w_canon.reset(); w_form = CRC_NTT; return; }
    if (w_form == CRC_NTTL || w_form == CRC_NTTL1 || w_form == CRC_NTTLS) { if (unpack) throw logic_error(kind() + (" " + name) +
        ": weights are in limb form (fuse() / broadcastParameters() must precede the first forward())"); return; }
    if ((w_form == CRC_NTTP) == !unpack) return;
    chk(crc_pack28(ctx(), (uint64_t *)d_w->ptr, nf * taps() * K(), unpack ? 1 : 0, stream()), "crc_pack28");
    w_form = unpack ? CRC_NTT : CRC_NTTP;
}
ciphertext3D MacLayer::run(const ciphertext3D &input, int zo, int xo, int yo)
{
    upload();
    // a tile-wise layer has no canonical weights: whoever reaches it first -- Network::forward through limbWeights, a direct call, a network with matrix_cores
    // off -- builds the limb tensor, the only form its weights exist in (the layer then runs on the limb GEMM whatever the plan would have been)
    if (tilewise) buildTilewise();
    last_B = input.B;
    ciphertext3D out(input.B, zo, xo, yo, out_form);
    if (streamed) { stream_form = forwardStreamed(input, out); return out; }
    // a boxed layer runs on the one-channel matrix-core kernel alone: a layer that reaches this point in another form (called directly, matrix cores off) takes
    // its enlarged window back
    if (boxed() && w_form != CRC_NTTL1) unbox();
    if (boxed()) {
        const size_t bw = crc_conv2d_box_forms_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, wxf(), wyf(), nf, bxf, byf, input.form, w_form, out_form);
        if (!bw) throw invalid_argument(kind() + string(": unsupported geometry"));
        ensure(g_scratch, bw);
        chk(crc_conv2d_box_forms(ctx(), input.data(), (const uint64_t *)d_w->ptr, w_form, (const uint64_t *)d_b[out_form != CRC_COEFF]->ptr, input.B, zd, xd, yd,
            xs, ys, wxf(), wyf(), nf, bxf, byf, input.form, out_form, out.data(), g_scratch->ptr, stream()), "crc_conv2d_box_forms");
        if (out_form == CRC_NTTLC) out.form = CRC_NTTL;
        return out;
    }
    size_t wb = crc_conv2d_forms_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, xf, yf, nf, input.form, w_form, out_form);
    if (!wb) throw invalid_argument(kind() + string(": unsupported geometry"));      // (a convolution's: a 1x1 geometry always has work bytes)
    ensure(g_scratch, wb);
    // (crc_dense_forms IS this call on the 1x1 geometry; a dense layer's failure keeps the name it has always been reported under)
    chk(crc_conv2d_forms(ctx(), input.data(), (const uint64_t *)d_w->ptr, w_form, (const uint64_t *)d_b[out_form != CRC_COEFF]->ptr, input.B, zd, xd, yd, xs,
        ys, xf, yf, nf, input.form, out_form, out.data(), g_scratch->ptr, stream()), dense ? "crc_dense_forms" : "crc_conv2d_forms");
    if (out_form == CRC_NTTLC) out.form = CRC_NTTL;         // what the convolution behind reads as its limb-form input
    return out;
}
// a streamed layer: lift + NTT a tile of filters, run the layer on the tile, scatter the tile's output channels into the [B][F][P] tensor
int MacLayer::forwardStreamed(const ciphertext3D &input, ciphertext3D &out)
{
    const size_t n = N(), k = K(), rowb = k * n * 8, ctb = ctBytes();
    const size_t T = taps(), P = (size_t)((xd - xf) / xs + 1) * ((yd - yf) / ys + 1);
    auto scatter = [&](int f0, int ft) {
        for (int b = 0; b < input.B; b++)
            chk(crc_memcpy_d2d(ctx(), (char *)out.buf->ptr + ((size_t)b * nf + f0) * P * ctb, (const char *)d_ytile->ptr + (size_t)b * ft * P * ctb,
                (size_t)ft * P * ctb, stream()), "crc_memcpy_d2d");
    };
    // On the matrix cores (a reduction the limb GEMM takes, at least 32 rows in this launch: crc_plan_mac): tiles of 64 filters in limb form, built from
    // canonical sub-tiles of 8 filters (crc_limb_pack_weights_tile), the layer's input converted to limb form once per launch -- PlainModelWoPad's fc3 with all
    // eight primes of n = 16384 (netrun.py does the same: 25 against 58 ms per image on the vector-ALU tiles)
    const bool ntt_in = input.form == CRC_NTT || input.form == CRC_NTTP || input.form == CRC_NTTL;
    if (ntt_in && plannedForm(input.B) == CRC_NTTL) {
        const int ft_max = min(64, nf), sub = min(8, ft_max);
        const size_t wt = (size_t)sub * T * rowb, wl = crc_limb_weights_bytes(ctx(), ft_max, zd, xf, yf), yt = (size_t)input.B * ft_max * P * ctb;
        ensure(d_wtile, wt);
        ensure(d_ytile, yt);
        ensure(g_wltile, wl);
        const void *xl = input.data();
        if (input.form != CRC_NTTL) {
            const size_t xb = crc_limb_tensor_bytes(ctx(), input.B, zd, xd, yd);
            ensure(g_xltile, xb);
            chk(crc_limb_pack_tensor(ctx(), input.data(), input.form, input.B, zd, xd, yd, g_xltile->ptr, stream()), "crc_limb_pack_tensor");
            xl = g_xltile->ptr;
        }
        const size_t wb = crc_conv2d_forms_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, xf, yf, ft_max, CRC_NTTL, CRC_NTTL, out_form);
        ensure(g_scratch, wb);
        for (int f0 = 0; f0 < nf; f0 += ft_max) {
            const int ft = min(ft_max, nf - f0);
            for (int s0 = 0; s0 < ft; s0 += sub) {
                const int fs = min(sub, ft - s0);
                chk(crc_plain_to_ntt(ctx(), (const uint64_t *)d_plain->ptr + (size_t)(f0 + s0) * T * n, (size_t)fs * T, (uint64_t *)d_wtile->ptr, stream()),
                    "crc_plain_to_ntt");
                chk(crc_limb_pack_weights_tile(ctx(), (const uint64_t *)d_wtile->ptr, ft, s0, fs, zd, xf, yf, g_wltile->ptr, stream()),
                    "crc_limb_pack_weights_tile");
            }
            chk(crc_conv2d_forms(ctx(), (const uint64_t *)xl, (const uint64_t *)g_wltile->ptr, CRC_NTTL,
                (const uint64_t *)((const char *)d_b[out_form != CRC_COEFF]->ptr + (size_t)f0 * rowb),
                                 input.B, zd, xd, yd, xs, ys, xf, yf, ft, CRC_NTTL, out_form, (uint64_t *)d_ytile->ptr, g_scratch->ptr, stream()),
                                     "crc_conv2d_forms");
            scatter(f0, ft);
        }
        return CRC_NTTL;
    }
    // tile: as many filters (a multiple of 8, the MAC kernel's filter granule) as make 2-16 GiB of NTT-form weights, by what HBM has left
    size_t free_b = 0, total_b = 0;
    chk(crc_mem_info(ctx(), &free_b, &total_b), "crc_mem_info");
    const size_t tile_bytes = d_wtile && d_wtile->bytes >= ((size_t)1 << 30) ? d_wtile->bytes : max<size_t>((size_t)2 << 30, min<size_t>((size_t)16 << 30,
        free_b / 8));
    size_t ftv = tile_bytes / (T * rowb); if (ftv >= 8) ftv = ftv / 8 * 8;
    const int ft_max = (int)max<size_t>(1, min<size_t>(nf, ftv));
    ensure(d_wtile, ft_max * T * rowb);
    ensure(d_ytile, (size_t)input.B * ft_max * P * ctb);
    size_t wb = crc_conv2d_forms_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, xf, yf, ft_max, input.form, CRC_NTT, out_form);
    ensure(g_scratch, wb);
    for (int f0 = 0; f0 < nf; f0 += ft_max) {
        const int ft = min(ft_max, nf - f0);
        chk(crc_plain_to_ntt(ctx(), (const uint64_t *)d_plain->ptr + (size_t)f0 * T * n, (size_t)ft * T, (uint64_t *)d_wtile->ptr, stream()),
            "crc_plain_to_ntt");
        chk(crc_conv2d_forms(ctx(), input.data(), (const uint64_t *)d_wtile->ptr, CRC_NTT, (const uint64_t *)((const char *)d_b[out_form != CRC_COEFF]->ptr +
            (size_t)f0 * rowb), input.B,
                             zd, xd, yd, xs, ys, xf, yf, ft, input.form, out_form, (uint64_t *)d_ytile->ptr, g_scratch->ptr, stream()), "crc_conv2d_forms");
        scatter(f0, ft);
    }
    return CRC_NTT;
}

// ---- ConvolutionalLayer -----------------------------------------------------------------------------------------------
ConvolutionalLayer::ConvolutionalLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count, plaintext4D &filters,
    vector<Plaintext> &biases)
    : MacLayer(name, false, zd, xd, yd, xs, ys, xf, yf, nf), th_count(th_count), xo((xd - xf) / xs + 1), yo((yd - yf) / ys + 1), zo(nf), filters(filters),
      biases(biases) {}
ConvolutionalLayer::ConvolutionalLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count, istream *infile)
    : MacLayer(name, false, zd, xd, yd, xs, ys, xf, yf, nf), th_count(th_count), xo((xd - xf) / xs + 1), yo((yd - yf) / ys + 1), zo(nf)
    { loadPlaintextParameters(infile); }
void ConvolutionalLayer::plaintexts(int f0, int fn, vector<const Plaintext *> &w, vector<const Plaintext *> *b) const
{
    if ((int)filters.size() != nf || (int)biases.size() != nf) throw invalid_argument("conv: filter/bias count mismatch");
    for (int f = f0; f < f0 + fn; f++) {
        if ((int)filters[f].size() != zd || (int)filters[f][0].size() != xf ||
            (int)filters[f][0][0].size() != yf) throw invalid_argument("conv: kernel shape mismatch");
        for (int z = 0; z < zd; z++) for (int i = 0; i < xf; i++) for (int j = 0; j < yf; j++) w.push_back(&filters[f][z][i][j]);
        if (b) b->push_back(&biases[f]);
    }
}
ciphertext3D ConvolutionalLayer::forward(ciphertext3D input)
{
    checkInput(input, zd, xd, yd, "ConvolutionalLayer");
    return run(input, zo, xo, yo);
}
void ConvolutionalLayer::savePlaintextParameters(ostream *outfile)
{   // order of convolutionalLayer.cpp:213-229
    if ((int)filters.size() != nf) throw logic_error("ConvolutionalLayer " + name +
        ": a folded layer has no plaintext parameters to save (save before Network::fuse())");
    for (int n = 0; n < nf; n++) { for (int z = 0; z < zd; z++) for (int i = 0; i < xf; i++) for (int j = 0; j < yf; j++) filters[n][z][i][j].save(*outfile);
        biases[n].save(*outfile); outfile->flush(); }
}
void ConvolutionalLayer::loadPlaintextParameters(istream *infile)
{
    filters.assign(nf, plaintext3D(zd, plaintext2D(xf, vector<Plaintext>(yf)))); biases.assign(nf, Plaintext());
    for (int n = 0; n < nf; n++) { for (int z = 0; z < zd; z++) for (int i = 0; i < xf; i++) for (int j = 0; j < yf; j++) filters[n][z][i][j].load(*infile);
        biases[n].load(*infile); }
    filters_already_ntt = false;
}
void ConvolutionalLayer::printLayerStructure()
{
    cerr << "Convolutional " << name << " : input (" << zd << "," << xd << "," << yd << "); kernel(" << nf << "," << xf << "," << yf << "); stride(" << xs <<
        "," << ys << "); output("
         << zo << "," << xo << "," << yo << ") " << "run with " << th_count << " threads" << endl;
}

// ---- FullyConnectedLayer ----------------------------------------------------------------------------------------------
FullyConnectedLayer::FullyConnectedLayer(string name, int in_dim, int out_dim, int th_count, plaintext2D &weights, vector<Plaintext> &biases)
    : MacLayer(name, true, in_dim, 1, 1, 1, 1, 1, 1, out_dim), in_dim(in_dim), out_dim(out_dim), th_count(th_count), weights(weights), biases(biases) {}
FullyConnectedLayer::FullyConnectedLayer(string name, int in_dim, int out_dim, int th_count, istream *infile)
    : MacLayer(name, true, in_dim, 1, 1, 1, 1, 1, 1, out_dim), in_dim(in_dim), out_dim(out_dim), th_count(th_count) { loadPlaintextParameters(infile); }
void FullyConnectedLayer::plaintexts(int f0, int fn, vector<const Plaintext *> &w, vector<const Plaintext *> *b) const
{
    if ((int)weights.size() != out_dim || (int)biases.size() != out_dim) throw invalid_argument("fc: weight/bias count mismatch");
    for (int i = f0; i < f0 + fn; i++) {
        if ((int)weights[i].size() != in_dim) throw invalid_argument("fc: row length mismatch");
        for (int j = 0; j < in_dim; j++) w.push_back(&weights[i][j]);
        if (b) b->push_back(&biases[i]);
    }
}
ciphertext3D FullyConnectedLayer::forward(ciphertext3D input)
{
    // reshapeInput, :38-56
    if (!input.buf || input.zd * input.xd * input.yd != in_dim) throw invalid_argument("FullyConnectedLayer: input size does not match in_dim");
    return run(input, 1, out_dim, 1);
}
void FullyConnectedLayer::savePlaintextParameters(ostream *outfile)
{
    for (int i = 0; i < out_dim; i++) { for (int j = 0; j < in_dim; j++) weights[i][j].save(*outfile); biases[i].save(*outfile); outfile->flush(); }
}
void FullyConnectedLayer::loadPlaintextParameters(istream *infile)
{
    weights.assign(out_dim, vector<Plaintext>(in_dim)); biases.assign(out_dim, Plaintext());
    for (int i = 0; i < out_dim; i++) { for (int j = 0; j < in_dim; j++) weights[i][j].load(*infile); biases[i].load(*infile); }
    weights_already_ntt = false;
}
void FullyConnectedLayer::printLayerStructure() { cerr << "Fully connected " << name << " : (" << in_dim << " -> " << out_dim << ")" << "run with " <<
    th_count << " threads" << endl; }

// ---- Pooling ----------------------------------------------------------------------------------------------------------
PoolingLayer::PoolingLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf)
    : Layer(name), xd(xd), yd(yd), zd(zd), xs(xs), ys(ys), xf(xf), yf(yf), xo((xd - xf) / xs + 1), yo((yd - yf) / ys + 1), zo(zd) {}
ciphertext3D PoolingLayer::forward(ciphertext3D input)
{
    checkInput(input, zd, xd, yd, "PoolingLayer");
    ciphertext3D out(input.B, zo, xo, yo, input.form);
    chk(crc_pool(ctx(), input.data(), input.B, zd, xd, yd, xs, ys, xf, yf, d_div ? (const uint64_t *)d_div->ptr : nullptr, input.form, out.data(), stream()),
        "crc_pool");
    toForm(out, out_form, "PoolingLayer");          // pooling is form-preserving
    return out;
}
void PoolingLayer::printLayerStructure()
{
    cerr << "Pooling " << name << " : input (" << zo << "," << xd << "," << yd << "); kernel(" << xf << "," << yf << "); stride(" << xs << "," << ys <<
        "); output(" << zo << "," << xo << "," << yo << ")" << endl;
}
AvgPoolingLayer::AvgPoolingLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf) : PoolingLayer(name, xd, yd, zd, xs, ys, xf, yf)
{
    // slot encoding has no 1 / (xf yf): the layer is the sum pool (no divisor row) and the scale ledger carries the factor xf yf
    if (g_slot_on) { div_factor = scalarPlain(1.0, 1.0); return; }
    div_factor = fraencode(1. / (xf * yf));                 // avgPoolingLayer.cpp:12
    d_div = uploadPlain({&div_factor}, 0);
}

// ---- Padding ----------------------------------------------------------------------------------------------------------
PaddingLayer::PaddingLayer(string name, int xd, int yd, int zd, int px, int py)
    : Layer(name), xd(xd), yd(yd), zd(zd), px(px), py(py), xo(xd + 2 * px), yo(yd + 2 * py), zo(zd)
{
    if (xd < 1 || yd < 1 || zd < 1 || px < 0 || py < 0) throw invalid_argument("PaddingLayer: dimensions must be positive and pads non-negative");
}
ciphertext3D PaddingLayer::forward(ciphertext3D input)
{
    checkInput(input, zd, xd, yd, "PaddingLayer");
    if (input.form != CRC_COEFF && input.form != CRC_NTT) throw invalid_argument("PaddingLayer: input must be in CRC_COEFF or CRC_NTT form");
    ciphertext3D out(input.B, zo, xo, yo, input.form);
    chk(crc_pad(ctx(), input.data(), input.B, zd, xd, yd, px, px, py, py, input.form, out.data(), stream()), "crc_pad");
    toForm(out, out_form, "PaddingLayer");          // padding is form-preserving
    return out;
}
void PaddingLayer::printLayerStructure()
{
    cerr << "Padding " << name << " : input (" << zd << "," << xd << "," << yd << "); pad(" << px << "," << py << "); output(" << zo << "," << xo << "," << yo
         << ")" << endl;
}

// ---- ActivationLayer: what the five activation layers share -----------------------------------------------------------------------------------
ActivationLayer::ActivationLayer(string name, const char *kind, int th_count, int xd, int yd, int zd, int xs, int ys, int xf, int yf, shared_ptr<DeviceBuffer> d_div)
    : Layer(name), xd(xd), yd(yd), zd(zd), xs(xs), ys(ys), xf(xf), yf(yf), xo((xd - xf) / xs + 1), yo((yd - yf) / ys + 1), zo(zd), th_count(th_count), kind(kind),
        d_div(d_div) {}
size_t ActivationLayer::deviceBytes() const { size_t b = bytesOf(d_div); for (auto &r : d_p) b += bytesOf(r); return b; }
ciphertext3D ActivationLayer::begin(const ciphertext3D &input, int form)
{
    if (!input.buf || (pooled() && (input.zd != zd || input.xd != xd || input.yd != yd)))
        throw invalid_argument(string(kind) + ": the input tensor is empty or its shape does not match the layer");
    if (!ev_keys16) throw invalid_argument(string(kind) + ": not enough evaluation keys");
    // the packed / limb operand forms are not produced here (Network::forward never asks an activation layer for them)
    if (out_form != CRC_NTT && out_form != CRC_COEFF) throw invalid_argument(string(kind) + ": out_form must be CRC_NTT or CRC_COEFF");
    if (!uploaded) { rows(); uploaded = true; }
    return pooled() ? ciphertext3D(input.B, zo, xo, yo, form) : ciphertext3D(input.B, input.zd, input.xd, input.yd, form);
}
void *ActivationLayer::scratch(size_t bytes) const { return ensure(g_scratch, bytes)->ptr; }
static const uint64_t *evk16() { return (const uint64_t *)ev_keys16->ptr; }
static const uint64_t *rowPtr(const shared_ptr<DeviceBuffer> &b) { return b ? (const uint64_t *)b->ptr : nullptr; }
// one coefficient encoded (at `scale` under slot encoding) and uploaded as its NTT-form row: mode 0 the plaintext itself (a factor), mode 2 Delta times it (a summand)
static shared_ptr<DeviceBuffer> coeffRow(float c, double scale, int mode) { const Plaintext p = encodeScaled((double)c, scale); return uploadPlain({&p}, mode); }
// the three rows crc_poly2_*_relin_forms take (empty = 1, 0, 0), with the window count and the divisor of a pooling behind the activation folded in
void ActivationLayer::poly2Rows(float c2, float c1, float c0, const double *sc)
{
    const size_t rowb = (size_t)K() * N() * 8;
    auto copyOf = [&](const shared_ptr<DeviceBuffer> &src) {
        auto r = make_shared<DeviceBuffer>(rowb);
        chk(crc_memcpy_d2d(ctx(), r->ptr, src->ptr, rowb, stream()), "crc_memcpy_d2d");
        return r;
    };
    auto timesDiv = [&](const shared_ptr<DeviceBuffer> &r) {
        if (d_div) chk(crc_multiply_plain_ntt(ctx(), (uint64_t *)r->ptr, (const uint64_t *)d_div->ptr, 1, 1, 1, stream()), "crc_multiply_plain_ntt");
    };
    if (c2 != 1.0f || sc[0] != 0) { d_p[0] = coeffRow(c2, sc[0], 0); timesDiv(d_p[0]); }                    // (a scaled 1 is not 1)
    else if (d_div) d_p[0] = copyOf(d_div);
    if (c1 != 0.0f) { d_p[1] = coeffRow(c1, sc[1], 0); timesDiv(d_p[1]); }
    if (c0 != 0.0f) {
        const shared_ptr<DeviceBuffer> one = coeffRow(c0, sc[2], 2);
        d_p[2] = copyOf(one);
        for (int w = 1; w < (pooled() ? xf * yf : 1); w++) chk(crc_add(ctx(), (uint64_t *)d_p[2]->ptr, (const uint64_t *)one->ptr, 1, 1, stream()), "crc_add");
        timesDiv(d_p[2]);
    }
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
}
static void polyCheck(const string &what, float c2, float c1, float c0)
{
    if (!isfinite(c2) || !isfinite(c1) || !isfinite(c0)) throw invalid_argument(what + ": the coefficients must be finite");
    if (c2 == 0.0f) throw invalid_argument(what + ": c2 must not be zero (a polynomial without its square term is a batch norm, not an activation)");
}

// ---- Square -----------------------------------------------------------------------------------------------------------
ciphertext3D SquareLayer::forward(ciphertext3D input)
{
    // either form in, the requested form out: crc_square_relin_forms keeps an NTT-resident network resident
    ciphertext3D out = begin(input, out_form);
    chk(crc_square_relin_forms(ctx(), input.data(), input.form, input.count(), evk16(), 16, out.data(), out_form,
                               scratch(crc_square_relin_work_bytes(ctx(), input.count(), 16)), stream()), "crc_square_relin_forms");
    return out;
}
void SquareLayer::printLayerStructure() { cerr << "Square run with " << th_count << " threads" << endl; }

// ---- Square + pooling (Network::fuse) ---------------------------------------------------------------------------------
ciphertext3D SquarePoolLayer::forward(ciphertext3D input)
{
    // an average pooling's divisor multiplies slot-wise: the pooled tensor is made NTT-resident for it, and brought back to coefficients when the network asked
    // for those
    const int of = d_div ? CRC_NTT : out_form;
    ciphertext3D out = begin(input, of);
    chk(crc_square_pool_relin_forms(ctx(), input.data(), input.form, input.B, zd, xd, yd, xs, ys, xf, yf, evk16(), 16, rowPtr(d_div), out.data(), of,
                                    scratch(crc_square_pool_relin_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, xf, yf, 16)), stream()), "crc_square_pool_relin_forms");
    toForm(out, out_form, kind);
    return out;
}
void SquarePoolLayer::printLayerStructure()
{
    cerr << "Square + Pooling " << name << " : input (" << zd << "," << xd << "," << yd << "); kernel(" << xf << "," << yf << "); stride(" << xs << "," <<
        ys << "); output(" << zo << "," << xo << "," << yo << "); one key switch per pooled ciphertext" << endl;
}

// ---- polynomial activation ------------------------------------------------------------------------------------------------
PolyLayer::PolyLayer(string name, float c2, float c1, float c0, int th_count) : ActivationLayer(name, "PolyLayer", th_count), c2(c2), c1(c1), c0(c0)
    { polyCheck(kind, c2, c1, c0); }
ciphertext3D PolyLayer::forward(ciphertext3D input)
{
    ciphertext3D out = begin(input, out_form);
    chk(crc_poly2_relin_forms(ctx(), input.data(), input.form, input.count(), evk16(), 16, rowPtr(d_p[0]), rowPtr(d_p[1]), rowPtr(d_p[2]), out.data(), out_form,
                              scratch(crc_poly2_relin_work_bytes(ctx(), input.count(), 16)), stream()), "crc_poly2_relin_forms");
    return out;
}
void PolyLayer::printLayerStructure()
{
    cerr << "Poly " << name << " : " << c2 << " x^2 + " << c1 << " x + " << c0 << " run with " << th_count << " threads" << endl;
}

// ---- ciphertext x ciphertext multiply, degree-3 activation ------------------------------------------------------------------
ciphertext3D multiplyRelin(const ciphertext3D &a, const ciphertext3D &b, int out_form)
{
    if (!a.buf || !b.buf) throw invalid_argument("multiplyRelin: empty input");
    if (a.B != b.B || a.zd != b.zd || a.xd != b.xd || a.yd != b.yd) throw invalid_argument("multiplyRelin: the tensors differ in shape");
    if (a.form != b.form || (a.form != CRC_NTT && a.form != CRC_COEFF)) throw invalid_argument("multiplyRelin: both tensors must be in CRC_NTT or both in CRC_COEFF form");
    if (out_form != CRC_NTT && out_form != CRC_COEFF) throw invalid_argument("multiplyRelin: out_form must be CRC_NTT or CRC_COEFF");
    if (!ev_keys16) throw invalid_argument("not enough evaluation keys");
    ciphertext3D out(a.B, a.zd, a.xd, a.yd, out_form);
    ensure(g_scratch, crc_multiply_relin_work_bytes(ctx(), a.count(), 16));
    chk(crc_multiply_relin_forms(ctx(), a.data(), b.data(), a.form, a.count(), (const uint64_t *)ev_keys16->ptr, 16, out.data(), out_form, g_scratch->ptr,
                                 stream()), "crc_multiply_relin_forms");
    return out;
}
Poly3Layer::Poly3Layer(string name, float c3, float c2, float c1, float c0, int th_count) : ActivationLayer(name, "Poly3Layer", th_count), c3(c3), c2(c2), c1(c1),
    c0(c0)
{
    if (!isfinite(c3) || !isfinite(c2) || !isfinite(c1) || !isfinite(c0)) throw invalid_argument("Poly3Layer: the coefficients must be finite");
    if (c3 == 0.0f) throw invalid_argument("Poly3Layer: c3 must not be zero (a polynomial without its cubic term is a PolyLayer)");
}
void Poly3Layer::rows()
{
    if (c3 != 1.0f || slot_scale[0] != 0) d_p[0] = coeffRow(c3, slot_scale[0], 0);
    if (c2 != 0.0f) d_p[1] = coeffRow(c2, slot_scale[1], 0);
    if (c1 != 0.0f) d_p[2] = coeffRow(c1, slot_scale[2], 0);
    if (c0 != 0.0f) d_p[3] = coeffRow(c0, slot_scale[3], 2);
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
}
ciphertext3D Poly3Layer::forward(ciphertext3D input)
{
    ciphertext3D out = begin(input, out_form);
    chk(crc_poly3_relin_forms(ctx(), input.data(), input.form, input.count(), evk16(), 16, rowPtr(d_p[0]), rowPtr(d_p[1]), rowPtr(d_p[2]), rowPtr(d_p[3]), out.data(),
                              out_form, scratch(crc_poly3_relin_work_bytes(ctx(), input.count(), 16)), stream()), "crc_poly3_relin_forms");
    return out;
}
void Poly3Layer::printLayerStructure()
{
    cerr << "Poly3 " << name << " : " << c3 << " x^3 + " << c2 << " x^2 + " << c1 << " x + " << c0 << " run with " << th_count << " threads" << endl;
}

// ---- polynomial activation + pooling (Network::fuse) ------------------------------------------------------------------------
PolyPoolLayer::PolyPoolLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int th_count, float c2, float c1, float c0,
    shared_ptr<DeviceBuffer> d_div) : ActivationLayer(name, "PolyPoolLayer", th_count, xd, yd, zd, xs, ys, xf, yf, d_div), c2(c2), c1(c1), c0(c0)
    { polyCheck(kind, c2, c1, c0); }
ciphertext3D PolyPoolLayer::forward(ciphertext3D input)
{
    ciphertext3D out = begin(input, out_form);
    chk(crc_poly2_pool_relin_forms(ctx(), input.data(), input.form, input.B, zd, xd, yd, xs, ys, xf, yf, evk16(), 16, rowPtr(d_p[0]), rowPtr(d_p[1]), rowPtr(d_p[2]),
                                   out.data(), out_form, scratch(crc_poly2_pool_relin_work_bytes(ctx(), input.B, zd, xd, yd, xs, ys, xf, yf, 16)), stream()),
        "crc_poly2_pool_relin_forms");
    return out;
}
void PolyPoolLayer::printLayerStructure()
{
    cerr << "Poly + Pooling " << name << " : " << c2 << " x^2 + " << c1 << " x + " << c0 << "; input (" << zd << "," << xd << "," << yd << "); kernel(" << xf << ","
         << yf << "); stride(" << xs << "," << ys << "); output(" << zo << "," << xo << "," << yo << "); one key switch per pooled ciphertext" << endl;
}

// ---- BatchNorm --------------------------------------------------------------------------------------------------------
BatchNormLayer::BatchNormLayer(string name, int num_channels, vector<Plaintext> &mean, vector<Plaintext> &var) : Layer(name), num_channels(num_channels),
    mean(mean), var(var) {}
BatchNormLayer::BatchNormLayer(string name, int num_channels, istream *infile) : Layer(name), num_channels(num_channels) { loadPlaintextParameters(infile); }
void BatchNormLayer::upload()
{
    if (d_invstd) return;
    if ((int)mean.size() != num_channels || (int)var.size() != num_channels) throw invalid_argument("bn: parameter count mismatch");
    vector<const Plaintext *> m, v;
    for (int i = 0; i < num_channels; i++) { m.push_back(&mean[i]); v.push_back(&var[i]); }
    d_mean[0] = uploadPlain(m, 1); d_mean[1] = uploadPlain(m, 2); d_invstd = uploadPlain(v, 0);
}
void BatchNormLayer::deviceParameters(vector<shared_ptr<DeviceBuffer>> &out, bool allocate_only)
{
    if (allocate_only && !d_invstd) {
        const size_t rowb = (size_t)K() * N() * 8;
        d_mean[0] = make_shared<DeviceBuffer>(num_channels * rowb); d_mean[1] = make_shared<DeviceBuffer>(num_channels * rowb);
            d_invstd = make_shared<DeviceBuffer>(num_channels * rowb);
    }
    upload();
    out.push_back(d_mean[0]); out.push_back(d_mean[1]); out.push_back(d_invstd);
}
ciphertext3D BatchNormLayer::forward(ciphertext3D input)
{
    if (!input.buf || input.zd != num_channels) throw invalid_argument("BatchNormLayer: channel count mismatch");
    upload();
    ciphertext3D out = deepCopyImage(input);                // the reference works on its by-value copy (batchNormLayer.cpp:29)
    chk(crc_batchnorm(ctx(), out.data(), out.B, out.zd, out.xd, out.yd, (const uint64_t *)d_mean[out.form == CRC_NTT]->ptr, (const uint64_t *)d_invstd->ptr,
        out.form, stream()), "crc_batchnorm");
    toForm(out, out_form, "BatchNormLayer");
    return out;
}
void BatchNormLayer::savePlaintextParameters(ostream *outfile) { for (int i = 0; i < num_channels; i++) { mean[i].save(*outfile); var[i].save(*outfile);
    outfile->flush(); } }
void BatchNormLayer::loadPlaintextParameters(istream *infile)
{
    mean.assign(num_channels, Plaintext()); var.assign(num_channels, Plaintext());
    for (int i = 0; i < num_channels; i++) { mean[i].load(*infile); var[i].load(*infile); }
    d_invstd.reset();
}
void BatchNormLayer::printLayerStructure() { cerr << "BatchNormLayer2D " << name << " :num_channels " << num_channels << endl; }

// ---- Network ----------------------------------------------------------------------------------------------------------
void Network::printNetworkStructure()
{
    for (size_t i = 0; i < layers.size(); i++) { cerr << "(" << i << ") : "; layers[i]->printLayerStructure(); cout << endl; }
}
// ---- Network::forward: plan, timing, range runner, chunk loop (crcnn_amd/netrun.py: _plan / _run / forward_group) ----------------------------------------
struct Network::ForwardRun {
    bool packable = true;                                   // no modulus above 55 bits: the MAC kernels' 28-bit limb pairs exist
    vector<shared_ptr<MacLayer>> mac;                       // the conv / dense layers (mac[L]: none behind the last layer)
    vector<char> limb, streams;                             // layer i reads a limb tensor / ... as a streamed dense layer (limb tiles built inside the forward)
    int split = 0;                                          // chunked: the first dense layer ([0, split) runs on sub-batches of head_chunk images)
    // two-level chunking / the dense layers chunk by chunk as well (no tail) / the refresh in front of `split` runs chunk by chunk, before the assembly
    bool chunked = false, per_chunk = false, chunk_refresh = false;
    struct Timed { int layer; void *start, *stop; };
    vector<Timed> events;                                   // time_with_events: read after the last layer; ev_used of event_pool's are taken
    size_t ev_used = 0;
    bool later_chunk = false;                               // two-level chunking: not the first chunk (profile_budget only lowers a layer's minimum)
};
// The hand-over form behind layer i: NTT between linear layers when resident, coefficient form into Square and out of the net; a producer writes the form its
// consumer's plan names
int Network::boundaryForm(const ForwardRun &f, int i) const
{
    const bool checking = max_num_of_reencryptions >= 0;
    const shared_ptr<MacLayer> &m = f.mac[i], &next = f.mac[i + 1];
    if (!ntt_resident || i + 1 == (int)layers.size()) return CRC_COEFF;
    // the budget-checking forward's scope 0 reads ciphertext 0 on the host: coefficient form at every boundary
    if (checking && budget_scope == 0) return CRC_COEFF;
    // the tensor in front of the refresh is decrypted as it stands (crc_refresh_dev takes either ciphertext form): an NTT-resident network stays resident
    // across it, but no packed / limb hand-over spans it
    if (i + 1 == layer_before_reenc) return CRC_NTT;
    // scope 1 measures the tensor on the device, in CRC_COEFF or CRC_NTT: the packed and limb hand-overs are off under max_num_of_reencryptions >= 0
    if (checking) return CRC_NTT;
    // a limb layer feeding a DENSE limb layer hands its tensor over in limb form (not across the chunk boundary: a dense layer's limb tensor is laid out for its
    // whole batch, runChunks assembles the chunks into it).  The per-slot limb GEMM reads CRC_NTTL, which every limb layer writes; a scalar dense layer reads
    // CRC_NTTLS, which only a scalar layer writes (any other producer hands over packed rows and the consumer converts them)
    const bool across_chunks = f.chunked && !f.per_chunk && i + 1 == f.split;
    if (f.limb[i] && !f.streams[i] && f.limb[i + 1] && next->dense && !across_chunks) {
        if (next->w_form != CRC_NTTLS) return CRC_NTTL;
        if (m->w_form == CRC_NTTLS) return CRC_NTTLS;
    }
    // a one-channel convolution writes the limb tensor of a matrix-core CONVOLUTION behind it itself (the same bytes for CRC_NTTL and CRC_NTTLS)
    if (m && next && !m->dense && !next->dense && m->w_form == CRC_NTTL1 && (next->w_form == CRC_NTTL || next->w_form == CRC_NTTLS)) return CRC_NTTLC;
    // a conv / dense layer feeding another one hands its tensor over packed (28-bit limb pairs)
    if (f.packable && m && next) return CRC_NTTP;
    return CRC_NTT;
}
Network::ForwardRun Network::plan(int B)
{
    const int L = (int)layers.size();
    ForwardRun f;
    // conv / dense weights go into the MAC kernels' operand form (28-bit limb pairs) once; moduli above 55 bits cannot be packed
    { vector<uint64_t> q(K()); crc_ctx_table(ctx(), "q", q.data(), K()); for (uint64_t v : q) if (v >> 55) f.packable = false; }
    f.mac.resize(L + 1);
    for (int i = 0; i < L; i++) f.mac[i] = dynamic_pointer_cast<MacLayer>(layers[i]);
    f.limb.assign(L + 1, 0); f.streams.assign(L + 1, 0);
    // two-level chunking: the layers in front of the first dense layer on sub-batches of head_chunk images, the dense layers on the whole batch
    f.split = L;
    if (head_chunk > 0 && B > head_chunk && ntt_resident && max_num_of_reencryptions < 0)
        for (int i = 1; i < L; i++) if (f.mac[i] && f.mac[i]->dense) { f.split = i; break; }
    f.chunked = f.split < L;
    if (f.packable)
        for (int i = 0; i < L; i++) if (auto m = f.mac[i]) {
            const int Bi = f.chunked && i < f.split ? head_chunk : B;
            f.limb[i] = matrix_cores && m->limbWeights(Bi);
            if (!f.limb[i]) m->packWeights(false);
            // a STREAMED dense layer that will run on the matrix cores (64-filter limb tiles built inside the forward) reads a limb tensor like a resident
            // one: the chunks of a group are packed straight into it, and no second copy of the group's input is made inside the layer
            if (matrix_cores && m->dense && m->streamsOnMatrixCores(Bi)) { f.limb[i] = 1; f.streams[i] = 1; }
        }
    // a dense layer in scalar form (CRC_NTTLS) has no weight stream to amortise over a group of chunks: the whole network runs chunk by chunk instead
    f.per_chunk = f.chunked && f.mac[f.split]->w_form == CRC_NTTLS;
    // the refresh in front of the first dense layer runs chunk by chunk, before the chunks are assembled (the tail range then starts behind it)
    f.chunk_refresh = f.chunked && !f.per_chunk && f.split == layer_before_reenc;
    for (int i = 0; i < L; i++) layers[i]->out_form = boundaryForm(f, i);
    return f;
}
// events on the launch stream (read after the last layer), or wall clock + stream synchronisation
ciphertext3D Network::timed(ForwardRun &f, int i, const function<ciphertext3D()> &call)
{
    if (i >= 0) last_layer_launches[i]++;
    ciphertext3D out;
    if (time_with_events) {
        auto next_event = [&]() { auto &ev = event_pool->ev; if (f.ev_used == ev.size()) { void *e = nullptr; chk(crc_event_create(ctx(), &e), "crc_event_create");
            ev.push_back(e); } return ev[f.ev_used++]; };
        void *e0 = next_event(), *e1 = next_event();
        chk(crc_event_record(ctx(), e0, stream()), "crc_event_record");
        out = call();
        chk(crc_event_record(ctx(), e1, stream()), "crc_event_record");
        f.events.push_back({i, e0, e1});
    } else {
        auto t0 = chrono::high_resolution_clock::now();
        out = call();
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
        (i < 0 ? last_reenc_ms : last_layer_ms[i]) += chrono::duration<double, milli>(chrono::high_resolution_clock::now() - t0).count();
    }
    // profile_budget: the layer's output tensor measured on the device, outside the timed region.  A later chunk of the same layer (two-level chunking) only
    // lowers the minimum; a layer that is repeated after a refresh is measured afresh
    if (i < 0 || !profile_budget || (out.form != CRC_COEFF && out.form != CRC_NTT)) return out;
    int first = -1;
    const int mn = minAndFirstBudget(out, "Network::forward", nullptr, &first);
    if (f.later_chunk && last_layer_budget_min[i] >= 0) { last_layer_budget_min[i] = min(last_layer_budget_min[i], mn); return out; }
    last_layer_budget_min[i] = mn; last_layer_budget_first[i] = first;
    return out;
}
ciphertext3D Network::runLayer(ForwardRun &f, int i, const ciphertext3D &in) { return timed(f, i, [&] { return layers[i]->forward(in); }); }
// the client-side refresh (needs the secret key; network.cpp:30-34), timed like a layer: T_REENC of mainparams.cpp:81
ciphertext3D Network::runRefresh(ForwardRun &f, const ciphertext3D &in)
{
    const int of = ntt_resident && max_num_of_reencryptions < 0 ? CRC_NTT : CRC_COEFF;
    OutHint hint(&act_slot[in.buf == act_slot[0] ? 1 : 0]);
    return timed(f, -1, [&] {
        vector<float> v;
        ciphertext3D out = refreshImages(in, of, keep_reenc_values ? &v : nullptr, reenc_symmetric);
        last_reenc_values.insert(last_reenc_values.end(), v.begin(), v.end());
        return out;
    });
}
ciphertext3D Network::runRange(ForwardRun &f, int lo, int hi, ciphertext3D t, bool to_caller, bool refresh_at_lo)
{
    for (int i = lo; i < hi; i++) {
        if (i == layer_before_reenc && (i > lo || refresh_at_lo)) t = runRefresh(f, t);
        // every layer writes into one of the network's two activation slots (the one its input does not live in); but the last layer's output -- ten
        // ciphertexts per image -- is the caller's own tensor, as in the reference
        OutHint hint(to_caller && i + 1 == hi ? nullptr : &act_slot[t.buf == act_slot[0] ? 1 : 0]);
        t = runLayer(f, i, t);
    }
    // a last layer that hands its input back (none of CrCNN's does) must not give the caller a tensor that lives in a slot the next forward overwrites
    if (to_caller && t.buf && (t.buf == act_slot[0] || t.buf == act_slot[1] || t.buf == tail_slot)) {
        ciphertext3D own(t.B, t.zd, t.xd, t.yd, t.form);
        chk(crc_memcpy_d2d(ctx(), own.data(), t.data(), t.count() * ctBytes(), stream()), "crc_memcpy_d2d");
        t = own;
    }
    return t;
}
// Two-level chunking: layers [0, split) -- all of them when per_chunk -- on sub-batches of head_chunk images, every chunk's result put into one whole-batch tensor
ciphertext3D Network::runChunks(ForwardRun &f, const ciphertext3D &input)
{
    const int B = input.B, hi = f.per_chunk ? (int)layers.size() : f.split;
    const bool limb = !f.per_chunk && f.limb[f.split];
    ciphertext3D whole;
    for (int b0 = 0; b0 < B; b0 += head_chunk) {
        const int Bc = min(head_chunk, B - b0);
        f.later_chunk = b0 > 0;
        ciphertext3D t = runRange(f, 0, hi, input.images(b0, Bc), false, true);
        if (f.chunk_refresh) t = runRefresh(f, t);
        const size_t out_cts = (size_t)t.zd * t.xd * t.yd;
        if (!whole.buf) {
            // the dense layers' input is kept across calls like the activation slots (next to 182 GiB of weights the pool has no room to hold it); the result of
            // a network run chunk by chunk is the caller's own tensor
            OutHint hint(f.per_chunk ? nullptr : &tail_slot);
            whole = ciphertext3D(B, t.zd, t.xd, t.yd, limb ? CRC_NTTL : t.form);
        }
        if (limb)                 // every chunk's tensor goes straight into the dense layer's K-blocked limb tensor
            chk(crc_limb_pack_tensor_at(ctx(), t.data(), t.form, Bc, (int)out_cts, 1, 1, whole.data(), B, b0, stream()), "crc_limb_pack_tensor_at");
        else
            chk(crc_memcpy_d2d(ctx(), (char *)whole.data() + (size_t)b0 * out_cts * ctBytes(), t.data(), (size_t)Bc * out_cts * ctBytes(), stream()), "crc_memcpy_d2d");
    }
    f.later_chunk = false;
    if (!f.per_chunk) chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    return whole;
}
// network.cpp:52-96: after every layer the budget of its output; at <= 5 bits the layer's input is refreshed and the layer repeated (every output a fresh tensor)
ciphertext3D Network::runChecked(ForwardRun &f, ciphertext3D input)
{
    int refreshes_left = max_num_of_reencryptions;
    for (int i = 0; i < (int)layers.size(); i++) {
        ciphertext3D output = runLayer(f, i, input);
        // scope 0: ciphertext 0, on the host; scope 1: the whole tensor on the device, in the form boundaryForm chose (a profiled forward has just measured it)
        const int budget = budget_scope == 0 ? noiseBudget(output) : profile_budget ? last_layer_budget_min[i] : minNoiseBudget(output);
        if (budget <= 5) {
            if (refreshes_left <= 0) throw OutOfBudgetException(i - 1);
            input = runRefresh(f, input);
            refreshes_left--;
            i--;
            continue;
        }
        input = output;
    }
    return input;
}
ciphertext3D Network::forward(ciphertext3D input)
{   // network.cpp:22-47
    const int L = (int)layers.size();
    if (budget_scope != 0 && budget_scope != 1) throw invalid_argument("Network::budget_scope must be 0 or 1");
    // a width the parameters refuse is refused before the first launch
    if (flood_bits && !crc_flood_supported(ctx(), flood_bits)) throw invalid_argument("Network::flood_bits is not admissible for the encryption parameters");
    const shared_ptr<DeviceBuffer> callers = input.buf;
    // the planning flag is this forward's only: layers called directly afterwards plan with the default again
    struct Restore { bool &ref; bool old; ~Restore() { ref = old; } } restore_matrix_cores{g_matrix_cores, g_matrix_cores};
    g_matrix_cores = matrix_cores;
    ForwardRun f = plan(input.B);
    last_layer_ms.assign(L, 0.0);
    last_layer_launches.assign(L, 0);
    last_reenc_ms = 0.0;
    last_reenc_values.clear();
    last_layer_budget_min.assign(profile_budget ? L : 0, -1);
    last_layer_budget_first.assign(profile_budget ? L : 0, -1);
    if (time_with_events && !event_pool) event_pool = make_shared<EventPool>();
    if (max_num_of_reencryptions >= 0) input = runChecked(f, input);
    else {
        if (f.chunked) input = runChunks(f, input);
        // (a network run chunk by chunk has no tail; under two-level chunking the tail starts behind a refresh that ran chunk by chunk)
        if (!f.per_chunk) input = runRange(f, f.chunked ? f.split : 0, L, input, true, !f.chunk_refresh);
    }
    if (flood_bits) {                                       // the response: sanitised before the caller sees it
        if (input.buf == callers && (input.form == CRC_COEFF || input.form == CRC_NTT)) {                         // (a network whose output is its input's buffer: the caller's tensor is not forward's to write)
            ciphertext3D own(input.B, input.zd, input.xd, input.yd, input.form);
            chk(crc_memcpy_d2d(ctx(), own.data(), input.data(), input.count() * ctBytes(), stream()), "crc_memcpy_d2d");
            input = own;
        }
        floodImages(input, flood_bits);
    }
    if (time_with_events) {
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
        for (auto &t : f.events) { float ms = 0; chk(crc_event_elapsed_ms(ctx(), t.start, t.stop, &ms), "crc_event_elapsed_ms");
            (t.layer < 0 ? last_reenc_ms : last_layer_ms[t.layer]) += ms; }
    }
    return input;
}
Network::HbmPlan Network::hbmPlan() const
{
    HbmPlan p;
    for (auto &l : layers) p.parameters += l->deviceBytes();
    p.activations = bytesOf(act_slot[0]) + bytesOf(act_slot[1]) + bytesOf(tail_slot);
    p.work = bytesOf(g_scratch);
    p.keys = bytesOf(ev_keys16);
    return p;
}
Network::EventPool::~EventPool() { if (context) for (void *e : ev) crc_event_destroy(context, e); }

size_t Network::broadcastParameters(crc_comm *comm, int root, bool encode_locally)
{
    if (!comm) throw invalid_argument("broadcastParameters: no communicator");
    const int rank = crc_comm_rank(comm), world = crc_comm_world(comm);
    if (root < 0 || root >= world) throw invalid_argument("broadcastParameters: bad root");
    // the root's placement of every layer's weights (resident / streamed / tile-wise) sizes the buffers on the wire: every rank adopts it before it allocates
    {
        const size_t L = layers.size();
        vector<uint64_t> mine_pl(L, 0), all_pl(L * (size_t)world, 0);
        if (rank == root) for (size_t i = 0; i < L; i++) mine_pl[i] = (uint64_t)layers[i]->placement();
        if (L > 64) throw invalid_argument("broadcastParameters: more than 64 layers");
        if (L) chk(crc_comm_allgather_u64(comm, mine_pl.data(), L, all_pl.data(), stream()), "crc_comm_allgather_u64");
        if (rank != root) for (size_t i = 0; i < L; i++) layers[i]->adoptPlacement((int)all_pl[(size_t)root * L + i]);
    }
    vector<shared_ptr<DeviceBuffer>> bufs;
    // encode_locally: every rank lifts + transforms its own plaintext parameters (it read the same model file) and only the evaluation keys travel; the
    // checksums below then prove that the ranks' encoders agree bit for bit
    for (auto &l : layers) l->deviceParameters(bufs, rank != root && !encode_locally);
    if (!ev_keys16) throw logic_error("setParameters() must be called first");
    const size_t own = encode_locally ? bufs.size() : 0;    // buffers that stay off the wire
    bufs.push_back(ev_keys16);                              // the evaluation keys come from the client through the root
    size_t bytes = 0;
    uint64_t mine[2] = {0, 0};
    for (size_t bi = 0; bi < bufs.size(); bi++) {
        auto &b = bufs[bi];
        const size_t words = b->bytes / 8;
        if (bi >= own) chk(crc_broadcast_weights(comm, (uint64_t *)b->ptr, words, root, stream()), "crc_broadcast_weights");
        uint64_t cs[2];
        chk(crc_checksum64(ctx(), (const uint64_t *)b->ptr, words, cs, stream()), "crc_checksum64");
        mine[0] ^= cs[0]; mine[1] = mine[1] * 0x9E3779B97F4A7C15ULL + cs[1];
        if (bi >= own) bytes += b->bytes;
    }
    vector<uint64_t> all((size_t)2 * world);
    chk(crc_comm_allgather_u64(comm, mine, 2, all.data(), stream()), "crc_comm_allgather_u64");
    for (int r = 0; r < world; r++)
        if (all[2 * r] != all[2 * root] || all[2 * r + 1] != all[2 * root + 1])
            throw runtime_error("broadcastParameters: rank " + to_string(r) + " holds different parameter bytes than the root");
    if (rank != root) {                                     // host copy of the keys follows the device copy
        chk(crc_memcpy_d2h(ctx(), ev_keys16_host.data(), ev_keys16->ptr, ev_keys16_host.size() * 8, stream()), "crc_memcpy_d2h");
        chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    }
    return bytes;
}

int Network::fuse()
{
    const size_t rowb = (size_t)K() * N() * 8;
    int removed = 0;
    // The client-side refresh sits in front of layers[layer_before_reenc] (network.cpp:30-34).  No fold may span it, and the index follows the layers it
    // counts: erasing a layer below it moves the refresh point down with the layers behind it, so the refresh still runs in front of the same layer.
    auto refreshBetween = [&](size_t i) { return layer_before_reenc >= 0 && (int)i + 1 == layer_before_reenc; };
    auto eraseLayer = [&](size_t idx) {
        layers.erase(layers.begin() + idx);
        if (layer_before_reenc >= 0 && (int)idx < layer_before_reenc) layer_before_reenc--;
        removed++;
    };
    // the folding kernels work on canonical residues
    // (a network that has already run holds its weights in the MAC kernels' operand forms: packed residues are unpacked, matrix-core forms -- which drop
    // the canonical copy -- are rebuilt from the layer's plaintexts, so fuse() may follow a forward())
    for (auto &l : layers) if (auto m = dynamic_pointer_cast<MacLayer>(l)) m->restoreCanonical();
    // pool(conv(x)) as ONE convolution with the pooled kernel (crc_conv2d_fold_pool; div: an average pool's NTT-form divisor rows, or null)
    auto foldPool = [&](const ConvolutionalLayer &conv, const string &name, int pxs, int pys, int pxf, int pyf, const shared_ptr<DeviceBuffer> &div) {
        const int xf2 = (pxf - 1) * conv.xs + conv.xf, yf2 = (pyf - 1) * conv.ys + conv.yf;
        vector<Plaintext> nob; plaintext4D nof;
        auto fused = make_shared<ConvolutionalLayer>(name, conv.xd, conv.yd, conv.zd, conv.xs * pxs, conv.ys * pys, xf2, yf2, conv.nf, conv.th_count, nof, nob);
        fused->d_w = make_shared<DeviceBuffer>((size_t)conv.nf * conv.zd * xf2 * yf2 * rowb);
        fused->d_b[1] = make_shared<DeviceBuffer>((size_t)conv.nf * rowb);
        chk(crc_conv2d_fold_pool(ctx(), (const uint64_t *)conv.d_w->ptr, (const uint64_t *)conv.d_b[1]->ptr, div ? (const uint64_t *)div->ptr : nullptr,
                                 conv.nf, conv.zd, conv.xf, conv.yf, conv.xs, conv.ys, pxf, pyf, (uint64_t *)fused->d_w->ptr, (uint64_t *)fused->d_b[1]->ptr,
                                 stream()), "crc_conv2d_fold_pool");
        fused->d_b[0] = inttCopy(fused->d_b[1], conv.nf);
        fused->filters_already_ntt = true;
        return fused;
    };
    // 1. conv + pool
    for (size_t i = 0; i + 1 < layers.size(); i++) {
        auto conv = dynamic_pointer_cast<ConvolutionalLayer>(layers[i]);
        auto pool = dynamic_pointer_cast<PoolingLayer>(layers[i + 1]);
        if (!conv || !pool || refreshBetween(i)) continue;
        conv->upload();
        if (conv->streamed) continue;
        if (pool->zd != conv->nf || pool->xd != conv->xo || pool->yd != conv->yo) continue;
        const int xf2 = (pool->xf - 1) * conv->xs + conv->xf, yf2 = (pool->yf - 1) * conv->ys + conv->yf;
        const int xs2 = conv->xs * pool->xs, ys2 = conv->ys * pool->ys;
        if (xf2 > conv->xd || yf2 > conv->yd) continue;
        const int xo2 = (conv->xd - xf2) / xs2 + 1, yo2 = (conv->yd - yf2) / ys2 + 1;
        if (xo2 != pool->xo || yo2 != pool->yo) continue;
        // the cost model lives behind the C ABI (crc_plan_fold_pool), shared with netrun.py
        int fold = 0;
        chk(crc_plan_fold_pool(ctx(), conv->zd, conv->xd, conv->yd, conv->xs, conv->ys, conv->xf, conv->yf, conv->nf, pool->xs, pool->ys, pool->xf, pool->yf,
            &fold), "crc_plan_fold_pool");
        if (!fold) continue;
        // 1a. ... or the pool's window sum hoisted in front of the convolution (crc_plan_hoist_pool): the layer in front -- a resident convolution, as fused
        // so far, with no refresh in between -- takes the stride-1 sum pool into its weights and so hands over S, the window sums of this layer's input; this
        // layer keeps its window, takes the pool's stride, the divisor into its weights and the bias of every window position (crc_conv2d_hoist_pool).  Both
        // layers keep the names the weight-folded pair has
        auto up = i > 0 && !refreshBetween(i - 1) ? dynamic_pointer_cast<ConvolutionalLayer>(layers[i - 1]) : nullptr;
        if (up) { up->upload(); if (up->streamed || up->tilewise) up = nullptr; }
        int hoist = 0;
        chk(crc_plan_hoist_pool(ctx(), up ? up->zd : 0, up ? up->xd : 0, up ? up->yd : 0, up ? up->xs : 0, up ? up->ys : 0, up ? up->xf : 0, up ? up->yf : 0,
            up ? up->nf : 0, conv->zd, conv->xd, conv->yd, conv->xs, conv->ys, conv->xf, conv->yf, conv->nf, pool->xs, pool->ys, pool->xf, pool->yf,
            g_expected_batch, matrix_cores ? 1 : 0, &hoist), "crc_plan_hoist_pool");
        if (hoist) {
            auto sums = foldPool(*up, up->name, 1, 1, pool->xf, pool->yf, nullptr);
            // ... and a one-channel layer in front sums its INPUT instead of enlarging its window (crc_plan_conv1_box): it keeps its base weights and carries the
            // box; name, geometry and the bias of the fold (pxf pyf b) are the enlarged layer's.  Not behind a batch-norm layer, which step 2 folds into the
            // enlarged window's weights
            int box = 0;
            const bool bn_in_front = i >= 2 && !refreshBetween(i - 2) && dynamic_pointer_cast<BatchNormLayer>(layers[i - 2]);
            if (!up->boxed() && !bn_in_front)
                chk(crc_plan_conv1_box(ctx(), up->zd, up->xd, up->yd, up->xs, up->ys, up->xf, up->yf, up->nf, pool->xf, pool->yf, g_expected_batch,
                    matrix_cores ? 1 : 0, &box), "crc_plan_conv1_box");
            if (box) { sums->d_w = up->d_w; sums->bxf = pool->xf; sums->byf = pool->yf; }
            vector<Plaintext> nob; plaintext4D nof;
            auto down = make_shared<ConvolutionalLayer>(conv->name + "+" + pool->name, sums->xo, sums->yo, conv->zd, pool->xs, pool->ys, conv->xf, conv->yf,
                conv->nf, conv->th_count, nof, nob);
            down->d_w = make_shared<DeviceBuffer>((size_t)conv->nf * conv->zd * conv->xf * conv->yf * rowb);
            down->d_b[1] = make_shared<DeviceBuffer>((size_t)conv->nf * rowb);
            chk(crc_conv2d_hoist_pool(ctx(), (const uint64_t *)conv->d_w->ptr, (const uint64_t *)conv->d_b[1]->ptr, pool->d_div ?
                (const uint64_t *)pool->d_div->ptr : nullptr, conv->nf, conv->zd, conv->xf, conv->yf, pool->xf, pool->yf, (uint64_t *)down->d_w->ptr,
                (uint64_t *)down->d_b[1]->ptr, stream()), "crc_conv2d_hoist_pool");
            down->d_b[0] = inttCopy(down->d_b[1], conv->nf);
            down->filters_already_ntt = true;
            layers[i - 1] = sums;
            layers[i] = down;
            eraseLayer(i + 1);
            continue;
        }
        layers[i] = foldPool(*conv, conv->name + "+" + pool->name, pool->xs, pool->ys, pool->xf, pool->yf, pool->d_div);
        eraseLayer(i + 1);
    }
    // 1b. Square + pooling: one key switch per pooled ciphertext (SquarePoolLayer)
    for (size_t i = 0; i + 1 < layers.size(); i++) {
        auto sq = dynamic_pointer_cast<SquareLayer>(layers[i]);
        auto pool = dynamic_pointer_cast<PoolingLayer>(layers[i + 1]);
        if (!sq || !pool || refreshBetween(i)) continue;
        if (!crc_square_pool_relin_supported(ctx(), 16, pool->xf, pool->yf)) continue;
        layers[i] = make_shared<SquarePoolLayer>(sq->name + "+" + pool->name, pool->xd, pool->yd, pool->zd, pool->xs, pool->ys, pool->xf, pool->yf,
            sq->th_count,
                                                 pool->d_div);
        eraseLayer(i + 1);
    }
    // 1c. polynomial activation + pooling, the same way (PolyPoolLayer; a batch norm behind it is left to the fold below).  A Poly3Layer stays a layer of its
    // own, like a SquareLayer whose pooling cannot be paired: its two key switches are not linear in one set of digits
    for (size_t i = 0; i + 1 < layers.size(); i++) {
        auto po = dynamic_pointer_cast<PolyLayer>(layers[i]);
        auto pool = dynamic_pointer_cast<PoolingLayer>(layers[i + 1]);
        if (!po || !pool || refreshBetween(i)) continue;
        if (!crc_poly2_pool_relin_supported(ctx(), 16, pool->xf, pool->yf)) continue;
        auto pp = make_shared<PolyPoolLayer>(po->name + "+" + pool->name, pool->xd, pool->yd, pool->zd, pool->xs, pool->ys, pool->xf, pool->yf, po->th_count,
                                             po->c2, po->c1, po->c0, pool->d_div);
        for (int j = 0; j < 3; j++) pp->slot_scale[j] = po->slot_scale[j];
        layers[i] = pp;
        eraseLayer(i + 1);
    }
    // 2. batch-norm + conv / dense
    for (size_t i = 0; i + 1 < layers.size(); i++) {
        auto bn = dynamic_pointer_cast<BatchNormLayer>(layers[i]);
        if (!bn || refreshBetween(i)) continue;
        auto m = dynamic_pointer_cast<MacLayer>(layers[i + 1]);
        if (!m) continue;
        // (the fold is written for the window the layer reports: a boxed layer takes its enlarged weights back first -- step 1a does not box behind a batch norm,
        // so this serves a second fuse() only)
        if (m->boxed()) { m->upload(); m->unbox(); }
        // weights per output row and per batch-norm channel: a convolution has one channel per batch-norm channel, a dense layer reads the flattened
        // [ch][x][y] tensor
        const int ch = bn->num_channels, T = (int)m->taps();
        if (m->dense ? T % ch != 0 : m->zd != ch) continue;
        const int per_ch = T / ch;
        m->upload();
        if (m->streamed) continue;
        bn->upload();
        // no canonical weights to fold into: the fold is applied tile by tile when the limb weights are built
        if (m->tilewise) {
            if (m->tile_built) continue;
            m->fold_bn = bn;
            m->name = bn->name + "+" + m->name;
            eraseLayer(i);
            continue;
        }
        BnFold fold(*bn, T, per_ch, m->nf);
        vector<uint64_t> bias = m->hostBias();
        fold.apply((uint64_t *)m->d_w->ptr, m->nf, bias.data());
        m->setBias(bias);
        m->name = bn->name + "+" + m->name;
        eraseLayer(i);
    }
    chk(crc_stream_sync(ctx(), stream()), "crc_stream_sync");
    if (removed) fused_ = true;
    return removed;
}

// ---- network descriptions ---------------------------------------------------------------------------------------------
namespace {
const struct { const char *name, *text; } kBuiltinModels[] = {
#include "builtin_models.inc"
};
[[noreturn]] void descError(int line, const string &what) { throw invalid_argument("line " + to_string(line) + ": " + what); }
// a coefficient of a `poly` line: a decimal number read as double and rounded to float32 (what netrun.py's float() -> numpy.float32 gives)
float descFloat(int line, const string &tok, const char *what)
{
    // (decimal notation, `inf` and `nan` only: the characters both hosts' number parsers agree on)
    char *end = nullptr;
    const bool plain = !tok.empty() && tok.find_first_not_of("0123456789+-.eEinfatyINFATY") == string::npos;
    const double v = plain ? strtod(tok.c_str(), &end) : 0.0;
    if (!plain || end == tok.c_str() || *end) descError(line, string(what) + ": expected a number, got '" + tok + "'");
    const float f = (float)v;
    if (!isfinite(f)) descError(line, string(what) + ": the coefficient must be finite, got '" + tok + "'");
    return f;
}
string descFloatStr(float v) { char b[32]; snprintf(b, sizeof b, "%.9g", (double)v); return b; }
int descInt(int line, const string &tok, const char *what)
{
    if (tok.empty() || tok.size() > 9 || tok.find_first_not_of("0123456789") != string::npos)
        descError(line, string(what) + ": expected a non-negative integer, got '" + tok + "'");
    return atoi(tok.c_str());
}
// the shapes crc_conv2d / crc_pool take (abi.hip, conv_shape_ok): the window fits and the stride leaves no trailing outputs the reference would leave as
// empty ciphertexts
bool windowOk(int xd, int yd, int xs, int ys, int xf, int yf)
{
    if (xd < 1 || yd < 1 || xs < 1 || ys < 1 || xf < 1 || yf < 1 || xf > xd || yf > yd) return false;
    const int xl = xd - max(xf, xs) + 1, yl = yd - max(yf, ys) + 1;
    if (xl < 1 || yl < 1) return false;
    return (xl + xs - 1) / xs == (xd - xf) / xs + 1 && (yl + ys - 1) / ys == (yd - yf) / ys + 1;
}
}   // namespace
const char *builtinDescription(const string &model)
{
    for (auto &m : kBuiltinModels) if (model == m.name) return m.text;
    return nullptr;
}
NetworkDescription NetworkDescription::parse(const string &text, const string &h5_path)
{
    NetworkDescription d;
    bool have_input = false, flat = false;
    int pending_refresh = 0, refresh_line = 0, zd = 0, xd = 0, yd = 0, ln = 0;
    auto check = [&](int line, const string &name, long long count) {
        if (h5_path.empty()) return;
        size_t have = 0;
        if (crc_h5_dataset_count(h5_path.c_str(), name.c_str(), &have)) descError(line, "the model " + h5_path + " has no dataset " + name);
        if ((long long)have != count) descError(line, "dataset " + name + " holds " + to_string(have) + " values, the layer needs " + to_string(count));
    };
    istringstream in(text);
    string raw;
    while (getline(in, raw)) {
        ln++;
        raw = raw.substr(0, raw.find('#'));
        vector<string> tok;
        { istringstream ls(raw); string t; while (ls >> t) tok.push_back(t); }
        if (tok.empty()) continue;
        const string &kind = tok[0];
        if (!have_input) {
            if (kind != "input" || tok.size() != 4) descError(ln, "the first line must be `input zd xd yd`");
            d.zd = zd = descInt(ln, tok[1], "input"); d.xd = xd = descInt(ln, tok[2], "input"); d.yd = yd = descInt(ln, tok[3], "input");
            if (zd < 1 || xd < 1 || yd < 1) descError(ln, "input: dimensions must be positive");
            have_input = true;
            continue;
        }
        if (kind == "refresh") {
            if (tok.size() != 1) descError(ln, "unknown token '" + tok[1] + "' after refresh");
            if (refresh_line) descError(ln, "a second refresh (line " + to_string(refresh_line) + " has the first)");
            pending_refresh = refresh_line = ln;
            continue;
        }
        const bool windowed = kind == "conv" || kind == "pool" || kind == "avgpool" || kind == "client_maxpool";
        if (!windowed && kind != "bn" && kind != "square" && kind != "fc" && kind != "pad" && kind != "poly" && kind != "poly3" && kind != "rescale" &&
            kind != "client_relu") descError(ln, "unknown layer kind '" + kind + "'");
        if (tok.size() < 2) descError(ln, kind + ": the layer name is missing");
        LayerSpec L;
        L.kind = kind; L.name = tok[1]; L.line = ln; L.zd = zd; L.xd = xd; L.yd = yd;
        vector<string> rest(tok.begin() + 2, tok.end());
        if (rest.size() >= 2 && rest[rest.size() - 2] == "threads") {
            if (kind != "conv" && kind != "fc" && kind != "square" && kind != "poly" && kind != "poly3") descError(ln, "unknown token 'threads' for a " + kind + " layer");
            L.threads = descInt(ln, rest.back(), "threads");
            rest.resize(rest.size() - 2);
        }
        if (flat && (windowed || kind == "pad" || kind == "poly" || kind == "poly3"))
            descError(ln, "a " + kind + " layer cannot follow a fully connected layer: the tensor is flat (" + to_string(xd) + " values)");
        // what may follow the bit count of a client_relu / client_maxpool line: [relu] [cap C]; the cap in slot units is nearbyint(C 2^bits), at least 1 (its
        // upper limit (t - 1) / 2 is the builder's to check: it needs the plain modulus)
        auto clientTail = [&](size_t pos, bool with_relu) {
            if (L.bits > 30) descError(ln, kind + ": the bit count must be in 0..30");
            if (with_relu && pos < rest.size() && rest[pos] == "relu") { L.relu = true; pos++; }
            if (pos < rest.size() && rest[pos] == "cap") {
                if (pos + 1 >= rest.size()) descError(ln, kind + ": `cap` takes a value");
                L.cap = descFloat(ln, rest[pos + 1], "cap"); L.has_cap = true;
                if (nearbyint((double)L.cap * ldexp(1.0, L.bits)) < 1) descError(ln, kind + ": the cap " + rest[pos + 1] + " is below one unit of the scale 2^" + to_string(L.bits));
                pos += 2;
            }
            if (pos != rest.size()) descError(ln, "unknown token '" + rest[pos] + "'");
        };
        if (windowed) {
            size_t pos = 0;
            auto values = [&](const char *key, int *a, int *b) {
                if (pos >= rest.size() || rest[pos] != key) descError(ln, kind + ": expected `" + key + "`, got '" + (pos < rest.size() ? rest[pos] : "end of line") + "'");
                const size_t cnt = b ? 2 : 1;
                if (pos + cnt >= rest.size()) descError(ln, kind + ": `" + key + "` takes " + to_string(cnt) + " value(s)");
                *a = descInt(ln, rest[pos + 1], key); if (b) *b = descInt(ln, rest[pos + 2], key);
                pos += 1 + cnt;
            };
            values("stride", &L.xs, &L.ys);
            values(kind == "conv" ? "filter" : "window", &L.xf, &L.yf);
            if (kind == "conv") values("filters", &L.nf, nullptr);
            if (kind == "client_maxpool") { values("bits", &L.bits, nullptr); clientTail(pos, true); pos = rest.size(); }
            if (pos != rest.size()) descError(ln, "unknown token '" + rest[pos] + "'");
            if (L.xs < 1 || L.ys < 1 || L.xf < 1 || L.yf < 1) descError(ln, kind + ": strides and window sizes must be positive");
            if (L.xf > xd || L.yf > yd)
                descError(ln, kind + ": the " + to_string(L.xf) + " x " + to_string(L.yf) + " window is larger than its " + to_string(xd) + " x " + to_string(yd) + " input");
            if (!windowOk(xd, yd, L.xs, L.ys, L.xf, L.yf))
                descError(ln, kind + ": stride " + to_string(L.xs) + " x " + to_string(L.ys) + " over a " + to_string(L.xf) + " x " + to_string(L.yf) +
                    " window leaves a remainder of the " + to_string(xd) + " x " + to_string(yd) + " input without outputs");
            L.zo = zd; L.xo = (xd - L.xf) / L.xs + 1; L.yo = (yd - L.yf) / L.ys + 1;
            if (kind == "conv") {
                if (L.nf < 1) descError(ln, "conv: filters must be positive");
                L.zo = L.nf;
                check(ln, L.name + ".weight", (long long)L.nf * zd * L.xf * L.yf); check(ln, L.name + ".bias", L.nf);
            }
        } else if (kind == "fc") {
            if (rest.size() != 1) descError(ln, rest.size() > 1 ? "unknown token '" + rest[1] + "'" : string("fc: out_dim is missing"));
            L.out_dim = descInt(ln, rest[0], "out_dim");
            if (L.out_dim < 1) descError(ln, "fc: out_dim must be positive");
            if ((long long)zd * xd * yd > 0x7fffffffLL) descError(ln, "fc: the input is too large");
            check(ln, L.name + ".weight", (long long)zd * xd * yd * L.out_dim); check(ln, L.name + ".bias", L.out_dim);
            L.zo = 1; L.xo = L.out_dim; L.yo = 1;
        } else if (kind == "pad") {
            if (rest.size() != 2) descError(ln, rest.size() > 2 ? "unknown token '" + rest[2] + "'" : string("pad: takes px py"));
            L.px = descInt(ln, rest[0], "pad"); L.py = descInt(ln, rest[1], "pad");
            L.zo = zd; L.xo = xd + 2 * L.px; L.yo = yd + 2 * L.py;
        } else if (kind == "rescale") {
            if (rest.size() != 1) descError(ln, rest.size() > 1 ? "unknown token '" + rest[1] + "'" : string("rescale: takes the scale's bit count"));
            L.bits = descInt(ln, rest[0], "rescale");
            if (L.bits > 30) descError(ln, "rescale: the bit count must be in 0..30");
            L.zo = zd; L.xo = xd; L.yo = yd;
        } else if (kind == "client_relu") {
            if (rest.empty()) descError(ln, "client_relu: takes the scale's bit count");
            L.bits = descInt(ln, rest[0], "client_relu");
            clientTail(1, false);
            L.relu = true;
            L.zo = zd; L.xo = xd; L.yo = yd;
        } else if (kind == "poly") {
            if (rest.size() != 3) descError(ln, rest.size() > 3 ? "unknown token '" + rest[3] + "'" : string("poly: takes c2 c1 c0"));
            L.c2 = descFloat(ln, rest[0], "c2"); L.c1 = descFloat(ln, rest[1], "c1"); L.c0 = descFloat(ln, rest[2], "c0");
            if (L.c2 == 0.0f) descError(ln, "poly: c2 must not be zero (without its square term the layer is a batch norm, not an activation)");
            L.zo = zd; L.xo = xd; L.yo = yd;
        } else if (kind == "poly3") {
            if (rest.size() != 4) descError(ln, rest.size() > 4 ? "unknown token '" + rest[4] + "'" : string("poly3: takes c3 c2 c1 c0"));
            L.c3 = descFloat(ln, rest[0], "c3"); L.c2 = descFloat(ln, rest[1], "c2"); L.c1 = descFloat(ln, rest[2], "c1"); L.c0 = descFloat(ln, rest[3], "c0");
            if (L.c3 == 0.0f) descError(ln, "poly3: c3 must not be zero (without its cubic term the layer is a poly layer)");
            L.zo = zd; L.xo = xd; L.yo = yd;
        } else {
            if (!rest.empty()) descError(ln, "unknown token '" + rest[0] + "'");
            if (kind == "bn") { check(ln, L.name + ".running_mean", zd); check(ln, L.name + ".running_var", zd); }
            L.zo = zd; L.xo = xd; L.yo = yd;
        }
        if (pending_refresh) { d.layer_before_reenc = (int)d.layers.size(); pending_refresh = 0; }
        d.layers.push_back(L);
        zd = L.zo; xd = L.xo; yd = L.yo;
        flat = flat || kind == "fc";
    }
    if (!have_input) descError(1, "the first line must be `input zd xd yd`");
    if (pending_refresh) descError(pending_refresh, "refresh must be followed by a layer");
    d.refresh_line = refresh_line;
    if (d.layers.empty()) descError(ln, "the description has no layers");
    return d;
}
NetworkDescription NetworkDescription::load(const string &what, const string &h5_path)
{
    if (what.find('\n') != string::npos) return parse(what, h5_path);
    if (const char *text = builtinDescription(what)) return parse(text, h5_path);
    ifstream f(what);
    if (!f) throw invalid_argument("unknown model " + what + ": neither a built-in model nor a readable description file");
    stringstream ss; ss << f.rdbuf();
    return parse(ss.str(), h5_path);
}
string NetworkDescription::str() const
{
    ostringstream o;
    o << "input " << zd << " " << xd << " " << yd << "\n";
    for (size_t i = 0; i < layers.size(); i++) {
        const LayerSpec &L = layers[i];
        if ((int)i == layer_before_reenc) o << "refresh\n";
        o << L.kind << " " << L.name;
        if (L.kind == "conv") o << " stride " << L.xs << " " << L.ys << " filter " << L.xf << " " << L.yf << " filters " << L.nf;
        else if (L.kind == "pool" || L.kind == "avgpool") o << " stride " << L.xs << " " << L.ys << " window " << L.xf << " " << L.yf;
        else if (L.kind == "fc") o << " " << L.out_dim;
        else if (L.kind == "pad") o << " " << L.px << " " << L.py;
        else if (L.kind == "rescale") o << " " << L.bits;
        else if (L.kind == "client_relu") o << " " << L.bits << (L.has_cap ? " cap " + descFloatStr(L.cap) : string());
        else if (L.kind == "client_maxpool")
            o << " stride " << L.xs << " " << L.ys << " window " << L.xf << " " << L.yf << " bits " << L.bits << (L.relu ? " relu" : "")
              << (L.has_cap ? " cap " + descFloatStr(L.cap) : string());
        else if (L.kind == "poly") o << " " << descFloatStr(L.c2) << " " << descFloatStr(L.c1) << " " << descFloatStr(L.c0);
        else if (L.kind == "poly3") o << " " << descFloatStr(L.c3) << " " << descFloatStr(L.c2) << " " << descFloatStr(L.c1) << " " << descFloatStr(L.c0);
        if (L.threads >= 0 && L.threads != 1) o << " threads " << L.threads;          // (1 is what a layer without the token is built with)
        o << "\n";
    }
    return o.str();
}
string Network::describe() const
{
    if (fused_) throw logic_error("Network::describe: fuse() has folded layers; describe the network before it is fused");
    NetworkDescription d;
    d.zd = input_zd; d.xd = input_xd; d.yd = input_yd; d.layer_before_reenc = layer_before_reenc;
    for (auto &l : layers) {
        LayerSpec L; L.name = l->name;
        if (L.name.empty() || L.name.find_first_of(" \t\n#") != string::npos) throw logic_error("Network::describe: layer name '" + L.name + "' cannot be written");
        if (auto c = dynamic_pointer_cast<ConvolutionalLayer>(l)) { L.kind = "conv"; L.xs = c->xs; L.ys = c->ys; L.xf = c->xf; L.yf = c->yf; L.nf = c->nf;
            L.threads = c->th_count; }
        else if (auto f = dynamic_pointer_cast<FullyConnectedLayer>(l)) { L.kind = "fc"; L.out_dim = f->out_dim; L.threads = f->th_count; }
        else if (auto p = dynamic_pointer_cast<PoolingLayer>(l)) { L.kind = dynamic_pointer_cast<AvgPoolingLayer>(l) ? "avgpool" : "pool"; L.xs = p->xs; L.ys = p->ys;
            L.xf = p->xf; L.yf = p->yf; }
        else if (auto pd = dynamic_pointer_cast<PaddingLayer>(l)) { L.kind = "pad"; L.px = pd->px; L.py = pd->py; }
        else if (auto sq = dynamic_pointer_cast<SquareLayer>(l)) { L.kind = "square"; L.threads = sq->th_count; }
        else if (auto po = dynamic_pointer_cast<PolyLayer>(l)) { L.kind = "poly"; L.c2 = po->c2; L.c1 = po->c1; L.c0 = po->c0; L.threads = po->th_count; }
        else if (auto p3 = dynamic_pointer_cast<Poly3Layer>(l)) { L.kind = "poly3"; L.c3 = p3->c3; L.c2 = p3->c2; L.c1 = p3->c1; L.c0 = p3->c0;
            L.threads = p3->th_count; }
        else if (dynamic_pointer_cast<BatchNormLayer>(l)) L.kind = "bn";
        else if (auto rs = dynamic_pointer_cast<SlotRescaleLayer>(l)) { L.kind = "rescale"; L.bits = rs->bits; }
        else if (auto cr = dynamic_pointer_cast<SlotReluLayer>(l)) { L.kind = "client_relu"; L.bits = cr->bits; L.has_cap = cr->cap_value != 0; L.cap = cr->cap_value; }
        else if (auto cm = dynamic_pointer_cast<SlotMaxPoolLayer>(l)) { L.kind = "client_maxpool"; L.xs = cm->xs; L.ys = cm->ys; L.xf = cm->xf; L.yf = cm->yf;
            L.bits = cm->bits; L.relu = cm->relu; L.has_cap = cm->cap_value != 0; L.cap = cm->cap_value; }
        else throw logic_error("Network::describe: layer " + l->name + " has no description");
        d.layers.push_back(L);
    }
    // (parsing the text back infers every shape again and so checks that the layers fit each other)
    return NetworkDescription::parse(d.str()).str();
}

// ---- CnnBuilder -------------------------------------------------------------------------------------------------------
vector<float> CnnBuilder::getPretrained(string var_name)
{   // LoadH5::getData, cnnBuilder.cpp:20-23
    size_t cnt = 0;
    int rc = crc_h5_dataset_count(plain_model_path.c_str(), var_name.c_str(), &cnt);
    if (rc) throw runtime_error("cannot read dataset " + var_name + " from " + plain_model_path + ": " + crc_strerror(rc));
    vector<float> v(cnt);
    chk(crc_h5_read_f32(plain_model_path.c_str(), var_name.c_str(), v.data(), cnt, nullptr), "crc_h5_read_f32");
    return v;
}
// `which`: 0 the layer's first dataset (weights, mean), 1 its second (biases, invstd) -- slot encoding takes the scale the ledger set for it
static vector<Plaintext> encodeAll(const vector<float> &v, int which)
{
    if (g_slot_on) {
        const double scale = g_enc_scale[which];
        if (scale == 0) throw logic_error("slot encoding: layers with parameters are built from a description (CnnBuilder::buildNetworkFromDescription)");
        vector<Plaintext> out(v.size());
        crc_host::parallel_for(v.size(), 1024, [&](size_t b, size_t e) { for (size_t i = b; i < e; i++) out[i] = scalarPlain((double)v[i], scale); });
        return out;
    }
    // compact form (crc_encode_f32_compact: the 96 coefficients the encoder can set), encoded and turned into Plaintexts on the host threads
    // (csrc/host_parallel.h)
    const int n = N();
    vector<uint64_t> cp(v.size() * (size_t)CRC_PLAIN_COMPACT_WORDS); vector<int32_t> cc(v.size());
    chk(crc_encode_f32_compact(ctx(), v.data(), v.size(), cp.data(), cc.data()), "crc_encode_f32_compact");
    vector<Plaintext> out(v.size());
    crc_host::parallel_for(v.size(), 256, [&](size_t b, size_t e) {
        for (size_t i = b; i < e; i++) {
            const uint64_t *row = cp.data() + i * CRC_PLAIN_COMPACT_WORDS;
            Plaintext &p = out[i]; p.coeff_count_ = cc[i];
            for (int j = 0; j < CRC_PLAIN_COMPACT_LOW; j++) if (row[j]) p.nz.emplace_back(j, row[j]);
            for (int j = 0; j < CRC_PLAIN_COMPACT_HIGH; j++) if (row[CRC_PLAIN_COMPACT_LOW + j]) p.nz.emplace_back(n - CRC_PLAIN_COMPACT_HIGH + j,
                row[CRC_PLAIN_COMPACT_LOW + j]);
        }
    });
    return out;
}
ConvolutionalLayer *CnnBuilder::buildConvolutionalLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count,
    istream *infile)
{   // cnnBuilder.cpp:25-50
    if (infile != NULL) return new ConvolutionalLayer(name, xd, yd, zd, xs, ys, xf, yf, nf, th_count, infile);
    vector<float> weights = getPretrained(name + ".weight"), biases = getPretrained(name + ".bias");
    if ((int)weights.size() != nf * zd * xf * yf || (int)biases.size() != nf) throw invalid_argument("conv: dataset size does not match the layer");
    vector<Plaintext> ew = encodeAll(weights, 0), eb = encodeAll(biases, 1);
    plaintext4D encoded_weights(nf, plaintext3D(zd, plaintext2D(xf, vector<Plaintext>(yf))));
    size_t w = 0;
    for (int n = 0; n < nf; n++) for (int z = 0; z < zd; z++) for (int i = 0; i < xf; i++) for (int j = 0; j < yf; j++) encoded_weights[n][z][i][j] = ew[w++];
    return new ConvolutionalLayer(name, xd, yd, zd, xs, ys, xf, yf, nf, th_count, encoded_weights, eb);
}
FullyConnectedLayer *CnnBuilder::buildFullyConnectedLayer(string name, int in_dim, int out_dim, int th_count, istream *infile)
{   // cnnBuilder.cpp:53-76
    if (infile != NULL) return new FullyConnectedLayer(name, in_dim, out_dim, th_count, infile);
    vector<float> weights = getPretrained(name + ".weight"), biases = getPretrained(name + ".bias");
    if ((int)weights.size() != in_dim * out_dim || (int)biases.size() != out_dim) throw invalid_argument("fc: dataset size does not match the layer");
    vector<Plaintext> ew = encodeAll(weights, 0), eb = encodeAll(biases, 1);
    plaintext2D encoded_weights(out_dim, vector<Plaintext>(in_dim));
    size_t w = 0;
    for (int i = 0; i < out_dim; i++) for (int j = 0; j < in_dim; j++) encoded_weights[i][j] = ew[w++];
    return new FullyConnectedLayer(name, in_dim, out_dim, th_count, encoded_weights, eb);
}
PoolingLayer *CnnBuilder::buildPoolingLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf) { return new PoolingLayer(name, xd, yd, zd,
    xs, ys, xf, yf); }
AvgPoolingLayer *CnnBuilder::buildAvgPoolingLayer(string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf) { return new AvgPoolingLayer(name, xd,
    yd, zd, xs, ys, xf, yf); }
SquareLayer *CnnBuilder::buildSquareLayer(string name, int th_count) { return new SquareLayer(name, th_count); }
PolyLayer *CnnBuilder::buildPolyLayer(string name, float c2, float c1, float c0, int th_count) { return new PolyLayer(name, c2, c1, c0, th_count); }
Poly3Layer *CnnBuilder::buildPoly3Layer(string name, float c3, float c2, float c1, float c0, int th_count) { return new Poly3Layer(name, c3, c2, c1, c0, th_count); }
BatchNormLayer *CnnBuilder::buildBatchNormLayer(string name, int num_channels, istream *infile)
{   // cnnBuilder.cpp:89-105
    if (infile != NULL) return new BatchNormLayer(name, num_channels, infile);
    vector<float> mean = getPretrained(name + ".running_mean"), var = getPretrained(name + ".running_var");
    if ((int)mean.size() != num_channels || (int)var.size() != num_channels) throw invalid_argument("bn: dataset size does not match the layer");
    vector<float> invstd(var.size());
    chk(crc_bn_invstd_f32(var.data(), var.size(), invstd.data()), "crc_bn_invstd_f32");
    vector<Plaintext> em = encodeAll(mean, 0), ev = encodeAll(invstd, 1);
    return new BatchNormLayer(name, num_channels, em, ev);
}
Network CnnBuilder::buildNetwork(string file_name) { return buildNetworkByName("PlainModelTiny", file_name); }
PaddingLayer *CnnBuilder::buildPaddingLayer(string name, int xd, int yd, int zd, int px, int py) { return new PaddingLayer(name, xd, yd, zd, px, py); }
// the three networks of cnnBuilder.cpp:115-169 come from their descriptions (crcnn_amd/models/*.net, compiled in): same build*Layer calls, same arguments
Network CnnBuilder::buildNetworkByName(const string &model, string file_name) { return buildNetworkFromDescription(model, file_name); }
// ---- the scale ledger of slot encoding ---------------------------------------------------------------------------------------
// a * b for integer-valued doubles below 2^62, exact or std::invalid_argument
static double scaleTimes(int line, double a, double b)
{
    const unsigned __int128 z = (unsigned __int128)(uint64_t)a * (uint64_t)b;
    const double r = (double)(uint64_t)z;
    if ((z >> 62) || (unsigned __int128)(uint64_t)r != z) descError(line, "slot encoding: the scale leaves the integers below 2^62 that a double holds exactly");
    return r;
}
vector<double> slotScales(const NetworkDescription &d, int input_bits, int weight_bits)
{
    if (input_bits < 0 || input_bits > 30 || weight_bits < 0 || weight_bits > 30) throw invalid_argument("slotScales: bit counts must be in 0..30");
    if (d.layer_before_reenc >= 0) descError(d.refresh_line, "refresh is not available with slot encoding (it would need a slot-wise re-encoding)");
    const double W = ldexp(1.0, weight_bits);
    double s = ldexp(1.0, input_bits);
    vector<double> out;
    for (const LayerSpec &L : d.layers) {
        out.push_back(s);
        if (L.kind == "conv" || L.kind == "fc" || L.kind == "bn") s = scaleTimes(L.line, s, W);
        else if (L.kind == "avgpool") s = scaleTimes(L.line, s, (double)(L.xf * L.yf));
        else if (L.kind == "square") s = scaleTimes(L.line, s, s);
        else if (L.kind == "poly") s = scaleTimes(L.line, scaleTimes(L.line, s, s), W);
        else if (L.kind == "poly3") s = scaleTimes(L.line, scaleTimes(L.line, scaleTimes(L.line, s, s), s), W);
        else if (L.kind == "rescale" || L.kind == "client_relu" || L.kind == "client_maxpool") {
            // the client divides every slot by sigma / 2^bits: an integer >= 1, or the line is refused
            const double target = ldexp(1.0, L.bits);
            if (s < target || fmod(s, target) != 0) descError(L.line, L.kind + ": the scale 2^" + to_string(L.bits) + " does not divide the scale in front of it");
            s = target;
        }
    }
    out.push_back(s);
    return out;
}
Network CnnBuilder::buildNetworkFromDescription(const string &path_or_text, string file_name)
{
    // (an encoded-model file brings its own parameters: the HDF5 datasets are not consulted then, as in build*Layer)
    const NetworkDescription d = NetworkDescription::load(path_or_text, file_name == "" ? plain_model_path : string());
    Network net;
    unique_ptr<ifstream> infile;
    if (file_name != "") { infile.reset(new ifstream(file_name, ifstream::binary)); if (!*infile) throw runtime_error("cannot open " + file_name); }
    istream *in = infile.get();
    auto add = [&](Layer *l) { net.getLayers().push_back(shared_ptr<Layer>(l)); };
    // slot encoding: the ledger says at which scale every plaintext of the layer is an integer (slotScales)
    const vector<double> sigma = g_slot_on ? slotScales(d, g_slot_in_bits, g_slot_w_bits) : vector<double>();
    const double W = ldexp(1.0, g_slot_w_bits);
    struct ScaleScope { ~ScaleScope() { g_enc_scale[0] = g_enc_scale[1] = 0; } } scale_scope;
    size_t li = 0;
    for (const LayerSpec &L : d.layers) {
        const int th = L.threads >= 0 ? L.threads : 1;
        const double s = g_slot_on ? sigma[li] : 0;
        li++;
        if (g_slot_on) {
            if (L.kind == "bn") { g_enc_scale[0] = s; g_enc_scale[1] = W; }
            else { g_enc_scale[0] = W; g_enc_scale[1] = s * W; }
        }
        if (L.kind == "rescale") {
            if (!g_slot_on) descError(L.line, "rescale needs slot encoding (setSlotEncoding)");
            SlotRescaleLayer *r = new SlotRescaleLayer(L.name, L.bits);
            r->divisor = (uint64_t)(s / ldexp(1.0, L.bits));
            add(r);
        }
        else if (L.kind == "client_relu" || L.kind == "client_maxpool") {
            if (!g_slot_on) descError(L.line, L.kind + " needs slot encoding (setSlotEncoding)");
            const double capq = L.has_cap ? nearbyint((double)L.cap * ldexp(1.0, L.bits)) : 0;
            if (capq > (double)((g_plain_modulus - 1) / 2)) descError(L.line, L.kind + ": the cap exceeds (t - 1) / 2 at the scale 2^" + to_string(L.bits));
            const uint64_t divisor = (uint64_t)(s / ldexp(1.0, L.bits));
            if (L.kind == "client_relu") { SlotReluLayer *r = new SlotReluLayer(L.name, L.bits, L.has_cap ? L.cap : 0.0f); r->divisor = divisor; r->cap = (uint64_t)capq; add(r); }
            else {
                SlotMaxPoolLayer *r = new SlotMaxPoolLayer(L.name, L.xs, L.ys, L.xf, L.yf, L.bits, L.relu, L.has_cap ? L.cap : 0.0f);
                r->divisor = divisor; r->cap = (uint64_t)capq; add(r);
            }
        }
        else if (L.kind == "conv") add(buildConvolutionalLayer(L.name, L.xd, L.yd, L.zd, L.xs, L.ys, L.xf, L.yf, L.nf, th, in));
        else if (L.kind == "pool") add(buildPoolingLayer(L.name, L.xd, L.yd, L.zd, L.xs, L.ys, L.xf, L.yf));
        else if (L.kind == "avgpool") add(buildAvgPoolingLayer(L.name, L.xd, L.yd, L.zd, L.xs, L.ys, L.xf, L.yf));
        else if (L.kind == "bn") add(buildBatchNormLayer(L.name, L.zd, in));
        else if (L.kind == "square") add(buildSquareLayer(L.name, th));
        else if (L.kind == "poly") {
            PolyLayer *p = buildPolyLayer(L.name, L.c2, L.c1, L.c0, th);
            if (g_slot_on) { p->slot_scale[0] = W; p->slot_scale[1] = W * s; p->slot_scale[2] = W * s * s; }
            add(p);
        } else if (L.kind == "poly3") {
            Poly3Layer *p = buildPoly3Layer(L.name, L.c3, L.c2, L.c1, L.c0, th);
            if (g_slot_on) { p->slot_scale[0] = W; p->slot_scale[1] = W * s; p->slot_scale[2] = W * s * s; p->slot_scale[3] = W * s * s * s; }
            add(p);
        }
        else if (L.kind == "fc") add(buildFullyConnectedLayer(L.name, L.zd * L.xd * L.yd, L.out_dim, th, in));
        else add(buildPaddingLayer(L.name, L.xd, L.yd, L.zd, L.px, L.py));
    }
    net.input_zd = d.zd; net.input_xd = d.xd; net.input_yd = d.yd;
    net.layer_before_reenc = d.layer_before_reenc;
    net.slot_scale_ = g_slot_on ? sigma.back() : 0;
    return net;
}
Network CnnBuilder::buildAndSaveNetwork(string file_name)
{   // cnnBuilder.cpp:181-196
    ofstream outfile(file_name, ofstream::binary);
    Network net = buildNetwork();
    for (int i = 0; i < net.getNumLayers(); i++) net.getLayer(i)->savePlaintextParameters(&outfile);
    outfile.close();
    return net;
}
