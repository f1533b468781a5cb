// crcnn_host.h -- C++ host side of the engine: the reference's layer / network / builder interface, same names, same
// constructor argument order, same error behaviour (exceptions), implemented purely on the C ABI of include/crcnn_hip.h.
//
// What differs from CrCNN by design (MI355X-first):
//   * `ciphertext3D` is a handle to a device-resident tensor of ciphertexts [B][z][x][y] (B = image batch, 1 for the
//     reference's single-image calls) instead of nested std::vectors of SEAL objects (CrCNN/src/globals.h:10-16);
//     copying the handle is cheap, layers never modify their argument.
//   * `Plaintext` keeps the sparse balanced-ternary coefficients of an encoded weight (<= 96 non-zeros) instead of a dense
//     n+1 word array; its save/load wire format is SEAL's (plaintext.cpp:346-363) so encoded-model files interchange.
//   * th_count arguments are accepted and ignored (parallelism is the GPU's).
#pragma once
#include <cstdint>
#include <functional>
#include <istream>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/crcnn_hip.h"

// ---- plaintext / tensor types (CrCNN/src/globals.h:10-16) -----------------------------------------------------------
class Plaintext {
public:
    int coeff_count_ = 0;                                   // SEAL's Plaintext::coeff_count()
    std::vector<std::pair<int, uint64_t>> nz;               // (index, coefficient) for non-zero coefficients
    int coeff_count() const { return coeff_count_; }
    bool is_zero() const { return nz.empty(); }
    void save(std::ostream &stream) const;                  // SEAL wire format: int32 coeff_count, then uint64 coefficients
    void load(std::istream &stream);
    void dense(uint64_t *out, int n) const;                 // zero-extended to n coefficients
};
typedef std::vector<std::vector<std::vector<Plaintext>>> plaintext3D;
typedef std::vector<std::vector<Plaintext>> plaintext2D;
typedef std::vector<std::vector<std::vector<std::vector<Plaintext>>>> plaintext4D;
typedef std::vector<std::vector<std::vector<std::vector<float>>>> floatHypercube;
typedef std::vector<std::vector<std::vector<float>>> floatCube;

struct DeviceBuffer { void *ptr = nullptr; size_t bytes = 0; DeviceBuffer(size_t b); ~DeviceBuffer(); DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete; };

class ciphertext3D {          // device tensor of size-2 ciphertexts, [B][zd][xd][yd]
public:
    int B = 0, zd = 0, xd = 0, yd = 0, form = CRC_COEFF;
    std::shared_ptr<DeviceBuffer> buf;
    size_t offset = 0;        // bytes into buf: images() hands out views of a batch without copying it
    ciphertext3D() {}
    ciphertext3D(int B, int zd, int xd, int yd, int form = CRC_COEFF);
    size_t count() const { return (size_t)B * zd * xd * yd; }
    uint64_t *data() const { return buf ? (uint64_t *)((char *)buf->ptr + offset) : nullptr; }
    ciphertext3D images(int b0, int count) const;             // view of images [b0, b0 + count) (ciphertext forms only)
    // CrCNN code indexes input[0].size() etc.; the equivalents:
    int size() const { return zd; }
    static ciphertext3D fromHost(const uint64_t *h, int B, int zd, int xd, int yd);    // h: [B][zd][xd][yd][2][k][n]
    std::vector<uint64_t> toHost() const;
};
ciphertext3D stackImages(const std::vector<ciphertext3D> &images);      // B=1 tensors -> one batch
ciphertext3D deepCopyImage(const ciphertext3D &image);                  // globals.cpp:159-171

// ---- process-global crypto context (CrCNN/src/globals.h:18-48) --------------------------------------------------------
extern crc_ctx *context;                                    // the engine context (SEALContext + Evaluator tables)
// the HIP stream (hipStream_t behind void*; crc_stream_create makes one) all layer calls, copies and synchronisations of these classes go to; NULL = the
// default stream.  Install it before the first forward(); the caller keeps ownership and orders its own streams against it with events
// Announce the number of images a Network::forward will get (0 = unknown, the default) BEFORE the layers' weights are placed (fuse(), broadcastParameters(),
// the first forward()): a deployment that evaluates one image at a time keeps every dense layer's canonical weights resident and streams them, where a batched
// one may drop them for the matrix-core form (PlainModelWoPad's fc3 at n = 16384 has room for one of the two)
void setExpectedBatch(int images_per_forward);
void setStream(void *stream);
void *getStream();
extern std::vector<uint64_t> secret_key, public_key, ev_keys16_host;
extern std::shared_ptr<DeviceBuffer> ev_keys16;             // evaluation keys, dbc = 16, resident in HBM
// Client-side randomness (secret key, evaluation keys, every encryption).  The reference draws from std::random_device (SEAL 2.3.1
// randomgen.cpp:7); here setParameters() draws a fresh 256-bit ChaCha20 key from the OS (crc_random_key -> getrandom(2)) on every
// call and each encryption uses its own keystream under it.  setDeterministicSeed() replaces that by a PUBLIC 64-bit seed so that
// tests, benchmarks and golden vectors are reproducible -- a seeded run is NOT secure (anyone who knows the seed can decrypt).
void setDeterministicSeed(uint64_t seed);                   // tests / bench only; takes effect at the next setParameters()
void clearDeterministicSeed();                              // back to OS entropy (the default)
void setParameters(int poly_modulus = 4096, uint64_t plain_modulus = 1 << 20);          // coeff_modulus_128(poly_modulus)
void setParameters(int poly_modulus, const std::vector<uint64_t> &coeff_modulus, uint64_t plain_modulus, int device = 0);
void delParameters();
// Slot-batched inference (include/crcnn_hip.h, "Slot batching"): with a prime plain modulus t = 1 (mod 2n) one ciphertext tensor carries up to n images, image j
// in slot j of every ciphertext, through the same layers.  setSlotEncoding switches the encoding of everything these classes turn into plaintexts from the
// fractional encoder to SCALARS: the constant polynomial of nearbyint(value * scale) mod t (round half even on doubles), the same number in every slot.  Pixels
// are scaled by 2^input_bits, weights by 2^weight_bits, and every other plaintext by what CnnBuilder::buildNetworkFromDescription's scale ledger says (below,
// slotScales).  Both throw std::invalid_argument when crc_slots_supported(context) is 0 or a bit count is outside 0..30.  Off by default and after every
// setParameters(); with it off every path is what it is without these calls.
void setSlotEncoding(int input_bits, int weight_bits);
void clearSlotEncoding();
bool slotEncoding();
// key / ciphertext files in SEAL's wire formats, interchangeable with CrCNN's (globals.cpp:58-111, 174-205)
void setAndSaveParameters(std::string public_key_path, std::string secret_key_path, std::string evaluation_key_path, int poly_modulus, uint64_t plain_modulus);
void initFromKeys(std::string public_key_path, std::string secret_key_path, std::string evaluation_key_path, int poly_modulus, uint64_t plain_modulus);
ciphertext3D encryptAndSaveImage(std::vector<float> image, int zd, int xd, int yd, std::string file_name);
ciphertext3D loadEncryptedImage(int zd, int xd, int yd, std::string file_name);
Plaintext fraencode(double value);                          // fraencoder->encode(value)
double fradecode(const std::vector<uint64_t> &plain);
ciphertext3D encryptImage(std::vector<float> image, int zd, int xd, int yd);             // globals.cpp:127-142
ciphertext3D encryptImage(floatCube image);                                              // globals.cpp:144-157
std::vector<floatCube> decryptImages(const ciphertext3D &encrypted);                     // one floatCube per image of the batch
floatCube decryptImage(const ciphertext3D &encrypted_image);                             // globals.cpp:207-230 (B must be 1)
int noiseBudget(const ciphertext3D &t, size_t index = 0);
// Decryptor::invariant_noise_budget of EVERY ciphertext of a tensor, on the device and on the launch stream (crc_noise_budget_dev; the device copy of the secret
// key the refresh keeps, the layers' scratch area): the integers noiseBudget(t, i) gives, in [B][zd][xd][yd] order.  CRC_COEFF and CRC_NTT tensors (an
// NTT-resident tensor is measured as it stands); std::invalid_argument for the packed and limb forms.  Both calls wait for the stream.
std::vector<int> noiseBudgets(const ciphertext3D &t);
// the smallest budget of the tensor and (optionally) the index of the first ciphertext that has it: two integers come back over PCIe, not the tensor
int minNoiseBudget(const ciphertext3D &t, size_t *where = nullptr);
// ---- levels: modulus switching (include/crcnn_hip.h, "Modulus switching") ------------------------------------------------------------------------------------
// A Level is the parameters of setParameters() over the first `kept` coefficient moduli: its own context, and the rows [0, kept) of the secret and the public
// key, which are valid there as they stand (copies taken by makeLevel: a later assignment to the global keys does not reach a level).  Evaluation and Galois
// keys do NOT carry over to a plain level; nothing here generates them, the layers run at the full modulus.  A level belongs to the parameters it was made
// under: after the next setParameters() / delParameters() every call that is handed it, or a LevelTensor of it, throws std::invalid_argument.
// A DERIVED level (makeLevel(kept, true)) is made by crc_ctx_create_level: its key-switching gadget stays that of the parameters, and it holds device copies of
// the evaluation keys, the installed Galois keys and their conjugated blobs RESTRICTED from the global ones on the device (crc_keys_restrict_dev) -- the secret
// key is not touched for them, so a server that holds public material only can make one.  squareRelin and rotateRows run there.
struct Level {
    crc_ctx *ctx = nullptr;                                 // owned
    int kept = 0;
    uint64_t generation = 0;
    std::vector<uint64_t> secret_key, public_key;           // [kept][n] and [2][kept][n], NTT form
    std::shared_ptr<DeviceBuffer> d_secret_key;
    std::shared_ptr<DeviceBuffer> d_public_key;             // uploaded by the first floodImages at this level
    // a derived level's keys (null / empty on a plain one): what ev_keys16 and the Galois key set were when makeLevel ran
    bool derived = false;
    std::shared_ptr<DeviceBuffer> d_ev_keys16, d_galois_keys, d_galois_ckeys;
    std::vector<uint64_t> galois_elts;
    int galois_dbc = 0;
    Level() {}
    ~Level();
    Level(const Level &) = delete; Level &operator=(const Level &) = delete;
};
// valid after setParameters() / initFromKeys(); std::invalid_argument for `kept` outside 1 .. k - 1
std::shared_ptr<Level> makeLevel(int kept, bool derive_keys = false);
// a device tensor of size-2 ciphertexts of a level, [B][zd][xd][yd][2][kept][n] -- what a server sends back at a fraction of the bytes
struct LevelTensor {
    int B = 0, zd = 0, xd = 0, yd = 0, form = CRC_COEFF;
    std::shared_ptr<Level> level;
    std::shared_ptr<DeviceBuffer> buf;
    size_t count() const { return (size_t)B * zd * xd * yd; }
    uint64_t *data() const { return buf ? (uint64_t *)buf->ptr : nullptr; }
    std::vector<uint64_t> toHost() const;
    // the ciphertexts back to back in SEAL's Ciphertext::save format under the LEVEL's parameter hash (crc_seal_ct_save on the level's context), count() times
    // crc_seal_ct_bytes(level->ctx, 2) bytes; coefficient form only.  load: std::invalid_argument for a file of other parameters (another level among them), a
    // truncated one or one that holds more than [B][zd][xd][yd]
    void save(const std::string &path) const;
    static LevelTensor load(const std::shared_ptr<Level> &level, int B, int zd, int xd, int yd, const std::string &path);
};
// crc_mod_switch_forms on the launch stream, work space from the layers' scratch area: a CRC_COEFF or CRC_NTT tensor of the global context -> the level `to`, in
// out_form (CRC_COEFF / CRC_NTT).  Asynchronous.  The plaintexts are unchanged; the budget is at least floor(-log2(2^-b + t (n + 1) / q_to)) - 2 bits
LevelTensor modSwitch(const ciphertext3D &t, const std::shared_ptr<Level> &to, int out_form = CRC_COEFF);
// The two operations that make a DERIVED level worth visiting, on the launch stream with the level's restricted keys: relinearize(square(x)) elementwise, and
// rotateRows' slot rotation (the planner's steps over the level's Galois key set).  CRC_COEFF or CRC_NTT in, out_form out.  std::logic_error for a level that
// was not made with derive_keys (it has no keys) and, for rotateRows, parameters without batching; std::invalid_argument as their ciphertext3D namesakes
LevelTensor squareRelin(const LevelTensor &t, int out_form = CRC_COEFF);
LevelTensor rotateRows(const LevelTensor &t, int steps, int out_form = CRC_COEFF);
// the client side at a level, under the level's secret-key rows: as their ciphertext3D namesakes
std::vector<floatCube> decryptImages(const LevelTensor &t);
std::vector<std::vector<int64_t>> decryptSlots(const LevelTensor &t, int S);
std::vector<int> noiseBudgets(const LevelTensor &t);
int minNoiseBudget(const LevelTensor &t, size_t *where = nullptr);
// ---- noise flooding: sanitise a response before it leaves (include/crcnn_hip.h, "Noise flooding") ------------------------------------------------------------
// The noise of an evaluated ciphertext is a function of the model's weights, and the client who holds the secret key can read it (noiseBudgets).  floodImages
// adds to every ciphertext of a CRC_COEFF or CRC_NTT tensor, in place and on the launch stream (crc_flood_dev, work space from the layers' scratch area), a fresh
// public-key encryption of zero whose first error term is uniform on [-2^flood_bits, 2^flood_bits).  The plaintexts are unchanged; the budget afterwards is at
// least crc_flood_budget_bound(ctx, b, flood_bits) - 2 bits.  A LevelTensor is flooded under its level's public-key rows and context.  Key and counter
// discipline of encryptImage: the master key, a counter that advances by the ciphertext count, and the deterministic seed under setDeterministicSeed.
// std::invalid_argument for a width crc_flood_supported refuses, an empty tensor and the packed and limb forms.
void floodImages(ciphertext3D &t, int flood_bits);
void floodImages(LevelTensor &t, int flood_bits);
// crc_flood_bits on the parameters: the width that covers, by `lambda` bits, the noise of a ciphertext with budget_in bits of budget.  budget_in is the budget the
// server knows A PRIORI for its network (the plain-modulus search's), never a measured one -- measuring needs the secret key, and the measured value is itself a
// function of the weights.  std::invalid_argument where no admissible width exists
int floodBits(int budget_in, int lambda = 40);
// the server's last step: a flooded copy of `t` at the full modulus (t itself is not written), then modSwitch to `to` in out_form
LevelTensor sanitizeResponse(const ciphertext3D &t, int flood_bits, const std::shared_ptr<Level> &to, int out_form = CRC_COEFF);
// ---- several plain moduli: a residue base (include/crcnn_hip.h, "Several plain moduli") -----------------------------------------------------------------------
// A PlainBase is r <= CRC_SLOTS_CRT_MAX contexts over the n, q and device of setParameters() whose slot primes ts[j] are pairwise distinct with T = prod ts[j] <
// 2^63: member 0 is the global context (ts[0] must be its plain modulus), the others are owned sibling contexts.  The keys do not involve t, so the base holds
// device copies of the global secret and public key that serve every member.  The same network runs under every member -- each in a process of its own, whose
// parameters have t = ts[j]: the host classes' process-global context stands in the way of more -- and the slots recombine into integers mod T.  Like a Level a
// base belongs to the parameters it was made under: after the next setParameters() / delParameters() every call that is handed it throws std::invalid_argument.
struct PlainBase {
    std::vector<crc_ctx *> ctxs;                            // [0]: the global context; [1 ..]: owned
    std::vector<uint64_t> ts;
    uint64_t T = 0;
    uint64_t generation = 0;
    std::shared_ptr<DeviceBuffer> d_secret_key, d_public_key;
    PlainBase() {}
    ~PlainBase();
    PlainBase(const PlainBase &) = delete; PlainBase &operator=(const PlainBase &) = delete;
};
// std::invalid_argument unless ts[0] is the plain modulus of the parameters and the contexts are a base (crc_slots_crt_supported)
std::shared_ptr<PlainBase> makePlainBase(const std::vector<uint64_t> &ts);
// r device tensors of one shape and form, member j under ts[j]
struct PlainBaseTensor {
    std::shared_ptr<PlainBase> base;
    std::vector<ciphertext3D> parts;
    int form() const { return parts.empty() ? CRC_COEFF : parts[0].form; }
    size_t count() const { return parts.empty() ? 0 : parts[0].count(); }
};
// encryptImageSlots under every member: the same int64 pixels composed mod every ts[j] (r calls of crc_slots_compose_dev) and encrypted under the one public key,
// keystream discipline as encryptImageSlots (the counter advances by r times the ciphertexts of one member)
PlainBaseTensor encryptImageSlotsCrt(const std::vector<std::vector<int64_t>> &images, int zd, int xd, int yd, const std::shared_ptr<PlainBase> &base,
                                     int out_form = CRC_COEFF);
// the first S slots of every ciphertext as centred integers mod T, [S][count]: crc_decrypt_dev on every member, then ONE crc_slots_crt_decompose_dev
std::vector<std::vector<int64_t>> decryptSlotsCrt(const PlainBaseTensor &t, int S);
// the refresh over the base (crc_slots_crt_refresh[_sym]_dev_key): per slot the lifted integer V -> floor(V / divisor + 1/2), relu: max(., 0), cap (0: none):
// min(., cap), reduced mod every ts[j] and encrypted again.  Key and counter discipline of rescaleSlots (under setDeterministicSeed the key is the public
// expansion of the seed and the counter); bounded passes on the shared scratch.  std::invalid_argument as rescaleSlots, and for a cap above (T - 1) / 2
PlainBaseTensor rescaleSlotsCrt(const PlainBaseTensor &t, uint64_t divisor, int relu, uint64_t cap, int out_form, bool symmetric = false);
// member j as a ciphertext3D (a view, not a copy) for a process whose parameters have t = ts[j], and a tensor of that shape back in its place
ciphertext3D component(const PlainBaseTensor &t, int j);
void setComponent(PlainBaseTensor &t, int j, const ciphertext3D &part);
// decryptImage -> encryptImage for every image of a batch (the refresh Network::forward runs in front of layer_before_reenc, network.cpp:30-34), on the
// device and on the launch stream: the tensor may be in coefficient or NTT form, comes back in `out_form` (CRC_COEFF / CRC_NTT) under fresh randomness, and
// `values` (optional) receives the floats the client saw, [B][zd][xd][yd] -- asking for them makes the call wait for the stream
// `symmetric` (off by default: the reference's refresh calls Encryptor::encrypt): the re-encryption runs under the secret key the refresh holds anyway
// (crc_refresh_sym_dev: c1 uniform in the NTT domain, one forward transform per modulus instead of three, fresh noise e alone) -- another ciphertext
// distribution, the same plaintexts and floats; only the cached device copy of the secret key is needed
ciphertext3D refreshImages(const ciphertext3D &encrypted, int out_form = CRC_COEFF, std::vector<float> *values = nullptr, bool symmetric = false);
// the refresh of a SLOT-BATCHED tensor: decrypt, every slot of every plaintext divided by `divisor` (1..2^62) and rounded to nearest, ties towards +infinity
// (crc_slots_rescale_dev), encrypt under fresh randomness -- crc_slots_refresh[_sym]_dev in bounded passes on the shared scratch, seed / key and counter as
// refreshImages.  CRC_COEFF / CRC_NTT in and out; std::invalid_argument for other forms, a divisor out of range or a context without slots
ciphertext3D rescaleSlots(const ciphertext3D &encrypted, uint64_t divisor, int out_form, bool symmetric = false);
// rescaleSlots with a client-side activation between decrypt and encrypt (crc_slots_refresh_act[_sym]_dev): per slot the maximum over the xf x yf window of
// stride (xs, ys) of every [xd][yd] plane, floor(m / divisor + 1/2), relu: max(., 0), cap (slot units, 0: none): min(., cap).  The result has the window's
// output shape, so a 2 x 2 / 2 window re-encrypts a quarter of what it decrypts.  Same seed / key / counter discipline (the counter advances by the OUTPUT
// ciphertexts) and the same bounded passes on the shared scratch, cut at whole planes.  std::invalid_argument as rescaleSlots, and for a window the library's
// window test refuses, relu outside {0, 1} or a cap above (t - 1) / 2.  The key holder sees the activations at this point, as with every rescale
ciphertext3D actSlots(const ciphertext3D &encrypted, int xs, int ys, int xf, int yf, uint64_t divisor, int relu, uint64_t cap, int out_form, bool symmetric = false);
// encryptImage's sibling for a client that holds the secret key: the pixels of one image ([zd][xd][yd]) or of a batch ([B][zd][xd][yd] floats, B = size /
// (zd xd yd)) encrypted under the secret key on the device (crc_encrypt_sym_dev); same keystream discipline as encryptImage
ciphertext3D encryptImageSymmetric(const std::vector<float> &pixels, int zd, int xd, int yd, int out_form = CRC_COEFF);
ciphertext3D encryptImageSymmetric(floatCube image, int out_form = CRC_COEFF);
// SEEDED images: c1 of a secret-key ciphertext is a function of a PUBLIC seed (include/crcnn_hip.h, "SEEDED secret-key ciphertexts"), so a client sends the
// c0 rows and 32 bytes -- half of what encryptImage's ciphertexts take over a network or PCIe -- and the server regenerates c1 on the device.
struct SeededImages {
    int B = 0, zd = 0, xd = 0, yd = 0;
    std::vector<uint64_t> c0;                               // [B][zd][xd][yd][k][n], NTT form
    uint8_t seed[32] = {0};                                 // PUBLIC
    uint64_t stream_base = 0;
    size_t count() const { return (size_t)B * zd * xd * yd; }
    // four little-endian int32 (B, zd, xd, yd), then the container of crc_seeded_ct_save; load throws std::invalid_argument for anything else
    void save(std::ostream &out) const;
    void load(std::istream &in);
};
// encryption under the global secret_key of one image or a batch ([B][zd][xd][yd] floats), as encryptImageSymmetric takes them.  The PRIVATE noise key
// follows encryptImage's keystream discipline (the master key and the ciphertext counter); the PUBLIC seed is a fresh crc_random_key per call -- under
// setDeterministicSeed both derive from the deterministic seed and the counter, so that tests reproduce
// `on_device` (off by default: the host encryptor, spread over the host threads): the floats go up at 4 bytes per pixel, crc_encrypt_f32_seeded_dev[_key] encodes
// and encrypts them on the installed stream under the cached device copy of the secret key, and the packed rows come back -- the same seed, stream_base and
// counter discipline, and under setDeterministicSeed byte for byte the same SeededImages
SeededImages encryptImageSeeded(const std::vector<float> &pixels, int zd, int xd, int yd, bool on_device = false);
SeededImages encryptImageSeeded(floatCube image, bool on_device = false);
// upload the packed rows on the installed stream and expand them on the device (crc_seeded_expand_dev) into an ordinary tensor of `out_form` CRC_NTT / CRC_COEFF
ciphertext3D expandSeeded(const SeededImages &images, int out_form = CRC_NTT);
// the same for rows that are already on the device (a host that uploads on a copy stream of its own): d_c0 packed [B zd xd yd][k][n], `dst` a tensor of that
// shape whose form says what to produce; asynchronous on the installed stream
void expandSeeded(const uint64_t *d_c0, int B, int zd, int xd, int yd, const uint8_t *seed, uint64_t stream_base, ciphertext3D &dst);

// S images ([S][zd xd yd] pixels each, S <= n) -> ONE tensor [1][zd][xd][yd] whose ciphertext (z, x, y) holds pixel (z, x, y) of image j in slot j: the pixels
// are quantised as nearbyint(double(p) 2^input_bits) (the int64 overload takes them as they are), composed on the device (crc_slots_compose_dev, image-major) and
// encrypted there (crc_encrypt_dev_forms); keystream discipline as encryptImage.  std::logic_error unless setSlotEncoding is on
ciphertext3D encryptImageSlots(const std::vector<std::vector<float>> &images, int zd, int xd, int yd, int out_form = CRC_COEFF);
ciphertext3D encryptImageSlots(const std::vector<std::vector<int64_t>> &images, int zd, int xd, int yd, int out_form = CRC_COEFF);
// the first S slots of every ciphertext of a tensor (CRC_COEFF or CRC_NTT), as centred integers [S][count]: crc_decrypt_dev, then crc_slots_decompose_dev
std::vector<std::vector<int64_t>> decryptSlots(const ciphertext3D &t, int S);
// ... divided by `scale` (Network::slot_scale() of the network that produced the tensor)
std::vector<std::vector<double>> decryptImageSlots(const ciphertext3D &t, int S, double scale);
// Galois keys and the operations that move data between slots (include/crcnn_hip.h, "Galois automorphisms": Evaluator::rotate_rows / rotate_columns of SEAL
// 2.3.1, KeyGenerator::generate_galois_keys).  generateGaloisKeys builds the keys of the default set (2n - 1 and 3^(+-2^i): every rotation in at most log2 n key
// switches) or of the given elements from the global secret_key, keeps them beside the evaluation keys and uploads them once; setParameters() / delParameters()
// drop them.  std::invalid_argument for a dbc outside 1..60 or an invalid element
void generateGaloisKeys(int dbc = 16);
void generateGaloisKeys(int dbc, std::vector<uint64_t> elts);
extern std::vector<uint64_t> galois_elts, galois_keys_host;             // the elements, and their key blobs [elts][crc_evk_words(dbc)]
// SEEDED Galois keys (include/crcnn_hip.h, "SEEDED key-switching keys"): the second polynomial of every key pair is a function of a PUBLIC seed, so a client
// sends the first rows, the elements and 32 bytes -- half of what the blobs take -- and the server regenerates the rest on the device.
struct SeededKeys {
    int dbc = 0;
    std::vector<uint64_t> ids;                              // the Galois elements
    uint8_t seed[32] = {0};                                 // PUBLIC
    std::vector<uint64_t> rows;                             // [ids][P][k][n], NTT form (crc_seeded_key_words(dbc) per element)
    // the container of crc_seeded_keys_save; load throws std::invalid_argument for anything else
    void save(std::ostream &out) const;
    void load(std::istream &in);
};
// the CLIENT side: the first rows of the keys of `elts` from the global secret_key, on the host threads or (`on_device`) on the installed stream under the cached
// device copy of the secret key (crc_gen_keys_seeded[_dev]).  The PRIVATE key is the master key and the PUBLIC seed a function of it (half a keystream block under a domain of its
// own), NOT a fresh draw: the keystreams are named by element, dbc and modulus count alone, so an element made again -- in another set, by another call -- must
// meet the same seed, and is then the same key byte for byte, as under generateGaloisKeys (equal noise around two different masks would give the secret key
// away).  Under setDeterministicSeed both derive from the deterministic seed as generateGaloisKeys' does.  Either way the two paths give the same SeededKeys.  Installs
// nothing.  Exceptions as generateGaloisKeys
SeededKeys generateGaloisKeysSeeded(int dbc, std::vector<uint64_t> elts, bool on_device = false);
// the SERVER side: uploads the rows, expands the blobs and their conjugated forms on the device (crc_seeded_keys_expand_dev) and leaves the Galois key set as
// generateGaloisKeys(keys.dbc, keys.ids) would: every rotation, matvecSlots*, convSlots and densePlanes call works unchanged.  No secret key is needed and none
// is read; galois_keys_host stays empty (the blobs exist on the device only).  std::invalid_argument for a bad dbc, an invalid element or rows of another size
void installGaloisKeys(const SeededKeys &keys);
// Every ciphertext of the tensor rotated (CRC_COEFF / CRC_NTT in, out_form CRC_COEFF / CRC_NTT out; a new tensor of the same shape).  The n slots are a
// 2 x n/2 matrix: rotateRows puts old slot (i + steps) mod n/2 of each row at slot i (to the left for positive steps), rotateColumns swaps the rows, sumSlots
// leaves the sum of all n slots in every slot.  As in the reference: std::logic_error when the parameters do not support batching, std::invalid_argument for
// |steps| >= n/2 ("step count too large"), a key that is not in the set ("galois key not present") and the other operand forms
ciphertext3D rotateRows(const ciphertext3D &t, int steps, int out_form = CRC_COEFF);
ciphertext3D rotateColumns(const ciphertext3D &t, int out_form = CRC_COEFF);
ciphertext3D sumSlots(const ciphertext3D &t, int out_form = CRC_COEFF);
// Hoisted rotations (include/crcnn_hip.h, "Hoisted rotations"): generateGaloisKeys also keeps every key's CONJUGATED blob on the device, and rotateRowsMany
// rotates every ciphertext of the tensor by each of `steps` from ONE digit decomposition -- result r is what rotateRows(t, steps[r]) decrypts to, in a ciphertext
// of its own definition (not rotateRows' bits), as a view of one shared buffer.  Every step's element 3^steps needs ITS OWN key in the set: no chain of steps is
// planned ("galois key not present" otherwise; step 0 needs none).  Exceptions as rotateRows
std::vector<ciphertext3D> rotateRowsMany(const ciphertext3D &t, const std::vector<int> &steps, int out_form = CRC_COEFF);
// y = W x over the slots of ONE image per ciphertext, by the diagonal method: y = Sum_d diag_d (.) rotateRows(x, d) over the non-zero diagonals of W, each
// rotation hoisted and the products fused with it (crc_diag_mac_forms).  W: out x in integers mod t (any int64 is taken mod t), out, in <= M, zero-padded to
// M x M; M a power of two <= n/2.
// INPUT CONTRACT: the vector x (in <= M entries, zero-padded to M) must be TILED WITH PERIOD M over all n slots of every ciphertext -- slot i holds x[i mod M]
// in both rows of n/2 slots -- so that a row rotation is a rotation mod M.  The result is tiled the same way: slot i holds (W x)[i mod M], zero beyond `out`.
// The keys of 3^d for every non-zero diagonal d >= 1 must be in the set (generateGaloisKeys(dbc, elements)).  A host function, not a layer kind: a slot-batched
// network keeps one IMAGE per slot, this keeps one VECTOR ENTRY per slot -- the low-latency counterpart for a single image.
// std::logic_error when the parameters do not support batching, std::invalid_argument for a bad M or shape, other forms, a missing key
ciphertext3D matvecSlots(const ciphertext3D &t, const std::vector<std::vector<int64_t>> &W, int M, int out_form = CRC_COEFF);
// the plan matvecSlots follows: the steps of W's non-zero diagonals and their slot rows [steps][n], rows[r][i] = W[i mod M][(i mod M + steps[r]) mod M]
void diagMatvecPlan(const std::vector<std::vector<int64_t>> &W, int M, int n, std::vector<int> &steps, std::vector<int64_t> &rows);
// The same product by baby steps and giant steps (include/crcnn_hip.h: crc_diag_mac_bsgs_forms): the diagonal d = B j + b is a giant rotation by B j of a product
// with a baby rotation by b, so a dense W takes B + M/B - 2 key switches and keys where matvecSlots takes M - 1 -- the keys of crc_bsgs_elements(M, B, n)
// (crcnn_amd/host/diag_plan.h) are what generateGaloisKeys(dbc, elements) must hold.  B: a power of two, 1 <= B <= M; 0: bsgsDefaultSplit(M), the power of two
// B >= M/B nearest the square root.  Input contract, result, forms and exceptions as matvecSlots (plus a bad B); a ciphertext of its own definition, not
// matvecSlots' bits, with one more key switch and a sum of M/B terms in its noise.  B = M is matvecSlots' product
ciphertext3D matvecSlotsBsgs(const ciphertext3D &t, const std::vector<std::vector<int64_t>> &W, int M, int B = 0, int out_form = CRC_COEFF);
int bsgsDefaultSplit(int M);
// the plan it follows (crc_bsgs_plan): rows [giant][baby][n], rows[j][b][i] = W[(i - giant_steps[j]) mod M][(i + baby_steps[b]) mod M]
void bsgsMatvecPlan(const std::vector<std::vector<int64_t>> &W, int M, int n, int B, std::vector<int> &baby_steps, std::vector<int> &giant_steps,
                    std::vector<int64_t> &rows);

// A convolution over the slots of ONE image, one channel plane per ciphertext (include/crcnn_hip.h: crc_conv_slots_forms; the plan: crc_conv_slots_plan in
// crcnn_amd/host/diag_plan.h).  SlotPlanes says where a tensor [1][zd][1][1] keeps its planes: pixel (r, c) of an H x W plane at slot dil (r pitch + c), tiled with
// period M over both rows of n/2 slots (matvecSlots' input contract); fh, fw, pool describe the layer applied to it -- a 'valid' fh x fw convolution of stride 1,
// then a pool x pool sum pool of stride pool, folded into the taps.  Slots that hold no valid pixel hold junk: no masks, no zero padding.
// The appended fields are the general layer (crc_conv_slots_plan_geom): the plane begins at slot `origin`, the window has `pad` zero pixels on every side and
// moves with `stride`, the pool's windows with pool_stride (0: pool).  pad > 0 needs a CLEAN tensor -- every slot of a period that holds no pixel exactly 0 -- which
// encryptImagePlanes with a margin, a masked convSlots and densePlanes give.
struct SlotPlanes { int M = 0, pitch = 0, H = 0, W = 0, dil = 1, fh = 1, fw = 1, pool = 1, origin = 0, stride = 1, pad = 0, pool_stride = 0; };
// pixels [zd][xd][yd] (integers as they are; floats quantised as encryptImageSlots quantises) -> a tensor [1][zd][1][1] of zd ciphertexts, plane z with its xd rows
// of yd pixels at pitch yd, dilation 1, period M.  Keystream discipline as encryptImage.  std::logic_error unless setSlotEncoding is on; std::invalid_argument
// for M not a power of two <= n/2 or a plane that does not fit it.  planesOf: the SlotPlanes of such a tensor
ciphertext3D encryptImagePlanes(const std::vector<int64_t> &pixels, int zd, int xd, int yd, int M, int out_form = CRC_COEFF);
ciphertext3D encryptImagePlanes(const std::vector<float> &pixels, int zd, int xd, int yd, int M, int out_form = CRC_COEFF);
SlotPlanes planesOf(int xd, int yd, int M);
// the same with `margin` empty slots around the plane: pitch yd + margin, origin margin (pitch + 1), zeros everywhere else -- a clean tensor whose first layer may
// have a pad of up to `margin`.  std::invalid_argument also for a negative margin or a plane that no longer fits M
ciphertext3D encryptImagePlanes(const std::vector<int64_t> &pixels, int zd, int xd, int yd, int M, int margin, int out_form);
ciphertext3D encryptImagePlanes(const std::vector<float> &pixels, int zd, int xd, int yd, int M, int margin, int out_form);
SlotPlanes planesOf(int xd, int yd, int M, int margin);
// the H x W valid pixels of every plane of the tensor, from the first period, as centred integers [zd][H W]
std::vector<std::vector<int64_t>> decryptPlanes(const ciphertext3D &t, const SlotPlanes &g);
// y[co] = Sum_ci conv(x[ci], weights[co][ci]) (+ pool) over the global Galois keys: plans (crc_conv_slots_plan), folds and packs the weights
// [Cout][Cin = t.zd][fh][fw] (any int64, taken mod t), calls crc_conv_slots_forms.  Returns the Cout ciphertexts [1][Cout][1][1] and sets *out to where their valid
// pixels are (fh = fw = pool = 1: ready for the next layer's window).  The keys of convSlotsElements(g) must be in the set (generateGaloisKeys(dbc, elements)).
// Exceptions as matvecSlots: std::logic_error without batching, std::invalid_argument for a geometry the planner refuses, a weight count that is not
// Cout t.zd fh fw, other forms, a missing key
ciphertext3D convSlots(const ciphertext3D &t, const std::vector<int64_t> &weights, int Cout, const SlotPlanes &g, SlotPlanes *out = nullptr, int out_form = CRC_COEFF);
// The same with a bias [Cout] (any int64, taken mod t; empty: none) added to every slot and, with mask = true, every slot that holds no output set to exactly 0:
// crc_conv_slots_bias_mask_forms, both inside the channel mix's epilogue.  The mask row is composed and transformed once per call.  A masked result is clean: the
// next layer may have a pad, as far as the margin around the plane reaches.  std::invalid_argument also for a bias whose size is neither 0 nor Cout
ciphertext3D convSlots(const ciphertext3D &t, const std::vector<int64_t> &weights, int Cout, const SlotPlanes &g, const std::vector<int64_t> &bias, bool mask,
                       SlotPlanes *out = nullptr, int out_form = CRC_COEFF);
// the Galois elements of the layer's taps without the element 1, each once (at most T - 1 keys; a tap left of or above the anchor is a right rotation);
// std::invalid_argument as convSlots
std::vector<uint64_t> convSlotsElements(const SlotPlanes &g);
// The dense layer behind the last packed convolution (crc_dense_planes_forms): t [1][Cin][1][1] holds Cin planes whose valid entries sit at in_slots [P] of every
// period M (the H x W pixels of a SlotPlanes: densePlanesInSlots; every other slot may hold junk), W [O][Cin][P] are integer weights (any int64, taken mod t).  The
// result [1][1][1][1] holds Sum_c Sum_p W[o][c][p] x_c[in_slots[p]] at slot out_slots[o] of every period (default: o) and exactly 0 at every other slot -- a clean
// vector, so the same call at Cin = 1 with in_slots = the previous out_slots is the next dense layer.  The OUTPUTS are rotated: one key switch per distinct value
// of (in_slots[p] - out_slots[o]) mod M whatever Cin is, so the choice of out_slots decides the cost (crcnn_amd/host/diag_plan.h).  The keys of
// densePlanesElements must be in the set (generateGaloisKeys(dbc, elements)); the prepared form of a key is made when a layer first uses it and kept until the keys
// change -- the buffer has a slot for every key of the set (preparedGaloisKeyBytes), the keys of other layers are never prepared.  Exceptions as matvecSlots: std::logic_error without batching, std::invalid_argument for lists the planner refuses, a weight count that
// is not O Cin P, a tensor that is not [1][zd][1][1], a missing key ("galois key not present") or a form other than CRC_COEFF / CRC_NTT.
ciphertext3D densePlanes(const ciphertext3D &t, const std::vector<int64_t> &W, int O, const SlotPlanes &g, const std::vector<int> &out_slots = {}, int out_form = CRC_COEFF);
ciphertext3D densePlanes(const ciphertext3D &t, const std::vector<int64_t> &W, int O, int M, const std::vector<int> &in_slots, const std::vector<int> &out_slots = {},
                         int out_form = CRC_COEFF);
std::vector<int> densePlanesInSlots(const SlotPlanes &g);
// the Galois elements of the layer's steps without the element 1, each once; std::invalid_argument as densePlanes
std::vector<uint64_t> densePlanesElements(const SlotPlanes &g, int O, const std::vector<int> &out_slots = {});
std::vector<uint64_t> densePlanesElements(int M, const std::vector<int> &in_slots, int O, const std::vector<int> &out_slots = {});
size_t preparedGaloisKeyBytes();
// the integers at out_slots of every ciphertext of t: [count][out_slots.size()]
std::vector<std::vector<int64_t>> decryptVector(const ciphertext3D &t, const std::vector<int> &out_slots);

// ---- layers (CrCNN/src/layer.h:10-31) ------------------------------------------------------------------------------
class Layer {
public:
    std::string name;
    int out_form = CRC_COEFF;                               // CRC_NTT keeps the output NTT-resident (set by Network::forward)
    Layer() {}
    Layer(std::string layer_name) : name(layer_name) {}
    virtual ~Layer() {}
    std::string getName() { return name; }
    virtual void printLayerStructure() = 0;
    virtual ciphertext3D forward(ciphertext3D input) = 0;
    virtual void savePlaintextParameters(std::ostream *outfile) = 0;
    virtual void loadPlaintextParameters(std::istream *infile) = 0;
    void computeBoundaries(int xd, int yd, int xs, int ys, int xf, int yf, int *xl, int *yl);   // layer.cpp:12-26
    // device-resident encoded parameters of this layer, in a fixed order (Network::broadcastParameters).  allocate_only: a receiving
    // rank sizes the buffers without encoding anything; otherwise the plaintext parameters are lifted + NTT'd into them first.
    virtual void deviceParameters(std::vector<std::shared_ptr<DeviceBuffer>> &out, bool allocate_only) { (void)out; (void)allocate_only; }
    // where this layer keeps its weights: 0 resident in NTT form, 1 streamed (coefficient-form plaintexts, transformed tile by tile inside every forward),
    // 2 tile-wise limb weights (no canonical copy is ever made).  Decided from the memory the rank has; Network::broadcastParameters makes every rank adopt the
    // root's decision, because the buffers on the wire are sized by it
    virtual int placement() { return 0; }
    virtual void adoptPlacement(int p) { (void)p; }
    // reporting (bench_host): bytes this layer holds in HBM right now (parameters in whatever operand form they are in, streaming tiles), and the
    // multiply-accumulate kernel a conv / dense layer runs on ("" for the others)
    virtual size_t deviceBytes() const { return 0; }
    virtual std::string kernelName() const { return ""; }
};

class BatchNormLayer;
struct BnFold;
// What a convolutional and a fully connected layer share: the multiply-accumulate layer y[f] = sum_t x[t] (*) w[f][t] + Delta b[f] over a geometry
// (zd, xd, yd, xs, ys, xf, yf, nf) -- a dense layer is the 1x1 convolution (in_dim, 1, 1, 1, 1, 1, 1, out_dim), as everywhere below the host -- with ONE copy
// of the weights' device state, of their placement and operand forms, and of the forward call.  The two classes add the reference's constructors, fields and
// plaintext containers.  The geometry is fixed at construction
class MacLayer : public Layer {
public:
    friend class Network;
    const int zd, xd, yd, xs, ys, xf, yf, nf;
    void deviceParameters(std::vector<std::shared_ptr<DeviceBuffer>> &out, bool allocate_only) override;
    int placement() override;
    void adoptPlacement(int p) override { forced_placement = p; }
    // weights back to canonical NTT form (unpacked; rebuilt from the plaintexts when the matrix-core form replaced them)
    void restoreCanonical();
    size_t deviceBytes() const override;
    std::string kernelName() const override;
    // the box the layer carries at this moment (1 x 1: none -- never taken, or given back by unbox())
    void boxSize(int &bx, int &by) const { bx = bxf; by = byf; }
protected:
    MacLayer(std::string name, bool dense, int zd, int xd, int yd, int xs, int ys, int xf, int yf, int nf)
        : Layer(name), zd(zd), xd(xd), yd(yd), xs(xs), ys(ys), xf(xf), yf(yf), nf(nf), dense(dense), slot_weights(slotEncoding()) {}
    // the layer on an input the caller has checked; the output tensor is [B][zo][xo][yo]
    ciphertext3D run(const ciphertext3D &input, int zo, int xo, int yo);
private:
    // what the shared code asks of the class's plaintext containers: the reference's "weights are on the device" flag, whether the containers are filled (a
    // layer Network::fuse() made has none), and the plaintexts of output rows [f0, f0 + fn) in the order the kernels read them, [f][zd][xf][yf], with the
    // biases of those rows when b is given (std::invalid_argument when the containers do not have the layer's shape)
    virtual bool &alreadyNtt() = 0;
    virtual bool hasPlaintexts() const = 0;
    virtual void plaintexts(int f0, int fn, std::vector<const Plaintext *> &w, std::vector<const Plaintext *> *b) const = 0;
    const bool dense;                                       // decides the two one-sided features below, and the class name in error texts
    const char *kind() const { return dense ? "FullyConnectedLayer" : "ConvolutionalLayer"; }
    // CONVOLUTIONS ONLY (Network::fuse() step 1a, crc_plan_conv1_box): a one-channel layer whose xf x yf window is a base window convolved with a bxf x byf sum at
    // the layer's stride keeps the BASE window's weights and has the image pack sum its input instead (crc_conv2d_box_forms).  The layer still reports the
    // geometry of the map it computes; unbox() goes back to the enlarged window's weights where the layer cannot run on the one-channel matrix-core kernel
    int bxf = 1, byf = 1;
    bool boxed() const { return bxf * byf > 1; }
    int wxf() const { return xf - (bxf - 1) * xs; }         // the window the weights are stored for
    int wyf() const { return yf - (byf - 1) * ys; }
    void unbox();
    size_t taps() const { return (size_t)zd * wxf() * wyf(); }    // weights per output row
    std::shared_ptr<DeviceBuffer> d_w, d_b[2];              // NTT-form weights, bias delta in coefficient / NTT form
    // weights whose NTT form (k rows each) would take more than 75 % of HBM stay coefficient-form plaintexts (ONE row each) and are lifted + transformed a
    // ~2-GiB filter tile at a time inside every forward (SURVEY section 7's fall-back; PlainModelWoPad's fc3 with all eight primes of n = 16384 is 419 GB)
    bool streamed = false;
    int stream_form = CRC_NTT;                              // operand form of the last streamed forward (CRC_NTTL: 64-filter limb tiles on the matrix cores)
    std::shared_ptr<DeviceBuffer> d_plain, d_wtile, d_ytile;
    // CRC_NTTP / CRC_NTTL / CRC_NTTL1 / CRC_NTTLS once Network::forward has put the weights into their MAC kernel's operand form
    int w_form = CRC_NTT;
    // built under setSlotEncoding: the weights are constant polynomials and the layer asks crc_plan_mac_scalar (the scalar form CRC_NTTLS, one GEMM per modulus
    // over all slots).  Cleared for good when crc_scalar_pack_weights finds a row that is not constant: the layer then keeps the row path
    bool slot_weights;
    // CONVOLUTIONS ONLY: the one-channel matrix-core form CRC_NTTL1 (limbWeights), and with it the canonical NTT-form weights it keeps beside the limb copy
    std::shared_ptr<DeviceBuffer> d_w_canon;
    // DENSE LAYERS ONLY (upload): a layer whose canonical NTT-form weights and their limb copy do not fit in HBM together (PlainModelWoPad's fc3 at n = 16384,
    // k = 4: 202 + 182 GiB) never gets a canonical copy: its limb weights are built a tile of output rows at a time straight from the plaintexts (lift + NTT ->
    // batch-norm fold of the tile -> pack), a batch-norm layer that Network::fuse() folds into it being applied to every tile (same ciphertexts; netrun.py
    // does the same)
    bool tilewise = false, tile_built = false;
    std::shared_ptr<BatchNormLayer> fold_bn;
    int last_B = 0;                                         // images of the last forward (kernelName: one image through a dense layer runs as a weight stream)
    int forced_placement = -1;
    bool forcedTilewise() const { return dense && forced_placement == 2; }
    int plannedForm(int B) const;                           // the kernel crc_plan_mac picks for a launch on B images
    bool limbFits() const;
    void upload();
    void buildTilewise();
    void packWeights(bool unpack);
    // -> CRC_NTTL / CRC_NTTL1 (matrix-core kernels) when the layer qualifies (for batches of B) and HBM has room for the second copy
    bool limbWeights(int B);
    bool streamsOnMatrixCores(int B);                       // streamed, and a launch on B images takes the limb GEMM (forwardStreamed's 64-filter limb tiles)
    int forwardStreamed(const ciphertext3D &input, ciphertext3D &out);
    std::vector<uint64_t> hostBias();                       // the NTT-form bias rows [nf][k][n]
    void setBias(const std::vector<uint64_t> &ntt_rows);    // ... replaced, with their coefficient-form twin
};

class ConvolutionalLayer : public MacLayer {                // convolutionalLayer.h:33-34
public:
    int th_count;
    int xo, yo, zo;
    plaintext4D filters;                                    // nf,zd,xf,yf
    std::vector<Plaintext> biases;
    bool filters_already_ntt = false;
    ConvolutionalLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count, plaintext4D &filters,
        std::vector<Plaintext> &biases);
    ConvolutionalLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count, std::istream *infile);
    ciphertext3D forward(ciphertext3D input) override;
    plaintext3D getKernel(int kernel_index) { return filters[kernel_index]; }
    Plaintext getBias(int bias_index) { return biases[bias_index]; }
    void savePlaintextParameters(std::ostream *outfile) override;
    void loadPlaintextParameters(std::istream *infile) override;
    void printLayerStructure() override;
private:
    bool &alreadyNtt() override { return filters_already_ntt; }
    bool hasPlaintexts() const override { return (int)filters.size() == nf; }
    void plaintexts(int f0, int fn, std::vector<const Plaintext *> &w, std::vector<const Plaintext *> *b) const override;
};

class FullyConnectedLayer : public MacLayer {               // fullyConnectedLayer.h:22-24
public:
    int in_dim, out_dim, th_count;
    plaintext2D weights;
    std::vector<Plaintext> biases;
    bool weights_already_ntt = false;
    FullyConnectedLayer(std::string name, int in_dim, int out_dim, int th_count, plaintext2D &weights, std::vector<Plaintext> &biases);
    FullyConnectedLayer(std::string name, int in_dim, int out_dim, int th_count, std::istream *infile);
    ciphertext3D forward(ciphertext3D input) override;
    Plaintext getWeight(int x_index, int y_index) { return weights[x_index][y_index]; }
    Plaintext getBias(int x_index) { return biases[x_index]; }
    void savePlaintextParameters(std::ostream *outfile) override;
    void loadPlaintextParameters(std::istream *infile) override;
    void printLayerStructure() override;
private:
    bool &alreadyNtt() override { return weights_already_ntt; }
    bool hasPlaintexts() const override { return (int)weights.size() == out_dim; }
    void plaintexts(int f0, int fn, std::vector<const Plaintext *> &w, std::vector<const Plaintext *> *b) const override;
};

class PoolingLayer : public Layer {                         // poolingLayer.h:15
public:
    friend class Network;
    int xd, yd, zd, xs, ys, xf, yf, xo, yo, zo;
    PoolingLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf);
    ciphertext3D forward(ciphertext3D input) override;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    void printLayerStructure() override;
protected:
    std::shared_ptr<DeviceBuffer> d_div;                    // NTT-form divisor (AvgPoolingLayer only)
public:
    size_t deviceBytes() const override { return d_div ? d_div->bytes : 0; }
};

class AvgPoolingLayer : public PoolingLayer {               // avgPoolingLayer.h:11
public:
    Plaintext div_factor;
    AvgPoolingLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf);
};

// Zero padding of the two spatial dimensions (no layer of the reference, whose convolution is valid-only): px all-zero ciphertexts on both sides of the
// first dimension, py on both sides of the second (crc_pad).  The all-zero ciphertext is BFV's additive identity in either form, so the layer keeps its
// input's form, like PoolingLayer, and takes canonical CRC_COEFF or CRC_NTT rows only: Network::forward plans the layer in front of it as it plans the layer
// in front of a pooling layer, and no packed or limb hand-over spans it.  Nothing to save or load
class PaddingLayer : public Layer {
public:
    int xd, yd, zd, px, py, xo, yo, zo;
    PaddingLayer(std::string name, int xd, int yd, int zd, int px, int py);
    ciphertext3D forward(ciphertext3D input) override;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    void printLayerStructure() override;
};

// `rescale NAME BITS` of a slot-batched network: in front of the next layer the client re-encodes every slot to the scale 2^BITS -- decrypt, every slot divided
// by `divisor` = sigma / 2^BITS and rounded to nearest, encrypt (rescaleSlots).  Takes CRC_COEFF / CRC_NTT and writes out_form CRC_COEFF / CRC_NTT
// (std::invalid_argument otherwise); no plaintext parameters.  The divisor is set by CnnBuilder::buildNetworkFromDescription from the scale ledger
class SlotRescaleLayer : public Layer {
public:
    int bits;
    uint64_t divisor = 1;
    bool symmetric = false;                                 // re-encrypt under the secret key (crc_slots_refresh_sym_dev)
    SlotRescaleLayer(std::string name, int bits) : Layer(name), bits(bits) {}
    ciphertext3D forward(ciphertext3D input) override;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    void printLayerStructure() override;
};

// `client_relu NAME BITS [cap C]` and `client_maxpool NAME stride XS YS window XF YF bits BITS [relu] [cap C]` of a slot-batched network: where the client
// re-encodes every slot to the scale 2^BITS it also applies max(x, 0) and / or takes the maximum over a window of ciphertexts, slot by slot (actSlots).  Forms,
// divisor and `symmetric` as SlotRescaleLayer; `cap` is in slot units of the scale behind the layer (0: none), set by the builder from C.  Network::fuse pairs
// neither with anything
class SlotReluLayer : public Layer {
public:
    int bits;
    float cap_value;                                        // C of the description (0: no cap)
    uint64_t divisor = 1, cap = 0;
    bool symmetric = false;
    SlotReluLayer(std::string name, int bits, float cap_value = 0.0f) : Layer(name), bits(bits), cap_value(cap_value) {}
    ciphertext3D forward(ciphertext3D input) override;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    void printLayerStructure() override;
};
class SlotMaxPoolLayer : public Layer {
public:
    int xs, ys, xf, yf, bits;
    bool relu;
    float cap_value;
    uint64_t divisor = 1, cap = 0;
    bool symmetric = false;
    SlotMaxPoolLayer(std::string name, int xs, int ys, int xf, int yf, int bits, bool relu = false, float cap_value = 0.0f)
        : Layer(name), xs(xs), ys(ys), xf(xf), yf(yf), bits(bits), relu(relu), cap_value(cap_value) {}
    ciphertext3D forward(ciphertext3D input) override;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    void printLayerStructure() override;
};

// What the five activation layers share, as MacLayer does for conv / dense: the pooling window Network::fuse() may put behind the activation (a flat layer has
// none: the fields are 0, any input shape goes in and comes out) with the pooling's divisor, the NTT-form coefficient rows with their upload at the first forward,
// and what every forward starts with.  The classes add their constructor, their one C-ABI call and printLayerStructure.  Nothing to save or load
class ActivationLayer : public Layer {
public:
    int xd = 0, yd = 0, zd = 0, xs = 0, ys = 0, xf = 0, yf = 0, xo = 0, yo = 0, zo = 0, th_count;
    void savePlaintextParameters(std::ostream *) override {}
    void loadPlaintextParameters(std::istream *) override {}
    size_t deviceBytes() const override;
protected:
    ActivationLayer(std::string name, const char *kind, int th_count) : Layer(name), th_count(th_count), kind(kind) {}
    ActivationLayer(std::string name, const char *kind, int th_count, int xd, int yd, int zd, int xs, int ys, int xf, int yf, std::shared_ptr<DeviceBuffer> d_div);
    bool pooled() const { return xf > 0; }
    // Every forward's start: std::invalid_argument for an empty input (a pooled layer: any shape but its own), without evaluation keys and for an out_form other
    // than CRC_COEFF / CRC_NTT; the rows uploaded at the first call.  Returns the output tensor, in `form`.  scratch: the shared work area, `bytes` at least
    ciphertext3D begin(const ciphertext3D &input, int form);
    void *scratch(size_t bytes) const;
    void poly2Rows(float c2, float c1, float c0, const double *scales);
    const char *const kind;                                 // the class's name, for error texts
    std::shared_ptr<DeviceBuffer> d_div;                    // NTT-form divisor of an average pooling
    std::shared_ptr<DeviceBuffer> d_p[4];                   // the rows, highest power first; empty = 1 for the first, 0 for the others
private:
    virtual void rows() {}                                  // fills d_p (once)
    bool uploaded = false;
};

class SquareLayer : public ActivationLayer {                // squareLayer.h:12
public:
    SquareLayer(std::string name, int th_count) : ActivationLayer(name, "SquareLayer", th_count) {}
    ciphertext3D forward(ciphertext3D input) override;
    void printLayerStructure() override;
};

// Network::fuse(): a SquareLayer with a (sum or average) PoolingLayer behind it.  Relinearisation is linear in the digit polynomials of c2, so the digits of a
// pooling window are added and ONE key switch serves the pooled ciphertext (crc_square_pool_relin_forms): the ciphertexts squareLayer.cpp:21-39 followed by
// poolingLayer.cpp:22-44 produce, bit for bit, with xo yo / (xd yd) of the key-switching work.  The divisor is applied to the pooled ciphertexts
class SquarePoolLayer : public ActivationLayer {
public:
    SquarePoolLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int th_count, std::shared_ptr<DeviceBuffer> d_div)
        : ActivationLayer(name, "SquarePoolLayer", th_count, xd, yd, zd, xs, ys, xf, yf, d_div) {}
    ciphertext3D forward(ciphertext3D input) override;
    void printLayerStructure() override;
};

// Degree-2 polynomial activation c2 x^2 + c1 x + c0 (no layer of the reference, whose one non-linearity is SquareLayer): per ciphertext the Evaluator sequence
//     s = relinearize(square(x), ev_keys16); s = multiply_plain(s, encode(c2)); s = add(s, multiply_plain(x, encode(c1))); s = add_plain(s, encode(c0))
// (a step is left out for c2 == 1, c1 == 0, c0 == 0), computed with one key switch per ciphertext (crc_poly2_relin_forms).  The coefficients are float32
// and encoded as the weights are; c2 == 0 (a batch norm, not an activation) and non-finite values are std::invalid_argument.  PolyLayer(name, 1, 0, 0, ...)
// produces SquareLayer's ciphertexts bit for bit.  Rows: encode(c2), encode(c1), Delta encode(c0)
class PolyLayer : public ActivationLayer {
public:
    float c2, c1, c0;
    // slot encoding: the scales of c2, c1, c0 (the rows are the constants nearbyint(c * scale) mod t); 0 = the fractional encoder.  Set before the first forward
    double slot_scale[3] = {0, 0, 0};
    PolyLayer(std::string name, float c2, float c1, float c0, int th_count);
    ciphertext3D forward(ciphertext3D input) override;
    void printLayerStructure() override;
private:
    void rows() override { poly2Rows(c2, c1, c0, slot_scale); }
};

// Degree-3 polynomial activation c3 x^3 + c2 x^2 + c1 x + c0: per ciphertext the Evaluator sequence
//     s = relinearize(square(x), ev_keys16); u = relinearize(multiply(s, x), ev_keys16); r = multiply_plain(u, encode(c3));
//     r = add(r, multiply_plain(s, encode(c2))); r = add(r, multiply_plain(x, encode(c1))); r = add_plain(r, encode(c0))
// (a step is left out for c3 == 1, c2 == 0, c1 == 0, c0 == 0), computed by crc_poly3_relin_forms: TWO key switches and a multiplicative depth of 2 -- the
// parameters must leave noise budget for a second multiplication (CrCNN's published (4096, two moduli, t = 2^29) leave none).  c3 == 0 (a PolyLayer) and
// non-finite values are std::invalid_argument.  Network::fuse() treats the layer as an unfused SquareLayer: nothing is paired with a pooling behind it.
// Rows: encode(c3), encode(c2), encode(c1), Delta encode(c0)
class Poly3Layer : public ActivationLayer {
public:
    float c3, c2, c1, c0;
    double slot_scale[4] = {0, 0, 0, 0};                    // of c3, c2, c1, c0, as PolyLayer's
    Poly3Layer(std::string name, float c3, float c2, float c1, float c0, int th_count);
    ciphertext3D forward(ciphertext3D input) override;
    void printLayerStructure() override;
private:
    void rows() override;
};
// relinearize(multiply(a, b), ev_keys16) elementwise on two tensors of equal shape and form (CRC_COEFF or CRC_NTT), the result in out_form
// (crc_multiply_relin_forms: Evaluator::multiply of SEAL 2.3.1, bit for bit); std::invalid_argument otherwise
ciphertext3D multiplyRelin(const ciphertext3D &a, const ciphertext3D &b, int out_form = CRC_COEFF);

// Network::fuse(): a PolyLayer with a (sum or average) PoolingLayer behind it, as SquarePoolLayer pairs a SquareLayer:
//     Sum_w (c2 x_w^2 + c1 x_w + c0) = c2 Sum_w relin(x_w^2) + c1 Sum_w x_w + W c0
// keeps ONE key switch per pooled ciphertext (crc_poly2_pool_relin_forms); the window count and an average pooling's divisor are folded into the three
// rows once (exact ring arithmetic).  Same ciphertexts as the two layers one after the other
class PolyPoolLayer : public ActivationLayer {
public:
    float c2, c1, c0;
    double slot_scale[3] = {0, 0, 0};                       // as PolyLayer's (Network::fuse() copies them)
    PolyPoolLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int th_count, float c2, float c1, float c0,
        std::shared_ptr<DeviceBuffer> d_div);
    ciphertext3D forward(ciphertext3D input) override;
    void printLayerStructure() override;
private:
    void rows() override { poly2Rows(c2, c1, c0, slot_scale); }
};

class BatchNormLayer : public Layer {                       // batchNormLayer.h:18-20
public:
    friend class Network;
    friend struct BnFold;
    int num_channels;
    std::vector<Plaintext> mean, var;                       // var already holds encode(1/sqrt(var+1e-5)) (cnnBuilder.cpp:100-102)
    BatchNormLayer(std::string name, int num_channels, std::vector<Plaintext> &mean, std::vector<Plaintext> &var);
    BatchNormLayer(std::string name, int num_channels, std::istream *infile);
    ciphertext3D forward(ciphertext3D input) override;
    Plaintext getMean(int index) { return mean[index]; }
    Plaintext getVar(int index) { return var[index]; }
    void savePlaintextParameters(std::ostream *outfile) override;
    void loadPlaintextParameters(std::istream *infile) override;
    void printLayerStructure() override;
private:
    std::shared_ptr<DeviceBuffer> d_mean[2], d_invstd;
public:
    size_t deviceBytes() const override { return (d_mean[0] ? d_mean[0]->bytes : 0) + (d_mean[1] ? d_mean[1]->bytes : 0) + (d_invstd ? d_invstd->bytes : 0); }
private:
    void upload();
public:
    void deviceParameters(std::vector<std::shared_ptr<DeviceBuffer>> &out, bool allocate_only) override;
};

// ---- network (CrCNN/src/network.h:11-39) ---------------------------------------------------------------------------
class OutOfBudgetException : public std::exception {
public:
    const int last_layer_computed;
    std::string msg;
    OutOfBudgetException(int last_layer_computed) : last_layer_computed(last_layer_computed), msg("OutOfBudgetException at layer " +
        std::to_string(last_layer_computed)) {}
    const char *what() const throw() override { return msg.c_str(); }
};

class Network {
public:
    std::vector<std::shared_ptr<Layer>> layers;
    // shape of one input image, [zd][xd][yd]: what the description the network was built from says (CrCNN's three models: 1 x 28 x 28)
    int input_zd = 1, input_xd = 28, input_yd = 28;
    // the layer list as a description (NetworkDescription, INTEGRATION.md "Network descriptions") that CnnBuilder::buildNetworkFromDescription builds back
    // into this network, refresh point included.  It describes the layers as built: std::logic_error once fuse() has folded some
    std::string describe() const;
    // network.cpp:23 hard-codes a client-side decrypt/re-encrypt "refresh" before layer 6; it needs the secret key and is off
    // the accelerated path, so it is a setting here: 6 reproduces the committed reference, -1 (default) never refreshes.
    int layer_before_reenc = -1;
    // true: every refresh of forward() -- the fixed refresh point and the budget-checking forward's -- re-encrypts under the secret key
    // (refreshImages(..., symmetric = true)).  Off by default: the reference's refresh calls Encryptor::encrypt
    bool reenc_symmetric = false;
    bool ntt_resident = true;                               // keep tensors in NTT form between linear layers (bit-identical)
    // conv / dense layers with long reductions (>= 8 steps of 32 channels) run as an int8 limb GEMM on the matrix cores (CRC_NTTL, kernels_mfma.hip):
    // exact integer arithmetic, identical ciphertexts, about 4x the vector-ALU kernel.  The conversion of a layer's weights drops their canonical copy:
    // broadcastParameters() must come before the first forward(); fuse() may follow one (it rebuilds the canonical weights from the plaintexts).
    bool matrix_cores = true;
    // >= 0 selects the budget-checking forward the reference keeps for its parameter search (network.cpp:52-96): after every layer the
    // noise budget of output[0][0][0] is measured (secret key, coefficient form at every boundary); at <= 5 bits the layer's input is
    // refreshed and the layer repeated while refreshes are left, then OutOfBudgetException(i - 1) is thrown.  -1: plain forward.
    int max_num_of_reencryptions = -1;
    // what the budget-checking forward looks at.  0: noiseBudget(output), ciphertext 0 of image 0, every boundary in coefficient form (the reference ran one
    // image at a time, so that WAS its whole check).  1: minNoiseBudget of the whole output tensor, every image of the batch, measured on the device in whatever
    // ciphertext form the layer wrote -- the layers keep CRC_NTT output between linear layers when ntt_resident is set (the packed and limb hand-overs stay
    // off, as in scope 0).  The output ciphertexts are the same bits in both scopes as long as no refresh is triggered.
    int budget_scope = 0;
    // true: every forward (plain or budget-checking) measures the output tensor of every layer on the device and fills last_layer_budget_min (smallest budget
    // of the tensor; over all chunks under two-level chunking) and last_layer_budget_first (ciphertext 0 of image 0: what noiseBudget(output) gives), one entry
    // per layer, -1 where the output is in a packed or limb form and cannot be measured (ntt_resident with matrix_cores; switch them off for a full profile).
    // Costs one stream synchronisation per layer call.
    bool profile_budget = false;
    // non-zero: forward() floods its OUTPUT tensor with this width before it returns (floodImages: the response carries no trace of the weights in its noise;
    // floodBits(a-priori budget) chooses it).  0 (default): off, and not one launch differs.  std::invalid_argument for a width the parameters refuse, before
    // the first launch; for an output in a packed or limb form (which only the last layer decides), after it.  The caller's own tensor is never written: an
    // output that shares the input's buffer is copied first
    int flood_bits = 0;
    std::vector<int> last_layer_budget_min, last_layer_budget_first;
    std::vector<double> last_layer_ms;                      // per-layer wall milliseconds of the last forward (T_LAYER_i, mainparams.cpp:81)
    // true: last_layer_ms comes from HIP events recorded on the launch stream around every layer call -- no synchronisation between the layers, what a
    // throughput measurement wants (crcnn_amd/host/bench_host.cpp); false: wall clock around Layer::forward + a stream synchronisation, as the reference's
    // driver measures
    bool time_with_events = false;
    // Layer::forward calls per layer in the last forward (two-level chunking: a head layer runs once per chunk)
    std::vector<int> last_layer_launches;
    double last_reenc_ms = 0.0;
    // true: the floats the client saw at the refresh(es) of the last forward are kept (in the order the refreshes ran: chunk by chunk under two-level
    // chunking); costs a stream synchronisation per refresh
    bool keep_reenc_values = false;
    std::vector<float> last_reenc_values;
    // Two-level chunking (> 0): the layers in front of the first dense layer run on sub-batches of `head_chunk` images, the dense layers once on the whole
    // batch -- a dense layer streams all of its weights per launch, so its time per image falls with the rows it is used for (PlainModelWoPad at n = 16384:
    // 6-image chunks fit beside 190 GiB of weights, fc3 wants 24+ images).  0: every layer on the whole batch
    int head_chunk = 0;
    // where this rank's HBM goes (bytes): the layers' parameters in their current operand forms, the activation slots forward() keeps, the shared work buffer,
    // the evaluation keys
    struct HbmPlan { size_t parameters = 0, activations = 0, work = 0, keys = 0; };
    HbmPlan hbmPlan() const;
private:
    struct EventPool { std::vector<void *> ev; ~EventPool(); };
    std::shared_ptr<EventPool> event_pool;                  // HIP events of time_with_events, reused from forward to forward (copies of a Network share them)
    // forward() in pieces, as crcnn_amd/netrun.py reads.  ForwardRun (crcnn_host.cpp): the plan of one forward and what it keeps between its layer calls.  plan(B)
    // puts the conv / dense weights into their operand forms, decides the chunking and sets every layer's out_form: boundaryForm, the form behind layer i
    struct ForwardRun;
    ForwardRun plan(int B);
    int boundaryForm(const ForwardRun &f, int i) const;
    // one timed call, booked under layer i (-1: the refresh); a layer's launch is counted and its output budget-profiled behind the timed region
    ciphertext3D timed(ForwardRun &f, int i, const std::function<ciphertext3D()> &call);
    ciphertext3D runLayer(ForwardRun &f, int i, const ciphertext3D &in);
    ciphertext3D runRefresh(ForwardRun &f, const ciphertext3D &in);
    // layers [lo, hi) on t, with the refresh in front of layer_before_reenc (in front of lo: only if refresh_at_lo) and the ping-pong between the activation
    // slots; to_caller: layer hi - 1 is the network's last, its output the caller's own tensor
    ciphertext3D runRange(ForwardRun &f, int lo, int hi, ciphertext3D t, bool to_caller, bool refresh_at_lo);
    ciphertext3D runChunks(ForwardRun &f, const ciphertext3D &input);              // two-level chunking: the sub-batches, assembled
    ciphertext3D runChecked(ForwardRun &f, ciphertext3D input);                    // the budget-checking forward (max_num_of_reencryptions >= 0)
public:
    std::shared_ptr<DeviceBuffer> tail_slot;                // ... and the dense layers' whole-batch input under two-level chunking
    // the two ping-pong activation buffers forward() keeps across calls (sized by the largest layer output so far)
    std::shared_ptr<DeviceBuffer> act_slot[2];
    Network() {}
    ~Network() {}
    int getNumLayers() { return (int)layers.size(); }
    virtual std::shared_ptr<Layer> getLayer(int i) { return layers[i]; }
    std::vector<std::shared_ptr<Layer>> &getLayers() { return layers; }
    void printNetworkStructure();
    ciphertext3D forward(ciphertext3D input);
    // Exact layer folding (ring algebra over Z_q), done once on the device-resident parameters: a sum/avg pooling
    // layer is folded into the convolution in front of it (pooled kernel, xf' = (pxf-1)*cxs + xf, stride cxs*pxs) when that is
    // estimated to be cheaper, a batch-norm layer into the conv / dense layer behind it (w' = w (*) s[channel],
    // b' = b - sum_taps w' (*) mean[channel]).  The network's output ciphertexts stay bit-identical; only the folded layers'
    // intermediate tensors disappear (their plaintext parameters can no longer be saved).  Returns the number of layers removed.
    int fuse();
    // slot encoding: the scale of the network's outputs (decryptSlots' integers are slot_scale() times the numbers the float network computes); 0 for a
    // network built without setSlotEncoding
    double slot_scale() const { return slot_scale_; }
private:
    bool fused_ = false;
    double slot_scale_ = 0;
    friend class CnnBuilder;
public:
    // Multi-GPU start-up (no analogue in the reference): one process (or host thread) per GPU, images sharded across them
    // with no data-path collective.  Rank `root` holds the encoded model -- this call lifts + NTTs its plaintext parameters if that has
    // not happened yet -- and every other rank receives the NTT-form weights / bias / batch-norm rows and the evaluation keys over RCCL
    // (crc_broadcast_weights: ncclBroadcast in <= 1 GiB pieces), without encoding anything.  Every rank then checksums what it holds
    // (crc_checksum64) and the sums are compared with the root's; a mismatch throws std::runtime_error.  Call it before fuse() and
    // before the first forward() on the receiving ranks.  Returns the bytes received per rank.
    // encode_locally = true is SURVEY 8e's alternative: nothing but the evaluation keys is sent, every rank encodes + transforms the weights itself from the
    // model file it read (the 2 MB of floats instead of 35-200 GB of residues on the wire; the same placement agreement and the same checksum comparison).
    size_t broadcastParameters(crc_comm *comm, int root = 0, bool encode_locally = false);
};

// ---- network descriptions ------------------------------------------------------------------------------------------------
// A layer list as text (INTEGRATION.md "Network descriptions"; crcnn_amd/netrun.py parses the same format with the same checks): `#` comments, first
//   input zd xd yd
// then one layer per line, the input shape of each inferred from the line above:
//   conv NAME stride xs ys filter xf yf filters nf      pool | avgpool NAME stride xs ys window xf yf      bn NAME      square NAME
//   fc NAME out_dim      pad NAME px py      refresh (sets layer_before_reenc to the next layer; at most one)
//   poly NAME c2 c1 c0   (c2 x^2 + c1 x + c0: decimal numbers, read as double and rounded to float32; c2 != 0, all finite; written back as %.9g)
//   poly3 NAME c3 c2 c1 c0   (c3 x^3 + c2 x^2 + c1 x + c0, two key switches and depth 2; the same number rules, c3 != 0)
//   rescale NAME BITS   (slot encoding only: the client re-encodes every slot to the scale 2^BITS in front of the next layer, BITS in 0..30; SlotRescaleLayer)
//   client_relu NAME BITS [cap C]   (slot encoding only: as rescale, and the client applies max(x, 0) -- and min(x, C) -- to every slot; SlotReluLayer)
//   client_maxpool NAME stride xs ys window xf yf bits BITS [relu] [cap C]   (slot encoding only: as rescale, on the maximum over the window, slot by slot;
//       changes the shape like pool; SlotMaxPoolLayer).  C: a decimal number as in poly; nearbyint(C 2^BITS) must be in 1..(t - 1) / 2
// conv, fc, square, poly and poly3 lines may end in `threads N` (the th_count the reference's constructors take).  NAME is the HDF5 dataset prefix.
// Every error is a std::invalid_argument whose message starts with "line N:".
struct LayerSpec {
    std::string kind, name;
    int line = 0;
    int zd = 0, xd = 0, yd = 0;                             // the layer's input shape
    int xs = 0, ys = 0, xf = 0, yf = 0, nf = 0;             // conv / pool / avgpool
    int out_dim = 0;                                        // fc (in_dim = zd xd yd, the reference's reshapeInput order)
    int px = 0, py = 0;                                     // pad
    float c2 = 1.0f, c1 = 0.0f, c0 = 0.0f;                  // poly
    float c3 = 1.0f;                                        // poly3 (with c2 c1 c0)
    int bits = 0;                                           // rescale, client_relu, client_maxpool: the scale behind the layer is 2^bits
    bool relu = false, has_cap = false;                     // client_maxpool (client_relu: relu is implied); `cap C` present
    float cap = 0.0f;                                       // C
    int threads = -1;                                       // -1: no `threads` token (the layer is built with th_count 1)
    int zo = 0, xo = 0, yo = 0;                             // output shape
};
struct NetworkDescription {
    int zd = 1, xd = 28, yd = 28;
    int layer_before_reenc = -1;
    int refresh_line = 0;                                   // line of the `refresh` token (0: none)
    std::vector<LayerSpec> layers;
    // h5_path != "": the weight, bias and batch-norm datasets of the model file are checked against the inferred shapes
    static NetworkDescription parse(const std::string &text, const std::string &h5_path = "");
    // text (anything with a line break), the name of a built-in model, or the path of a description file
    static NetworkDescription load(const std::string &text_name_or_path, const std::string &h5_path = "");
    std::string str() const;                                // canonical form: parse(str()) gives the same description
};
// The scale ledger of slot encoding: the scale sigma IN FRONT of every layer of the description, and behind the last one (layers.size() + 1 entries).  sigma
// starts at 2^input_bits; with W = 2^weight_bits
//   conv / fc   weights at scale W, biases at sigma W                               -> sigma W
//   bn          mean at sigma, invstd at W                                          -> sigma W
//   pool, pad   no plaintexts                                                       -> sigma
//   avgpool     none: the layer is built as the sum pool                            -> sigma xf yf
//   square                                                                          -> sigma^2
//   poly        c2 at W, c1 at W sigma, c0 at W sigma^2                             -> sigma^2 W
//   poly3       c3 at W, c2 at W sigma, c1 at W sigma^2, c0 at W sigma^3            -> sigma^3 W
//   rescale     none: every slot divided by sigma / 2^BITS, an integer >= 1         -> 2^BITS
//   client_relu, client_maxpool   as rescale                                        -> 2^BITS
// Every scale must be an integer below 2^62 that a double holds exactly; std::invalid_argument ("line N: ...") otherwise, for a `rescale` whose 2^BITS does not
// divide sigma, and for a `refresh` (the fractional re-encoding of a refresh is not a slot-wise one: `rescale` is).  Needs no context
std::vector<double> slotScales(const NetworkDescription &d, int input_bits, int weight_bits);

// the description of "PlainModelTiny" | "ApproxPlainModel" | "PlainModelWoPad" (crcnn_amd/models/<name>.net, compiled in); nullptr for any other name
const char *builtinDescription(const std::string &model);

// ---- model loader + builder (CrCNN/src/cnnBuilder.h:16-44) ----------------------------------------------------------
class CnnBuilder {
public:
    std::string plain_model_path;
    CnnBuilder(std::string plain_model_path) : plain_model_path(plain_model_path) {}
    ~CnnBuilder() {}
    std::vector<float> getPretrained(std::string var_name);
    ConvolutionalLayer *buildConvolutionalLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf, int nf, int th_count,
        std::istream *infile);
    FullyConnectedLayer *buildFullyConnectedLayer(std::string name, int in_dim, int out_dim, int th_count, std::istream *infile);
    PoolingLayer *buildPoolingLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf);
    AvgPoolingLayer *buildAvgPoolingLayer(std::string name, int xd, int yd, int zd, int xs, int ys, int xf, int yf);
    SquareLayer *buildSquareLayer(std::string name, int th_count);
    PolyLayer *buildPolyLayer(std::string name, float c2, float c1, float c0, int th_count);
    Poly3Layer *buildPoly3Layer(std::string name, float c3, float c2, float c1, float c0, int th_count);
    PaddingLayer *buildPaddingLayer(std::string name, int xd, int yd, int zd, int px, int py);
    BatchNormLayer *buildBatchNormLayer(std::string name, int num_channels, std::istream *infile);
    // cnnBuilder.cpp:108-179 hard-codes one topology per source edit (Tiny is the committed one); all three are available here, and any other as a description
    Network buildNetwork(std::string file_name = "");                  // PlainModelTiny, as committed (cnnBuilder.cpp:157-169)
    // "PlainModelTiny" | "ApproxPlainModel" | "PlainModelWoPad" (built from their compiled-in descriptions), or the path of a description file
    Network buildNetworkByName(const std::string &model, std::string file_name = "");
    // any layer list: description text, a built-in name or the path of a description file (NetworkDescription::load).  The model file's datasets are checked
    // against the inferred shapes before anything is encoded (not when the parameters come from the encoded-model file `file_name`)
    Network buildNetworkFromDescription(const std::string &path_or_text, std::string file_name = "");
    Network buildAndSaveNetwork(std::string file_name);
};
