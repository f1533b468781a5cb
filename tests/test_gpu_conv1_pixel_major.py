"""GPU exactness of the two forms of the one-channel matrix-core convolution (kernels_mfma1.hip), through the public calls only:
  form 1  plane-major limb image, 13 diagonals, 49 MFMAs per tile (mfma_conv1_kernel);
  form 2  pixel-major limb image with the image limb index inside the reduction (weights W'_l = centred(w 256^l mod q)), 7 diagonals, 35 MFMAs per tile, one
          fold (mfma_conv1_kernel_px); windows of at most 40 taps.
Every case runs under conv1_form = 1 and = 2 (the weights are packed anew under each: they follow the form), asserts through limb_conv1_form which form ran, and
compares both outputs bit for bit with each other and with an exact reference in integers.

Reference.  For the shapes with many outputs the exact sum is computed in numpy uint64 without ever overflowing: x = x0 + x1 2^28, w = w0 + w1 2^28 (x0, w0 < 2^28,
x1, w1 < 2^27), so each of the four partial sums over at most 64 taps stays below 2^62; they are joined mod q by multiplications by 2^8 and 2^4 of values below
q < 2^55.  That helper is itself checked against Python integers, term by term, on every small shape; the extreme-digit cases use Python integers only."""
import numpy as np
import pytest

from netcommon import limb_extreme
from test_gpu_mac_bounds import Q54, Q55, balanced_digits, digit_extreme

pytestmark = pytest.mark.gpu

N = 64
Q = [Q55, Q54]

SHAPES = [
    # xd, yd, xs, ys, xf, yf, nf, B  (zd = 1)                                                                              form under conv1_form = 2
    ((28, 28, 2, 2, 6, 6, 32, 2), 2),      # the flagship window: every K group one 16-byte read
    ((9, 11, 1, 2, 3, 5, 5, 2), 2),        # 15 taps: the last group half empty, pairs straddle window rows and start at odd columns (two 8-byte reads)
    ((8, 10, 1, 1, 5, 8, 17, 1), 2),       # 40 taps, the largest accepted; 17 filters: a second filter group with one real filter
    ((3, 3, 1, 1, 1, 1, 1, 3), 2),         # one tap, one filter
    ((8, 8, 1, 1, 6, 7, 4, 1), 1),         # 42 taps: the plane-major form, whatever is asked for
]


@pytest.fixture(scope="module")
def eng():
    import crcnn_amd as ca
    E = ca.Engine(N, Q, 1 << 20, device=0)
    yield E, ca
    E.set_tuning("conv1_form", 0)
    E.close()


# ---- exact references --------------------------------------------------------------------------------------------------------------------------------------
def rand_rows(rng, lead, edge=False):
    out = np.empty(lead + (len(Q), N), dtype=np.uint64)
    for i, q in enumerate(Q):
        if edge:
            out[..., i, :] = rng.choice(np.array([0, 1, q - 1, q // 2, q // 2 + 1, digit_extreme(q, True), digit_extreme(q, False)], dtype=np.uint64), size=lead + (N,))
        else:
            out[..., i, :] = rng.integers(0, q, size=lead + (N,), dtype=np.uint64)
    return out


def shl_mod(v, bits, qa):
    """v 2^bits mod q for v < q < 2^55, eight bits at a time (v 2^8 < 2^63)"""
    while bits:
        s = min(8, bits)
        v = (v << np.uint64(s)) % qa
        bits -= s
    return v


def exact_conv(x, w, bias, xs, ys):
    """x [B][xd][yd][2][k][n], w [F][xf][yf][k][n], bias [F][k][n] canonical residues -> y [B][F][xo][yo][2][k][n] = sum over the window + bias on poly 0, mod q"""
    B, xd, yd = x.shape[:3]
    F, xf, yf = w.shape[:3]
    assert xf * yf <= 64
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    k, n = x.shape[-2:]
    qa = np.array(Q, dtype=np.uint64).reshape(k, 1)
    m28 = np.uint64((1 << 28) - 1)
    xl, xh, wl, wh = x & m28, x >> np.uint64(28), w & m28, w >> np.uint64(28)
    s = [np.zeros((B, F, xo, yo, 2, k, n), dtype=np.uint64) for _ in range(4)]         # ll, lh, hl, hh: each below 64 2^56 = 2^62
    for kx in range(xf):
        for ky in range(yf):
            sl = (slice(None), None, slice(kx, kx + (xo - 1) * xs + 1, xs), slice(ky, ky + (yo - 1) * ys + 1, ys))
            a, b = xl[sl], xh[sl]
            c, d = wl[:, kx, ky][None, :, None, None, None], wh[:, kx, ky][None, :, None, None, None]
            s[0] += a * c; s[1] += a * d; s[2] += b * c; s[3] += b * d
    mid = (s[1] % qa + s[2] % qa) % qa
    y = (s[0] % qa + shl_mod(mid, 28, qa) + shl_mod(s[3] % qa, 56, qa)) % qa
    y[:, :, :, :, 0] = (y[:, :, :, :, 0] + bias[None, :, None, None]) % qa
    return y


def exact_conv_python(x, w, bias, xs, ys):
    """the same in Python integers, term by term (as tests/test_gpu_mac_bounds.py::test_conv1_full_window_extreme_digits)"""
    B, xd, yd = x.shape[:3]
    F, xf, yf = w.shape[:3]
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    k, n = x.shape[-2:]
    xo_, wo, qo = x.astype(object), w.astype(object), np.array(Q, dtype=object).reshape(k, 1)
    want = np.empty((B, F, xo, yo, 2, k, n), dtype=np.uint64)
    for b in range(B):
        for i in range(xo):
            for j in range(yo):
                patch = xo_[b, i * xs:i * xs + xf, j * ys:j * ys + yf]                    # [xf][yf][2][k][n]
                for f in range(F):
                    acc = (patch * wo[f][:, :, None]).sum(axis=(0, 1))
                    acc[0] = acc[0] + bias[f].astype(object)
                    want[b, f, i, j] = (acc % qo).astype(np.uint64)
    return want


# ---- running the layer under a form ------------------------------------------------------------------------------------------------------------------------
class Layer:
    """operands of one case on the device; run(form, ...) packs the weights under that form and runs crc_conv2d_forms"""

    def __init__(self, E, ca, shape, x, w, bias):
        self.E, self.ca, self.shape = E, ca, shape
        xd, yd, xs, ys, xf, yf, nf, B = shape
        self.xo, self.yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
        self.d_x, self.d_w, self.d_b = E.upload(x), E.upload(w), E.upload(bias)
        self.rows_y = B * nf * self.xo * self.yo * 2 * E.k
        self.nb_limb = E.limb_tensor_bytes(B, nf, self.xo, self.yo)
        self.d_wl = E.alloc(E.limb_conv1_weights_bytes())

    def run(self, form, expect_form, fin=None, fout=None, d_x=None):
        E, ca = self.E, self.ca
        xd, yd, xs, ys, xf, yf, nf, B = self.shape
        fin = ca.NTT if fin is None else fin
        fout = ca.NTT if fout is None else fout
        E.set_tuning("conv1_form", form)
        assert E.limb_conv1_supported(1, xd, yd, xs, ys, xf, yf, nf)
        assert E.limb_conv1_form(1, xd, yd, xs, ys, xf, yf, nf) == expect_form, (self.shape, form)
        assert E.limb_conv1_weights_bytes_for(nf, xf, yf) <= E.limb_conv1_weights_bytes()
        E.limb_conv1_pack_weights(self.d_w, nf, xf, yf, self.d_wl)
        limb = fout in (ca.NTTLC, ca.NTTL)
        nbytes = self.nb_limb if limb else self.rows_y * E.n * 8
        d_y = E.alloc(nbytes)
        E.L.crc_memset(E.c, E.p(d_y), 0 if limb else 0xff, nbytes, E.stream)          # (a limb tensor's padding is nobody's to write; a u64 result left unwritten cannot pass)
        d_work = E.alloc(E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, fin, ca.NTTL1, fout))
        E.conv2d(self.d_x if d_x is None else d_x, self.d_wl, self.d_b, B, 1, xd, yd, xs, ys, xf, yf, nf, fin, fout, d_y, d_work, w_form=ca.NTTL1)
        E.sync()
        out = E.download(d_y, (nbytes // 8,)) if limb else E.download(d_y, (self.rows_y, E.n))
        d_y.free(); d_work.free()
        return out

    def both(self, expect2, **kw):
        """the layer under conv1_form = 1 and = 2: equal bytes"""
        y1 = self.run(1, 1, **kw)
        y2 = self.run(2, expect2, **kw)
        assert np.array_equal(y1, y2), (self.shape, kw, "the two forms differ")
        return y2

    def limb_of(self, want):
        """the limb tensor crc_limb_pack_tensor makes of the exact NTT-form result"""
        E, ca = self.E, self.ca
        xd, yd, xs, ys, xf, yf, nf, B = self.shape
        d_ref = E.alloc(self.nb_limb); E.L.crc_memset(E.c, E.p(d_ref), 0, self.nb_limb, E.stream)
        E.limb_pack_tensor(E.upload(np.ascontiguousarray(want).reshape(-1)), ca.NTT, B, nf, self.xo, self.yo, d_ref)
        E.sync()
        return E.download(d_ref, (self.nb_limb // 8,))


def operands(rng, shape, edge):
    xd, yd, xs, ys, xf, yf, nf, B = shape
    return rand_rows(rng, (B, xd, yd, 2), edge), rand_rows(rng, (nf, xf, yf), edge), rand_rows(rng, (nf,), edge)


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True], ids=["uniform", "edge"])
@pytest.mark.parametrize("shape,form2", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_conv1_forms_equal_exact_integers(eng, shape, form2, edge):
    E, ca = eng
    xd, yd, xs, ys, xf, yf, nf, B = shape
    rng = np.random.default_rng(xd * 1000 + yf * 10 + nf + edge)
    x, w, bias = operands(rng, shape, edge)
    want = exact_conv(x, w, bias, xs, ys)
    if want.size <= 200_000:
        assert np.array_equal(want, exact_conv_python(x, w, bias, xs, ys))          # the uint64 reference against Python integers
    L = Layer(E, ca, shape, x, w, bias)
    y = L.both(form2)
    assert np.array_equal(y, want.reshape(L.rows_y, E.n)), (shape, edge)


# ---- extreme digits at 40 taps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("neg", "pos"), ("neg", "neg"), ("pos", "pos"), ("mix", "mix")], ids=lambda k: "-".join(k))
def test_conv1_pixel_major_extreme_digits(eng, kinds):
    """40 taps with every image digit at its extreme; filter l has the weights e 256^-l mod q, so that W'_l = centred(w 256^l) = e carries the extreme digits in
    image-limb plane l (seven filters, l = 0 .. 6); bias q - 1; checked term by term in Python integers"""
    E, ca = eng
    k = E.k
    shape = (8, 10, 1, 1, 5, 8, 7, 2)
    xd, yd, xs, ys, xf, yf, nf, B = shape
    rng = np.random.default_rng(len(kinds[0]) + 40)
    ext = {"neg": lambda qi: [digit_extreme(qi, True)], "pos": lambda qi: [digit_extreme(qi, False)],
           "mix": lambda qi: [0, qi - 1, digit_extreme(qi, True), digit_extreme(qi, False), limb_extreme(qi)]}
    for qi in Q:
        for low in (True, False):
            c = digit_extreme(qi, low); c = c - qi if c > qi >> 1 else c
            assert balanced_digits(c)[:6] == [-128 if low else 127] * 6

    def draw(lead, kind):
        out = np.empty(lead + (k, N), dtype=np.uint64)
        for i, qi in enumerate(Q):
            v = np.array(ext[kind](qi), dtype=np.uint64)
            out[..., i, :] = v[rng.integers(0, len(v), size=lead + (N,))]
        return out
    x = draw((B, xd, yd, 2), kinds[0])
    e = draw((nf, xf, yf), kinds[1])
    w = np.empty_like(e)
    for f in range(nf):
        for i, qi in enumerate(Q):
            inv = pow(256, -f, qi)
            w[f, :, :, i] = (e[f, :, :, i].astype(object) * inv % qi).astype(np.uint64)
            assert np.array_equal((w[f, :, :, i].astype(object) * pow(256, f, qi) % qi).astype(np.uint64), e[f, :, :, i])       # W'_f = e
    x[0, 3, 4] = rng.integers(0, Q54, size=(2, k, N), dtype=np.uint64)        # a marker
    bias = np.tile((np.array(Q, dtype=np.uint64) - 1).reshape(1, k, 1), (nf, 1, N))
    want = exact_conv_python(x, w, bias, xs, ys)
    L = Layer(E, ca, shape, x, w, bias)
    assert np.array_equal(L.both(2), want.reshape(L.rows_y, E.n)), kinds
    # ... and into the limb tensor of a following convolution (7 filters: the flat form)
    assert np.array_equal(L.both(2, fout=ca.NTTLC), L.limb_of(want)), kinds


# ---- operand forms, hand-overs, several passes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0][0], SHAPES[1][0]], ids=["blocked-32-filters", "flat-5-filters"])
def test_conv1_pixel_major_forms_and_handover(eng, shape):
    """coefficient-form and 28-bit packed input, u64 and packed output, and the limb tensor handed to a following convolution: 32 filters write the blocked
    [7][P][2][32] form, 5 filters the flat one"""
    E, ca = eng
    xd, yd, xs, ys, xf, yf, nf, B = shape
    rng = np.random.default_rng(nf)
    x, w, bias = operands(rng, shape, False)
    want = exact_conv(x, w, bias, xs, ys)
    L = Layer(E, ca, shape, x, w, bias)
    flat = want.reshape(L.rows_y, E.n)
    d_xc = E.upload(x); E.ntt_inv(d_xc, B * xd * yd)
    assert np.array_equal(L.both(2, fin=ca.COEFF, d_x=d_xc), flat), "coefficient-form input"
    d_xp = E.upload(x); E.pack28(d_xp, B * xd * yd * 2 * E.k)
    m28 = np.uint64((1 << 28) - 1)
    assert np.array_equal(L.both(2, fin=ca.NTTP, fout=ca.NTTP, d_x=d_xp), (flat & m28) | ((flat >> np.uint64(28)) << np.uint64(32))), "packed input and output"
    assert np.array_equal(L.both(2, fout=ca.NTTLC), L.limb_of(want)), "limb tensor"


def test_conv1_pixel_major_single_pixel_dense_handover(eng):
    """a 1 x 1 result is a dense layer's input: the K-blocked limb tensor, made from the slot-major result"""
    E, ca = eng
    shape = (5, 8, 1, 1, 5, 8, 9, 3)
    xd, yd, xs, ys, xf, yf, nf, B = shape
    rng = np.random.default_rng(58)
    x, w, bias = operands(rng, shape, False)
    want = exact_conv_python(x, w, bias, xs, ys)
    L = Layer(E, ca, shape, x, w, bias)
    L.nb_limb = E.limb_tensor_bytes(B, nf)
    assert np.array_equal(L.both(2), want.reshape(L.rows_y, E.n))
    y = L.both(2, fout=ca.NTTL)
    d_ref = E.alloc(L.nb_limb); E.L.crc_memset(E.c, E.p(d_ref), 0, L.nb_limb, E.stream)
    E.limb_pack_tensor(E.upload(want.reshape(-1)), ca.NTT, B, nf, 1, 1, d_ref); E.sync()
    assert np.array_equal(y, E.download(d_ref, (L.nb_limb // 8,)))


def test_conv1_pixel_major_multi_pass(eng, request):
    """conv1_pass_bytes at a third of the whole work space: the batch runs in sub-batches -- same ciphertexts, same limb tensor, under both forms"""
    E, ca = eng
    shape = (28, 28, 2, 2, 6, 6, 32, 5)
    xd, yd, xs, ys, xf, yf, nf, B = shape
    rng = np.random.default_rng(5)
    x, w, bias = operands(rng, shape, False)
    want = exact_conv(x, w, bias, xs, ys)
    L = Layer(E, ca, shape, x, w, bias)
    request.addfinalizer(lambda: E.set_tuning("conv1_pass_bytes", 0))
    for form in (1, 2):
        E.set_tuning("conv1_form", form); E.set_tuning("conv1_pass_bytes", 0)
        whole = E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL1, ca.NTT)
        E.set_tuning("conv1_pass_bytes", whole // 3)
        assert E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL1, ca.NTT) < whole // 2
        assert np.array_equal(L.run(form, form), want.reshape(L.rows_y, E.n)), form
        assert np.array_equal(L.run(form, form, fout=ca.NTTLC), L.limb_of(want)), form


def test_conv1_form_switch_and_sizes(eng):
    """the tuning key, its fall-back and the weight sizes"""
    E, ca = eng
    per_slot = 7 * 32 * 64
    E.set_tuning("conv1_form", 0)
    assert E.limb_conv1_weights_bytes() == E.n * E.k * per_slot * 5
    assert E.limb_conv1_weights_bytes_for(20, 7, 7) == E.n * E.k * per_slot                   # 49 taps: plane-major only
    assert E.limb_conv1_form(1, 28, 28, 2, 2, 7, 7, 20) == 1
    assert E.limb_conv1_form(2, 28, 28, 2, 2, 6, 6, 32) == 0                                   # not a one-channel shape
    for form, want in ((1, 1), (2, 2)):
        E.set_tuning("conv1_form", form)
        assert E.limb_conv1_form(1, 28, 28, 2, 2, 6, 6, 32) == want
        assert E.limb_conv1_form(1, 28, 28, 2, 2, 7, 7, 20) == 1                               # a forced form the shape cannot take falls back
        assert E.limb_conv1_weights_bytes_for(32, 6, 6) == E.n * E.k * per_slot * (5 if want == 2 else 1)
    E.set_tuning("conv1_form", 0)
    assert E.limb_conv1_form(1, 10, 9, 1, 1, 3, 3, 17) == 1                                    # 17-20 filters keep the packed second filter group
