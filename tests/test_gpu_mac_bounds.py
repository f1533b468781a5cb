"""GPU exactness of the multiply-accumulate kernels at their worst-case operands and at their term-count limits.

Every conv / dense layer runs through one of six MAC kernels, each exact only by an overflow argument that depends on T, the number of reduction terms:
  * mac3_kernel / mac2_kernel / mac_stream_kernel (kernels.hip): 28-bit limbs, Karatsuba terms below 2^57.2 in 64-bit lazy sums, bit 63 parked in a 10-bit
    overflow field every 32 terms -- "exact up to 16 000 terms";
  * mac_kernel (kernels.hip): 128-bit sums, refuses a layer unless 2 bits + ceil(log2 T) <= 127;
  * the int8 limb GEMM (kernels_mfma.hip) and mfma_conv1_kernel (kernels_mfma1.hip): balanced base-256 digits into biased int32 diagonals -- T <= 18 000.
Uniform residues leave those bounds far away (Karatsuba terms about 4x below the maximum), so the operands here are the extreme ones: residues whose limb sum
(r mod 2^28) + (r >> 28) is maximal, q - 1, residues whose balanced digits are all -128 / all +127, next to zeros and uniform residues.  Bias rows are q - 1.

Reference.  Long reductions are not summed term by term in Python: every operand is a short periodic background plus a few "marker" terms at random positions
(always the first and the last term among them), so the exact sum is (T // p) periods + the remainder - the background products at the markers + the marker
products, in Python integers.  The markers catch term-index and offset errors a periodic operand would hide.  Short reductions are also checked term by term.

Which kernel a case reaches follows from k_mac2's dispatch (kernels.hip) and is recorded in profiles/mac_bounds_kernel_stats.csv (rocprofv3 --kernel-trace --stats
over this module) and, test by test, in profiles/mac_bounds_kernels_by_test.txt: mac3 holds its term table in LDS beside its stage buffers, 2 VEC 512 + 16 ceil((T + 8) / 4) + 1024 <= 160 KiB, i.e. T <= 7928 with the 12 x 8
tile and T <= 12024 with the 6 x 16 tile; past that, and for moduli without a fold constant, mac2_kernel; past 16 000 terms, mac_kernel."""
import numpy as np
import pytest

from netcommon import limb_extreme

pytestmark = pytest.mark.gpu

M28 = (1 << 28) - 1
Q55, Q54, Q55B = 0x7fffffff380001, 0x3fffffff000001, 0x7ffffffef00001          # 2^b - d, d < 2^26: mac3 / mac_stream fold
Q40 = 0xffffe80001                                                             # 40 bits: no fold constant (mac2_kernel's Barrett epilogue)
Q55NF = 0x7fffffbffd0001                                                       # 55 bits, 2^55 - q > 2^26: no fold constant either
Q60 = 0xffffffffffc0001                                                        # 60 bits: mac_kernel only
T_MAC3 = {8: 7928, 16: 12024}                                                  # largest T whose term table fits beside mac3's stage buffers, per tile (k_mac2 "pick")
TILES = {8: (7, 3), 16: (2, 5)}                                                # (M = B images, F filters) for which the padding rule picks 12 x 8 / 6 x 16


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------
def balanced_digits(c):
    d = []
    for _ in range(7):
        v = ((c + 128) & 255) - 128
        d.append(v); c = (c - v) >> 8
    assert c == 0
    return d


def digit_extreme(q, low):
    """centred representative c, |c| <= q >> 1, whose balanced base-256 digits d0..d5 are all -128 (low) or all +127, d6 as extreme as that allows"""
    d05 = -128 if low else 127
    base = sum(d05 << (8 * l) for l in range(6))
    h = q >> 1
    d6 = -((h + base) >> 48) if low else (h - base) >> 48                    # floor division: the most extreme d6 with |c| <= q >> 1
    c = base + d6 * (1 << 48)
    assert -h <= c <= h and not (-h <= c + (-1 if low else 1) * (1 << 48) <= h)
    dg = balanced_digits(c)
    assert dg[:6] == [d05] * 6 and dg[6] == d6
    return c % q


class Operands:
    """x [B][T][2][k][n] and w [F][T][k][n]: periodic backgrounds xbg [B][p][2][k][n], wbg [F][p][k][n] plus marker terms at positions xpos / wpos"""

    def __init__(self, rng, q, n, B, T, F, xvals, wvals, p=3, markers=5):
        k = len(q)
        qa = np.array(q, dtype=np.uint64)

        def bg(lead, vals):
            # vals: per modulus, the background values to draw from (one value: a constant background)
            out = np.empty(lead + (k, n), dtype=np.uint64)
            for i in range(k):
                v = np.array(vals[i], dtype=np.uint64)
                out[..., i, :] = v[rng.integers(0, len(v), size=lead + (n,))]
            return out

        def uniform(lead):
            return rng.integers(0, 1 << 62, size=lead + (k, n), dtype=np.uint64) % qa.reshape(k, 1)

        self.q, self.n, self.k, self.B, self.T, self.F, self.p = q, n, k, B, T, F, p
        self.xbg = bg((B, p, 2), xvals); self.wbg = bg((F, p), wvals)
        reps = -(-T // p)
        self.x = np.ascontiguousarray(np.tile(self.xbg, (1, reps, 1, 1, 1))[:, :T])
        self.w = np.ascontiguousarray(np.tile(self.wbg, (1, reps, 1, 1))[:, :T])
        self.xpos = sorted({0, T - 1} | set(rng.integers(0, T, size=markers).tolist()))
        self.wpos = sorted({T - 1} | set(rng.integers(0, T, size=markers).tolist()))
        self.x[:, self.xpos] = uniform((B, len(self.xpos), 2))
        self.w[:, self.wpos] = uniform((F, len(self.wpos)))
        self.bias = np.tile((qa - 1).reshape(1, k, 1), (F, 1, n))             # q - 1 bias rows

    def want(self):
        """exact y [B][F][2][k][n]: periods + remainder - background products at the markers + marker products, + bias on poly 0, mod q"""
        xo, wo = self.xbg.astype(object), self.wbg.astype(object)
        per = [xo[:, j][:, None] * wo[:, j][None, :, None] for j in range(self.p)]       # [B][F][2][k][n]
        acc = sum(per) * (self.T // self.p) + sum(per[:self.T % self.p], 0 * per[0])
        for t in sorted(set(self.xpos) | set(self.wpos)):
            acc = acc + self.x[:, t].astype(object)[:, None] * self.w[:, t].astype(object)[None, :, None] - per[t % self.p]
        acc[:, :, 0] += self.bias.astype(object)[None]
        qo = np.array(self.q, dtype=object).reshape(self.k, 1)
        return (acc % qo).astype(np.uint64)

    def want_termwise(self):
        acc = (self.x.astype(object)[:, None] * self.w.astype(object)[None, :, :, None]).sum(axis=2)
        acc[:, :, 0] += self.bias.astype(object)[None]
        return (acc % np.array(self.q, dtype=object).reshape(self.k, 1)).astype(np.uint64)


def values(q, kind):
    """per modulus, the background values of an operand kind"""
    make = {"limb": lambda qi: [limb_extreme(qi)], "qm1": lambda qi: [qi - 1], "zero": lambda qi: [0],
            "mix": lambda qi: [limb_extreme(qi), qi - 1, 0, int(np.random.default_rng(qi & 0xffff).integers(0, qi)), limb_extreme(qi)],
            "neg": lambda qi: [digit_extreme(qi, True)], "pos": lambda qi: [digit_extreme(qi, False)]}[kind]
    return [make(qi) for qi in q]


def split28(v):
    return (v & np.uint64(M28)) | ((v >> np.uint64(28)) << np.uint64(32))


# ---- running a dense layer ------------------------------------------------------------------------------------------------------------------------------
_ENGINES = {}


@pytest.fixture(scope="module")
def engines():
    yield _ENGINES
    for E in _ENGINES.values():
        E.close()
    _ENGINES.clear()


def engine(engines, n, q):
    import crcnn_amd as ca
    key = (n, tuple(q))
    if key not in engines:
        engines[key] = ca.Engine(n, q, 1 << 20, device=0)
    return engines[key]


@pytest.fixture
def tuned(request):
    """set_tuning(E, name, value) for this test, reset to the defaults afterwards"""
    done = []

    def set_(E, name, value, default):
        E.set_tuning(name, value); done.append((E, name, default))
    yield set_
    for E, name, default in reversed(done):
        E.set_tuning(name, default)


def run_dense(E, op, fin=None, fw=None, fout=None):
    import crcnn_amd as ca
    fin = ca.NTT if fin is None else fin; fw = ca.NTT if fw is None else fw; fout = ca.NTT if fout is None else fout
    B, T, F, k, n = op.B, op.T, op.F, E.k, E.n
    d_x = E.upload(op.x)
    if fin == ca.NTTP:
        E.pack28(d_x, B * T * 2 * k)
    d_w = E.upload(op.w.reshape(F * T, k, n))
    if fw == ca.NTTP:
        E.pack28(d_w, F * T * k)
    d_b = E.upload(op.bias)
    ybytes = B * F * 2 * k * n * 8
    d_y = E.alloc(ybytes)
    E.L.crc_memset(E.c, E.p(d_y), 0xff, ybytes, E.stream)            # an output the kernel does not write cannot pass
    d_work = E.alloc(E.dense_work_bytes(B, T, F, fin))
    E.dense(d_x, d_w, d_b, B, T, F, fin, fout, d_y, d_work, w_form=fw)
    y = E.download(d_y, (B, F, 2, k, n))
    for d in (d_x, d_w, d_b, d_y, d_work):
        d.free()
    return y


def check_dense(E, op, want=None, forms=((None, None, None),)):
    import crcnn_amd as ca
    want = op.want() if want is None else want
    for fin, fw, fout in forms:
        y = run_dense(E, op, fin, fw, fout)
        exp = split28(want) if fout == ca.NTTP else want
        bad = np.argwhere(y != exp)
        assert bad.size == 0, f"T={op.T} B={op.B} F={op.F} forms={(fin, fw, fout)}: {len(bad)} wrong residues, first at {bad[0].tolist()}"


# ---- mac3_kernel: both tiles, both walk orders, around the parking windows -----------------------------------------------------------------------------
PARK_T = [31, 32, 33, 63, 64, 65, 255, 256, 257, 1100]          # 1100: past the 569 limb-extreme terms at which parking every 64 terms overflows


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tile", [8, 16])
def test_mac3_parking_windows(engines, tuned, tile, order):
    """limb-extreme x and w (every Karatsuba middle term at its maximum) over T around 32 / 64 / 256 and past 569 terms; (n / 64) k = 4 and 8 slot blocks
    (the plain and the XCD-ordered block decode)"""
    B, F = TILES[tile]
    rng = np.random.default_rng(100 * tile + order)
    for n, q in ((128, [Q55, Q54]), (256, [Q55B, Q55])):
        E = engine(engines, n, q)
        tuned(E, "mac_order", order, -1)
        for T in PARK_T:
            op = Operands(rng, q, n, B, T, F, values(q, "limb"), values(q, "limb"))
            want = op.want()
            if T <= 65:
                assert np.array_equal(want, op.want_termwise())           # the periodic reference against the term-by-term one
            check_dense(E, op, want)


@pytest.mark.parametrize("tile", [8, 16])
def test_mac3_operand_kinds_and_forms(engines, tile):
    """q - 1, zero, mixed and uniform backgrounds; canonical and packed (CRC_NTTP) operands in and out"""
    import crcnn_amd as ca
    B, F = TILES[tile]
    rng = np.random.default_rng(7 + tile)
    forms = ((ca.NTT, ca.NTT, ca.NTT), (ca.NTTP, ca.NTTP, ca.NTTP), (ca.NTTP, ca.NTT, ca.NTT), (ca.NTT, ca.NTTP, ca.NTTP))
    for n, q in ((256, [Q55, Q54]), (128, [Q55, Q54, Q55B])):
        E = engine(engines, n, q)
        for xk, wk in (("qm1", "qm1"), ("zero", "limb"), ("mix", "mix"), ("limb", "qm1")):
            op = Operands(rng, q, n, B, 301, F, values(q, xk), values(q, wk), p=4)
            check_dense(E, op, forms=forms)
        op = Operands(rng, q, n, B, 97, F, [[int(v) for v in rng.integers(0, qi, 16)] for qi in q], [[int(v) for v in rng.integers(0, qi, 16)] for qi in q], p=5)
        check_dense(E, op, op.want_termwise(), forms=forms)


def test_mac3_lds_limit_and_mac2_beyond(engines):
    """default settings at T = the largest term table mac3 holds beside each tile's stage buffers and one term more (-> the register-staged mac2_kernel)"""
    rng = np.random.default_rng(5)
    q, n = [Q55], 128
    E = engine(engines, n, q)
    for tile, tmax in T_MAC3.items():
        B, F = TILES[tile]
        for T in (tmax, tmax + 1):
            check_dense(E, Operands(rng, q, n, B, T, F, values(q, "limb"), values(q, "limb")))


# ---- mac2_kernel: non-foldable moduli under default settings, and the tuning knobs -------------------------------------------------------------------------
@pytest.mark.parametrize("q", [[Q40], [Q55NF, Q55]], ids=["q40", "q55nofold"])
def test_mac2_nonfoldable_modulus(engines, q):
    """a modulus without a fold constant keeps mac3 / mac_stream off: mac2_kernel and its own recombination + Barrett epilogue, both tiles, packed forms"""
    import crcnn_amd as ca
    rng = np.random.default_rng(len(q))
    n = 128
    E = engine(engines, n, q)
    forms = ((ca.NTT, ca.NTT, ca.NTT), (ca.NTTP, ca.NTTP, ca.NTTP))
    for tile in (8, 16):
        B, F = TILES[tile]
        for T in (33, 65, 257, 1100):
            check_dense(E, Operands(rng, q, n, B, T, F, values(q, "limb"), values(q, "limb")), forms=forms)
        check_dense(E, Operands(rng, q, n, B, 300, F, values(q, "mix"), values(q, "qm1"), p=4), forms=forms)
    # batch 1 on a ring the weight stream would take: still mac2 (the stream kernel folds too)
    E2 = engine(engines, 512, q)
    check_dense(E2, Operands(rng, q, 512, 1, 600, 3, values(q, "limb"), values(q, "limb")), forms=forms)


@pytest.mark.parametrize("cfg", [8, 16])
def test_mac2_tuning_knobs(engines, tuned, cfg):
    """mac_regstage = 1 and mac2_cfg = 8 / 16 force mac2_kernel with a foldable modulus"""
    import crcnn_amd as ca
    rng = np.random.default_rng(cfg)
    for n, q in ((128, [Q55, Q54]), (256, [Q55B, Q54])):
        E = engine(engines, n, q)
        tuned(E, "mac_regstage", 1, 0); tuned(E, "mac2_cfg", cfg, 0)
        B, F = TILES[cfg]
        for T in (31, 32, 33, 63, 64, 65, 257, 1100):
            check_dense(E, Operands(rng, q, n, B, T, F, values(q, "limb"), values(q, "limb")))
        check_dense(E, Operands(rng, q, n, B, 200, F, values(q, "mix"), values(q, "mix"), p=4),
                    forms=((ca.NTT, ca.NTT, ca.NTT), (ca.NTTP, ca.NTTP, ca.NTTP)))


# ---- mac_stream_kernel: a dense layer on one image ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2, 3, 4, 5])
def test_mac_stream_shapes(engines, tuned, shape):
    """shapes 1-5 at n = 1024, k = 2 (n / 256 SL k = 8: the XCD-ordered decode for SL = 1, 4 slot blocks for SL = 2) and n = 512, k = 1; nine filters leave a partial
    filter group for every FT"""
    import crcnn_amd as ca
    rng = np.random.default_rng(shape)
    forms = ((ca.NTT, ca.NTT, ca.NTT), (ca.NTTP, ca.NTTP, ca.NTTP))
    for n, q in ((1024, [Q55, Q54]), (512, [Q55B])):
        E = engine(engines, n, q)
        tuned(E, "mac_stream", shape, 1)
        for T in (31, 32, 33, 63, 64, 65, 1100):
            check_dense(E, Operands(rng, q, n, 1, T, 9, values(q, "limb"), values(q, "limb")), forms=forms if T == 1100 else forms[:1])
        check_dense(E, Operands(rng, q, n, 1, 257, 9, values(q, "mix"), values(q, "qm1"), p=4), forms=forms)


# ---- past the vector-ALU contract: mac_kernel ----------------------------------------------------------------------------------------------------------
def test_16000_terms_and_beyond(engines):
    """T = 16 000 is the last reduction of the limb kernels (mac2_kernel: past mac3's term table), T = 16 001 goes to mac_kernel's 128-bit sums; both exact"""
    rng = np.random.default_rng(16)
    q, n = [Q55], 128
    E = engine(engines, n, q)
    for T in (16000, 16001):
        check_dense(E, Operands(rng, q, n, 2, T, 5, values(q, "limb"), values(q, "limb")))
        check_dense(E, Operands(rng, q, n, 2, T, 5, values(q, "qm1"), values(q, "limb"), p=2))


def test_mac_kernel_60bit_limit(engines):
    """a 60-bit modulus: mac_kernel up to 2 * 60 + ceil(log2 T) <= 127, i.e. 128 terms, exact at q - 1 everywhere; 129 terms are refused"""
    import crcnn_amd as ca
    rng = np.random.default_rng(60)
    q, n = [Q60], 128
    E = engine(engines, n, q)
    assert E.plan_mac(128, 1, 1, 1, 1, 1, 1, 4, 2) == ca.NTT                  # canonical weights: no packed form above 55 bits
    for T in (1, 64, 127, 128):
        check_dense(E, Operands(rng, q, n, 3, T, 5, values(q, "qm1"), values(q, "qm1"), p=1))
        op = Operands(rng, q, n, 3, T, 5, values(q, "mix"), values(q, "qm1"), p=4)
        check_dense(E, op, op.want_termwise())
    op = Operands(rng, q, n, 3, 129, 5, values(q, "qm1"), values(q, "qm1"), p=1)
    with pytest.raises(ca.CrcError):
        run_dense(E, op)


# ---- limb GEMM (kernels_mfma.hip) ------------------------------------------------------------------------------------------------------------------
def limb_weights(q, c):
    """NTT-form weight whose limb-form image (w 2^64 mod q, what limb_pack_weights digitises) is the residue c"""
    return c * pow(1 << 64, -1, q) % q


def run_dense_limb(E, op):
    import crcnn_amd as ca
    B, T, F, k, n = op.B, op.T, op.F, E.k, E.n
    d_w = E.upload(op.w.reshape(F * T, k, n))
    d_wl = E.alloc(E.limb_weights_bytes(F, T, 1, 1)); E.limb_pack_weights(d_w, F, T, 1, 1, d_wl); d_w.free()
    d_x = E.upload(op.x); d_b = E.upload(op.bias)
    ybytes = B * F * 2 * k * n * 8
    d_y = E.alloc(ybytes); E.L.crc_memset(E.c, E.p(d_y), 0xff, ybytes, E.stream)
    d_work = E.alloc(E.conv2d_forms_work_bytes(B, T, 1, 1, 1, 1, 1, 1, F, ca.NTT, ca.NTTL, ca.NTT))
    E.dense(d_x, d_wl, d_b, B, T, F, ca.NTT, ca.NTT, d_y, d_work, w_form=ca.NTTL)
    y = E.download(d_y, (B, F, 2, k, n))
    for d in (d_x, d_wl, d_b, d_y, d_work):
        d.free()
    return y


LIMB_KINDS = [("neg", "pos"), ("neg", "neg"), ("pos", "pos")]     # most negative / most positive diagonals


@pytest.mark.parametrize("variant", [1, 2])
def test_limb_gemm_term_limit(engines, tuned, variant):
    """dense-shaped limb GEMM (w_form = CRC_NTTL) with every digit d0..d5 of x and of the limb-form weights at -128 or +127 and d6 at its extreme, up to
    in_dim = 17 984 (T = 17 984, the largest multiple of 32 within T <= 18 000); in_dim = 17 985 pads to T = 18 016 and is refused, and crc_plan_mac does not
    choose the limb form there"""
    import crcnn_amd as ca
    rng = np.random.default_rng(variant)
    q, n = [Q55], 64
    E = engine(engines, n, q)
    tuned(E, "mfma_variant", variant, 2)
    for T, B, F, kinds in ((70, 3, 10, LIMB_KINDS), (1000, 2, 3, LIMB_KINDS[:2]), (17984, 2, 3, LIMB_KINDS[:2])):
        for xk, wk in kinds:
            wv = [[limb_weights(qi, c) for c in vs] for qi, vs in zip(q, values(q, wk))]
            op = Operands(rng, q, n, B, T, F, values(q, xk), wv, p=1)
            for qi, c in zip(q, values(q, wk)):
                assert (wv[0][0] << 64) % qi == c[0]
            y = run_dense_limb(E, op)
            assert np.array_equal(y, op.want()), (variant, T, xk, wk)
    # mixed background: zeros, q - 1, uniform and the digit extremes
    mixed = [[0, qi - 1, digit_extreme(qi, True), digit_extreme(qi, False), int(rng.integers(0, qi))] for qi in q]
    op = Operands(rng, q, n, 2, 333, 66, mixed, mixed, p=5)
    assert np.array_equal(run_dense_limb(E, op), op.want())
    # the limit
    assert E.limb_supported(17984) and not E.limb_supported(17985)
    assert E.plan_mac(17984, 1, 1, 1, 1, 1, 1, 3, 0) == ca.NTTL
    for B in (0, 1, 64):
        assert E.plan_mac(17985, 1, 1, 1, 1, 1, 1, 3, B) != ca.NTTL
        assert E.plan_mac(18001, 1, 1, 1, 1, 1, 1, 3, B) != ca.NTTL
    # (buffers of the sizes the layer would need if it ran: a refusal that came too late would still stay inside them)
    T, B, F = 17985, 2, 3
    steps = -(-T // 32) + (-(-T // 32) & 1)
    d_w = E.alloc(F * T * E.k * n * 8); d_wl = E.alloc(n * E.k * steps * 7 * 64 * 32)
    with pytest.raises(ca.CrcError):
        E.limb_pack_weights(d_w, F, T, 1, 1, d_wl)
    d_x = E.alloc(B * T * 2 * E.k * n * 8); d_b = E.alloc(F * E.k * n * 8); d_y = E.alloc(B * F * 2 * E.k * n * 8)
    d_work = E.alloc(n * E.k * B * 7 * 2 * steps * 32 + 8 * n * E.k * B * F * 2 + (1 << 20))
    with pytest.raises(ca.CrcError):
        E.dense(d_x, d_wl, d_b, B, T, F, ca.NTT, ca.NTT, d_y, d_work, w_form=ca.NTTL)


# ---- mfma_conv1_kernel: the 8 x 8 window -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", LIMB_KINDS + [("mix", "mix")], ids=lambda k: "-".join(k))
def test_conv1_full_window_extreme_digits(engines, kinds):
    """one-channel convolution on the matrix cores (w_form = CRC_NTTL1) with an 8 x 8 window: 64 terms per output, every digit at its extreme; checked term
    by term.  (The one-channel form takes the weights as they are: no 2^64 factor.)"""
    import crcnn_amd as ca
    rng = np.random.default_rng(len(kinds[0]))
    q, n = [Q55, Q54], 64
    E = engine(engines, n, q)
    k = E.k
    xd, yd, xf, yf, nf, B = 10, 9, 8, 8, 7, 2
    assert E.limb_conv1_supported(1, xd, yd, 1, 1, xf, yf, nf)
    xo, yo = xd - xf + 1, yd - yf + 1
    ext = {"neg": lambda qi: [digit_extreme(qi, True)], "pos": lambda qi: [digit_extreme(qi, False)],
           "mix": lambda qi: [0, qi - 1, digit_extreme(qi, True), digit_extreme(qi, False), limb_extreme(qi)]}

    def draw(lead, kind):
        out = np.empty(lead + (k, n), dtype=np.uint64)
        for i, qi in enumerate(q):
            v = np.array(ext[kind](qi), dtype=np.uint64)
            out[..., i, :] = v[rng.integers(0, len(v), size=lead + (n,))]
        return out
    x = draw((B, 1, xd, yd, 2), kinds[0]); w = draw((nf, 1, xf, yf), kinds[1])
    x[0, 0, 3, 4] = rng.integers(0, Q54, size=(2, k, n), dtype=np.uint64)        # a marker
    bias = np.tile((np.array(q, dtype=np.uint64) - 1).reshape(1, k, 1), (nf, 1, n))
    xo_, wo, qo = x.astype(object), w.astype(object), np.array(q, dtype=object).reshape(k, 1)
    want = np.empty((B, nf, xo, yo, 2, k, n), dtype=np.uint64)
    for b in range(B):
        for i in range(xo):
            for j in range(yo):
                patch = xo_[b, 0, i:i + xf, j:j + yf]                                   # [xf][yf][2][k][n]
                for f in range(nf):
                    acc = (patch * wo[f, 0][:, :, None]).sum(axis=(0, 1))
                    acc[0] = acc[0] + bias[f].astype(object)
                    want[b, f, i, j] = (acc % qo).astype(np.uint64)
    d_w = E.upload(w)
    d_wl = E.alloc(E.limb_conv1_weights_bytes()); E.limb_conv1_pack_weights(d_w, nf, xf, yf, d_wl)
    d_y = E.alloc(want.nbytes)
    d_work = E.alloc(E.conv2d_forms_work_bytes(B, 1, xd, yd, 1, 1, xf, yf, nf, ca.NTT, ca.NTTL1, ca.NTT))
    E.conv2d(E.upload(x), d_wl, E.upload(bias), B, 1, xd, yd, 1, 1, xf, yf, nf, ca.NTT, ca.NTT, d_y, d_work, w_form=ca.NTTL1)
    assert np.array_equal(E.download(d_y, want.shape), want), kinds


# ---- a convolution-shaped reduction (gathered terms) on the vector ALU -------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [[Q55, Q54], [Q40]], ids=["fold", "q40"])
def test_conv_gather_extreme_operands(engines, tuned, q):
    """crc_conv2d with a 3 x 3 window over 37 channels (T = 333) and stride 2: the term table, not the term index, addresses x; limb-extreme operands with
    uniform markers, checked term by term"""
    import crcnn_amd as ca
    rng = np.random.default_rng(len(q) + 33)
    n = 64
    E = engine(engines, n, q)
    k = E.k
    zd, xd, yd, xs, ys, xf, yf, nf, B = 37, 7, 6, 2, 2, 3, 3, 5, 2
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    L = np.array([limb_extreme(qi) for qi in q], dtype=np.uint64).reshape(k, 1)
    x = np.tile(L, (B, zd, xd, yd, 2, 1, n)); w = np.tile(L, (nf, zd, xf, yf, 1, n))
    qa = np.array(q, dtype=np.uint64).reshape(k, 1)
    for _ in range(6):
        x[tuple(rng.integers(0, s) for s in (B, zd, xd, yd))] = rng.integers(0, 1 << 62, size=(2, k, n), dtype=np.uint64) % qa
        w[tuple(rng.integers(0, s) for s in (nf, zd, xf, yf))] = rng.integers(0, 1 << 62, size=(k, n), dtype=np.uint64) % qa
    bias = np.tile(qa - 1, (nf, 1, n))
    xo_, wo, qo = x.astype(object), w.astype(object), np.array(q, dtype=object).reshape(k, 1)
    want = np.empty((B, nf, xo, yo, 2, k, n), dtype=np.uint64)
    for b in range(B):
        for i in range(xo):
            for j in range(yo):
                patch = xo_[b, :, i * xs:i * xs + xf, j * ys:j * ys + yf]
                for f in range(nf):
                    acc = (patch * wo[f][:, :, :, None]).sum(axis=(0, 1, 2))
                    acc[0] = acc[0] + bias[f].astype(object)
                    want[b, f, i, j] = (acc % qo).astype(np.uint64)
    d_x, d_w, d_b = E.upload(x), E.upload(w), E.upload(bias)
    d_y = E.alloc(want.nbytes)
    d_work = E.alloc(E.conv2d_work_bytes(B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT))
    for order in (0, 1):
        tuned(E, "mac_order", order, -1)
        E.L.crc_memset(E.c, E.p(d_y), 0xff, want.nbytes, E.stream)
        E.conv2d(d_x, d_w, d_b, B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTT, d_y, d_work)
        assert np.array_equal(E.download(d_y, want.shape), want), order
