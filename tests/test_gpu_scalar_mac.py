"""The scalar limb form (CRC_NTTLS): conv / dense layers of a slot-batched network, whose weights are constant polynomials -- one residue per modulus.

Every comparison is bit for bit.  The reference is the existing path: crc_conv2d_forms with w_form = CRC_NTT on the same weights expanded to constant rows (the
goldens pin that path to the reference implementation).  The packed weight bytes are checked against a numpy statement of the layout: the balanced base-256 digits
of w 2^64 mod q in CRC_NTTL's container for a one-slot ring, zero padding, a zero step behind an odd step count.

Rings are n = 256 with Q = {0x7fffffff380001, 0x3fffffff000001} unless a case says otherwise."""
import numpy as np
import pytest

from test_gpu_mac_bounds import LIMB_KINDS, Q55, Q60, Operands, limb_weights, values

pytestmark = pytest.mark.gpu

N, Q = 256, [0x7fffffff380001, 0x3fffffff000001]
UNSUPPORTED = -4

_ENGINES = {}


@pytest.fixture(scope="module")
def engines():
    yield _ENGINES
    for E in _ENGINES.values():
        E.close()
    _ENGINES.clear()


def engine(engines, n=N, q=Q):
    import crcnn_amd as ca
    key = (n, tuple(q))
    if key not in engines:
        engines[key] = ca.Engine(n, q, 1 << 20, device=0)
    return engines[key]


# ---- operands -------------------------------------------------------------------------------------------------------------------------------------------
def residues(rng, q, lead, tail=()):
    """uniform residues [lead..][k][tail..] with 0, q - 1, floor(q / 2) and floor(q / 2) + 1 planted in every modulus"""
    k = len(q)
    out = np.empty(lead + (k,) + tail, dtype=np.uint64)
    for i, qi in enumerate(q):
        v = rng.integers(0, qi, size=lead + tail, dtype=np.uint64)
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, size=min(8, flat.size), replace=False)
        for j, p in enumerate(pos):
            flat[p] = (0, qi - 1, qi >> 1, (qi >> 1) + 1)[j % 4]
        out[(slice(None),) * len(lead) + (i,)] = v
    return out


def split28(v):
    m = np.uint64((1 << 28) - 1)
    return (v & m) | ((v >> np.uint64(28)) << np.uint64(32))


def rows_of(ws, n):
    """k-word scalars [nf][zd][xf][yf][k] -> constant NTT rows [nf][zd][xf][yf][k][n]"""
    return np.ascontiguousarray(np.broadcast_to(ws[..., None], ws.shape + (n,)))


def round_up(v, m):
    return -(-v // m) * m


def packed_weights_ref(ws, q):
    """the CRC_NTTLS weight bytes [k][steps rounded up to even][7][Fp][32] of scalars ws [nf][zd][xf][yf][k]"""
    nf, zd, xf, yf, k = ws.shape
    Fp = round_up(nf, 64)
    zdc = round_up(zd, 4) if zd < 32 else 0                        # flat form: channel bytes per position
    S = -(-(yf * zdc) // 32) if zdc else 0
    zblks = round_up(zd, 32) // 32
    steps = xf * S if zdc else xf * yf * zblks
    out = np.zeros((k, round_up(steps, 2), 7, Fp, 32), dtype=np.int8)
    for i, qi in enumerate(q):
        v = ws[..., i].astype(object) * (1 << 64) % qi
        c = np.where(v > (qi >> 1), v - qi, v)                      # centred representative
        dig = np.empty(c.shape + (7,), dtype=np.int8)
        for l in range(7):
            d = ((c + 128) & 255) - 128
            dig[..., l] = d.astype(np.int64); c = (c - d) >> 8
        assert not c.any()
        for kx in range(xf):
            for ky in range(yf):
                for ch in range(zd):
                    if zdc:
                        j = ky * zdc + ch; step, byte = kx * S + j // 32, j % 32
                    else:
                        step, byte = (kx * yf + ky) * zblks + ch // 32, ch % 32
                    out[i, step, :, :nf, byte] = dig[:, ch, kx, ky].T
    return out


class Layer:
    """one conv / dense shape with its operands on the device: x rows, constant weight rows, the scalar pack of the weights, non-constant bias rows"""

    def __init__(self, E, rng, B, zd, xd, yd, xs, ys, xf, yf, nf, ws=None, x=None):
        import crcnn_amd as ca
        self.E, self.geom, self.B = E, (zd, xd, yd, xs, ys, xf, yf, nf), B
        n, k, q = E.n, E.k, [int(v) for v in E.q]
        self.P = ((xd - xf) // xs + 1) * ((yd - yf) // ys + 1)
        self.ws = residues(rng, q, (nf, zd, xf, yf)) if ws is None else ws
        self.x = residues(rng, q, (B, zd, xd, yd, 2), (n,)) if x is None else x
        self.bias = residues(rng, q, (nf,), (n,))                   # ordinary NTT rows: every slot its own value
        self.d_x = E.upload(self.x); self.d_b = E.upload(self.bias)
        self.d_xp = E.upload(self.x); E.pack28(self.d_xp, B * zd * xd * yd * 2 * k)
        self.d_w = E.upload(rows_of(self.ws, n))
        assert E.scalar_supported(B, *self.geom)
        self.d_ws = E.alloc(E.scalar_weights_bytes(nf, zd, xf, yf))
        assert E.scalar_pack_weights(self.d_w, n, nf, zd, xf, yf, self.d_ws) is True
        self.ybytes = B * nf * self.P * 2 * k * n * 8
        self.NTT, self.NTTLS = ca.NTT, ca.NTTLS

    def run(self, w_form, in_form, out_form, d_x=None, d_bias=None, out_bytes=None):
        import crcnn_amd as ca
        E, B = self.E, self.B
        d_x = d_x if d_x is not None else {ca.NTTP: self.d_xp}.get(in_form, self.d_x)
        nbytes = out_bytes or self.ybytes
        d_y = E.alloc(nbytes)
        E.L.crc_memset(E.c, E.p(d_y), 0xff, nbytes, E.stream)            # an output the kernel does not write cannot pass
        d_work = E.alloc(E.conv2d_forms_work_bytes(B, *self.geom, in_form, w_form, out_form))
        d_w = self.d_ws if w_form == ca.NTTLS else self.d_w
        E.conv2d(d_x, d_w, self.d_b if d_bias is None else d_bias, B, *self.geom, in_form, out_form, d_y, d_work, w_form=w_form)
        E.sync(); d_work.free()
        return d_y

    def rows(self, w_form, in_form, out_form, d_x=None):
        d_y = self.run(w_form, in_form, out_form, d_x)
        y = self.E.download(d_y, (self.B, self.geom[7], self.P, 2, self.E.k, self.E.n)); d_y.free()
        return y

    def check(self, in_forms, out_forms, what):
        for fi in in_forms:
            for fo in out_forms:
                ref, got = self.rows(self.NTT, fi, fo), self.rows(self.NTTLS, fi, fo)
                bad = np.argwhere(ref != got)
                assert bad.size == 0, f"{what} B={self.B} in_form={fi} out_form={fo}: {len(bad)} wrong residues, first at {bad[0].tolist()}"

    def free(self):
        for d in (self.d_x, self.d_xp, self.d_b, self.d_w, self.d_ws):
            d.free()


def coeff_input(E, L):
    """the layer's input in coefficient form (the inverse transform of its NTT rows), for in_form = CRC_COEFF"""
    d = E.upload(L.x); B, (zd, xd, yd) = L.B, L.geom[:3]
    E.ntt_inv(d, B * zd * xd * yd)
    return d


# ---- the weight pack --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(50, 20, 3, 3), (33, 40, 3, 3), (10, 70, 1, 1)], ids=["flat", "blocked", "dense-odd-steps"])
def test_pack_matches_the_layout(engines, shape):
    """rows (stride n) and k-word scalars (stride 1) give the bytes of the numpy statement of the layout; a row with one differing word is refused"""
    E = engine(engines)
    rng = np.random.default_rng(sum(shape))
    nf, zd, xf, yf = shape
    ws = residues(rng, Q, (nf, zd, xf, yf))
    want = packed_weights_ref(ws, Q)
    nbytes = E.scalar_weights_bytes(nf, zd, xf, yf)
    assert nbytes == want.nbytes and nbytes * N == E.limb_weights_bytes(nf, zd, xf, yf)
    rows = rows_of(ws, N)
    for src, stride in ((rows, N), (ws, 1)):
        d_src = E.upload(src); d_ws = E.alloc(nbytes)
        E.L.crc_memset(E.c, E.p(d_ws), 0x55, nbytes, E.stream)           # the pack writes its padding itself
        assert E.scalar_pack_weights(d_src, stride, nf, zd, xf, yf, d_ws) is True
        got = E.download(d_ws, want.shape, dtype=np.int8)
        assert np.array_equal(got, want), f"stride {stride}: {np.argwhere(got != want)[:4].tolist()}"
        d_src.free(); d_ws.free()
    # one word of one row differs: not a constant polynomial -- refused with constant == 0, nothing written
    rows[nf - 1, zd // 2, xf - 1, 0, 1, N - 3] ^= np.uint64(1)
    d_src = E.upload(rows); d_ws = E.alloc(nbytes)
    E.L.crc_memset(E.c, E.p(d_ws), 0x55, nbytes, E.stream)
    assert E.scalar_pack_weights(d_src, N, nf, zd, xf, yf, d_ws) is False
    assert (E.download(d_ws, (nbytes,), dtype=np.uint8) == 0x55).all()


# ---- dense layers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dims", [(70, 10), (1000, 33)], ids=["70x10", "1000x33"])
def test_dense(engines, dims, B):
    """3 steps padded to 4 with 10 filters in a 64-filter container; 32 steps with two ragged 32-filter tiles.  Non-constant biases prove the per-slot bias read"""
    import crcnn_amd as ca
    E = engine(engines)
    L = Layer(E, np.random.default_rng(dims[0] + B), B, dims[0], 1, 1, 1, 1, 1, 1, dims[1])
    L.check((ca.NTT, ca.NTTP), (ca.COEFF, ca.NTT, ca.NTTP), f"dense {dims}")
    L.free()


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------------------------
CONVS = {"blocked-P25": (40, 7, 7, 1, 1, 3, 3, 33), "flat-P16": (20, 6, 6, 1, 1, 3, 3, 50), "flat-P9-stride2": (20, 7, 7, 2, 2, 3, 3, 50)}


@pytest.mark.parametrize("name", list(CONVS))
def test_conv(engines, name):
    """blocked form with P = 25 (row tiles straddle images), flat form with P = 16 and, at stride 2, P = 9; rows in every form and the limb tensor (CRC_NTTL, the
    bytes conv1 hands over) as input"""
    import crcnn_amd as ca
    E = engine(engines)
    geom = CONVS[name]
    L = Layer(E, np.random.default_rng(len(name)), 2, *geom)
    L.check((ca.NTT, ca.NTTP), (ca.NTT, ca.NTTP, ca.COEFF), name)
    ref = L.rows(ca.NTT, ca.NTT, ca.NTT)
    d_c = coeff_input(E, L)
    assert np.array_equal(L.rows(ca.NTTLS, ca.COEFF, ca.NTT, d_x=d_c), ref), f"{name}: in_form COEFF"
    d_xl = E.alloc(E.limb_tensor_bytes(2, geom[0], geom[1], geom[2]))
    E.limb_pack_tensor(L.d_x, ca.NTT, 2, geom[0], geom[1], geom[2], d_xl)
    assert np.array_equal(L.rows(ca.NTTLS, ca.NTTL, ca.NTT, d_x=d_xl), ref), f"{name}: in_form NTTL"
    d_c.free(); d_xl.free(); L.free()


# ---- hand-over between layers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat-P16", "flat-P9-stride2"])
def test_chain_conv_into_dense(engines, name):
    """conv with out_form = CRC_NTTLS (P = 16: written by the GEMM itself; P = 9: re-limbed from the slot-major result) into a scalar dense layer equals the pair
    through NTT rows; a scalar conv with out_form = CRC_NTTL feeds today's dense layer (w_form = CRC_NTTL) just the same"""
    import crcnn_amd as ca
    E = engine(engines)
    rng = np.random.default_rng(len(name) + 1)
    B, geom = 2, CONVS[name]
    C = Layer(E, rng, B, *geom)
    in_dim, out_dim = geom[7] * C.P, 10
    zdp = round_up(in_dim, 32)
    # the dense layer's x is never uploaded from the host here: a placeholder of one row keeps Layer's bookkeeping happy
    D = Layer(E, rng, B, in_dim, 1, 1, 1, 1, 1, 1, out_dim, x=np.zeros((B, in_dim, 1, 1, 2, E.k, E.n), dtype=np.uint64))
    d_mid = C.run(ca.NTT, ca.NTT, ca.NTT)
    ref = D.rows(ca.NTT, ca.NTT, ca.NTT, d_x=d_mid); d_mid.free()
    limb_bytes = E.limb_tensor_bytes(B, in_dim)
    assert limb_bytes == E.n * E.k * B * 7 * 2 * zdp
    d_mid = C.run(ca.NTTLS, ca.NTT, ca.NTTLS, out_bytes=limb_bytes)
    assert np.array_equal(D.rows(ca.NTTLS, ca.NTTLS, ca.NTT, d_x=d_mid), ref), f"{name}: NTTLS hand-over"
    d_mid.free()
    # scalar conv -> CRC_NTTL -> the per-slot limb GEMM on row weights
    d_mid = C.run(ca.NTTLS, ca.NTT, ca.NTTL, out_bytes=limb_bytes)
    d_wl = E.alloc(E.limb_weights_bytes(out_dim, in_dim)); E.limb_pack_weights(D.d_w, out_dim, in_dim, 1, 1, d_wl)
    d_y = E.alloc(D.ybytes); d_work = E.alloc(E.conv2d_forms_work_bytes(B, *D.geom, ca.NTTL, ca.NTTL, ca.NTT))
    E.dense(d_mid, d_wl, D.d_b, B, in_dim, out_dim, ca.NTTL, ca.NTT, d_y, d_work, w_form=ca.NTTL)
    assert np.array_equal(E.download(d_y, ref.shape), ref), f"{name}: NTTL hand-over"
    for d in (d_mid, d_wl, d_y, d_work):
        d.free()
    C.free(); D.free()


# ---- the term limit ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", LIMB_KINDS[:2], ids=lambda k: "-".join(k))
def test_term_limit(engines, kinds):
    """in_dim = 17 984, the largest T k_limb_supported admits: every digit d0..d5 of x and of the limb-form weights at -128 / +127 and d6 at its extreme, plus
    uniform markers (made constant over the slots on the weight side); against the exact sum and against the row path"""
    import crcnn_amd as ca
    q, n, T, F, B = [Q55], 256, 17984, 2, 1
    E = engine(engines, n, q)
    rng = np.random.default_rng(len(kinds[1]))
    wv = [[limb_weights(qi, c) for c in vs] for qi, vs in zip(q, values(q, kinds[1]))]
    op = Operands(rng, q, n, B, T, F, values(q, kinds[0]), wv, p=1)
    op.w[:, op.wpos] = op.w[:, op.wpos][..., :1]                      # a marker weight is a constant polynomial too
    op.bias = residues(rng, q, (F,), (n,))
    want = op.want()
    assert E.scalar_supported(B, T, 1, 1, 1, 1, 1, 1, F)
    d_w = E.upload(op.w.reshape(F * T, 1, n)); d_x = E.upload(op.x); d_b = E.upload(op.bias)
    d_ws = E.alloc(E.scalar_weights_bytes(F, T)); assert E.scalar_pack_weights(d_w, n, F, T, 1, 1, d_ws) is True
    ybytes = B * F * 2 * n * 8
    got = {}
    for wf, dw in ((ca.NTTLS, d_ws), (ca.NTT, d_w)):
        d_y = E.alloc(ybytes); E.L.crc_memset(E.c, E.p(d_y), 0xff, ybytes, E.stream)
        d_work = E.alloc(E.conv2d_forms_work_bytes(B, T, 1, 1, 1, 1, 1, 1, F, ca.NTT, wf, ca.NTT))
        E.dense(d_x, dw, d_b, B, T, F, ca.NTT, ca.NTT, d_y, d_work, w_form=wf)
        got[wf] = E.download(d_y, (B, F, 2, 1, n)); d_y.free(); d_work.free()
    assert np.array_equal(got[ca.NTTLS], want), kinds
    assert np.array_equal(got[ca.NTT], want), kinds
    for d in (d_w, d_x, d_b, d_ws):
        d.free()


# ---- the smallest ring ------------------------------------------------------------------------------------------------------------------------------------
def test_smallest_ring(engines):
    """n = 64, k = 1: two row tiles for a dense layer on one image per slot, a convolution whose tiles are four whole images"""
    import crcnn_amd as ca
    E = engine(engines, 64, [Q55])
    rng = np.random.default_rng(64)
    for B, geom in ((1, (70, 1, 1, 1, 1, 1, 1, 10)), (1, CONVS["flat-P16"]), (3, CONVS["blocked-P25"])):
        L = Layer(E, rng, B, *geom)
        L.check((ca.NTT,), (ca.NTT,), f"n=64 {geom}")
        L.free()


# ---- refusals, decided before anything is launched -----------------------------------------------------------------------------------------------------
def test_refusals_without_a_launch(engines):
    """crc_scalar_supported is 0 for a modulus above 55 bits, past 18 000 terms and past the 32-bit offsets of the tile engine (which are refused, not widened);
    the forms call then returns CRC_ERR_UNSUPPORTED.  Buffers have the sizes the layer would need if it ran"""
    import crcnn_amd as ca
    E = engine(engines)
    assert E.scalar_supported(1, 17984, 1, 1, 1, 1, 1, 1, 3) and not E.scalar_supported(1, 17985, 1, 1, 1, 1, 1, 1, 3)
    # a dense tensor of n B images x 7 planes x 2 polys x 1024 channel bytes reaches 4 GiB at B = 1171
    assert E.scalar_supported(1170, 1000, 1, 1, 1, 1, 1, 1, 33) and not E.scalar_supported(1171, 1000, 1, 1, 1, 1, 1, 1, 33)
    # ... and a slot-major result of n B images x 2 polys x 4096 filters reaches 2^32 words at B = 2048
    assert E.scalar_supported(2047, 32, 1, 1, 1, 1, 1, 1, 4096) and not E.scalar_supported(2048, 32, 1, 1, 1, 1, 1, 1, 4096)
    assert not E.scalar_supported(0, 70, 1, 1, 1, 1, 1, 1, 10)
    E.set_tuning("scalar_mac", 1)
    assert E.plan_mac_scalar(1000, 1, 1, 1, 1, 1, 1, 33, 1) == ca.NTTLS and E.plan_mac_scalar(17985, 1, 1, 1, 1, 1, 1, 3, 1) != ca.NTTLS

    def refused(G, B, T, F):
        n, k = G.n, G.k
        steps = round_up(-(-T // 32), 2)
        d_w = G.alloc(F * T * k * n * 8); d_ws = G.alloc(k * steps * 7 * 64 * 32)
        with pytest.raises(ca.CrcError) as e:
            G.scalar_pack_weights(d_w, n, F, T, 1, 1, d_ws)
        assert e.value.status == UNSUPPORTED
        d_x = G.alloc(B * T * 2 * k * n * 8); d_b = G.alloc(F * k * n * 8); d_y = G.alloc(B * F * 2 * k * n * 8)
        d_work = G.alloc(n * k * B * 7 * 2 * steps * 32 + 8 * n * k * B * F * 2 + (1 << 20))
        with pytest.raises(ca.CrcError) as e:
            G.dense(d_x, d_ws, d_b, B, T, F, ca.NTT, ca.NTT, d_y, d_work, w_form=ca.NTTLS)
        assert e.value.status == UNSUPPORTED
        for d in (d_w, d_ws, d_x, d_b, d_y, d_work):
            d.free()
    refused(E, 2, 17985, 3)
    G = engine(engines, 128, [Q60])
    assert not G.scalar_supported(1, 70, 1, 1, 1, 1, 1, 1, 10)
    refused(G, 2, 70, 10)
