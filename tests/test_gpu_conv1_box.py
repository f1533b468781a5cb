"""GPU exactness of the box of the one-channel convolution (crc_conv2d_box_forms: the image pack sums the input over a bxf x byf window at the layer's stride, the
pixel-major kernel keeps the base window), n = 256, k = 2, the moduli of test_gpu_conv1_pixel_major.py.  Every comparison is bit for bit with what the layer
replaces: the same map with the box folded into the WEIGHTS (crc_conv2d_fold_pool, the bias of that fold), run
  on the vector-ALU kernel, and
  on the one-channel matrix-core kernel at the enlarged window (8 x 8: the plane-major form),
as NTT-form rows and as the limb tensor handed to the convolution behind.  Shapes: PlainModelTiny's (242 rows, a ragged 16th row tile), boundary operands (every
residue q - 1, every residue 0, the centring boundaries), 1 x 2 and 2 x 1 boxes, an odd base window with an odd summed width, packed and coefficient-form inputs,
several passes with a ragged image count; and PlainModelTiny through the C++ classes: the reference's digest with the box, without it, and without the hoist."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs, sha
from test_gpu_hoist_pool import DRIVER, FOLDED, HOISTED
from test_gpu_mac_bounds import Q54, Q55

pytestmark = pytest.mark.gpu

N = 256
Q = [Q55, Q54]
TINY = (1, 28, 28, 2, 2, 6, 6, 32)


@pytest.fixture(scope="module")
def eng():
    import crcnn_amd as ca
    E = ca.Engine(N, Q, 1 << 20, device=0)
    yield E, ca
    E.set_tuning("conv1_pass_bytes", 0)
    E.close()


def rand_rows(rng, lead, values=None):
    """canonical residues [lead][k][n]: uniform, or drawn from values(q)"""
    out = np.empty(lead + (len(Q), N), dtype=np.uint64)
    for i, q in enumerate(Q):
        if values is None:
            out[..., i, :] = rng.integers(0, q, size=lead + (N,), dtype=np.uint64)
        else:
            v = np.array(values(q), dtype=np.uint64)
            out[..., i, :] = v[rng.integers(0, len(v), size=lead + (N,))]
    return out


class Boxed:
    """one layer's operands on the device: the base weights and their limb form, the enlarged weights and the bias of the fold"""

    def __init__(self, E, ca, base, box, B, x, w, bias):
        self.E, self.ca, self.base, self.box, self.B = E, ca, base, box, B
        zd, xd, yd, xs, ys, xf, yf, nf = base
        bxf, byf = box
        self.big = (zd, xd, yd, xs, ys, (bxf - 1) * xs + xf, (byf - 1) * ys + yf, nf)
        self.xo, self.yo = (xd - self.big[5]) // xs + 1, (yd - self.big[6]) // ys + 1
        assert E.limb_conv1_box_supported(*base, bxf, byf) and E.limb_conv1_form(zd, xd - (bxf - 1) * xs, yd - (byf - 1) * ys, xs, ys, xf, yf, nf) == 2
        self.x = x
        self.d_x, d_w, d_b = E.upload(x), E.upload(w), E.upload(bias)
        rowb = E.k * E.n * 8
        self.d_wbig, self.d_bbig = E.alloc(nf * self.big[5] * self.big[6] * rowb), E.alloc(nf * rowb)
        E.conv2d_fold_pool(d_w, d_b, None, nf, 1, xf, yf, xs, ys, bxf, byf, self.d_wbig, self.d_bbig)
        self.d_wl = E.alloc(E.limb_conv1_weights_bytes_for(nf, xf, yf)); E.limb_conv1_pack_weights(d_w, nf, xf, yf, self.d_wl)
        self.rows = B * nf * self.xo * self.yo * 2 * E.k
        self.nb_limb = E.limb_tensor_bytes(B, nf, self.xo, self.yo)

    def _out(self, fout):
        E, ca = self.E, self.ca
        limb = fout == ca.NTTLC
        nbytes = self.nb_limb if limb else self.rows * E.n * 8
        d_y = E.alloc(nbytes)
        E.L.crc_memset(E.c, E.p(d_y), 0 if limb else 0xff, nbytes, E.stream)       # (a limb tensor's padding is nobody's to write; a u64 result left unwritten cannot pass)
        return d_y, nbytes

    def enlarged(self, w_form, fout=None):
        """the map on the enlarged window: the vector-ALU kernel (w_form NTT) or the one-channel matrix-core kernel (NTTL1)"""
        E, ca = self.E, self.ca
        fout = ca.NTT if fout is None else fout
        zd, xd, yd, xs, ys, xf, yf, nf = self.big
        d_w = self.d_wbig
        if w_form == ca.NTTL1:
            assert E.limb_conv1_supported(*self.big)
            d_w = E.alloc(E.limb_conv1_weights_bytes_for(nf, xf, yf)); E.limb_conv1_pack_weights(self.d_wbig, nf, xf, yf, d_w)
        d_y, nbytes = self._out(fout)
        d_work = E.alloc(E.conv2d_forms_work_bytes(self.B, *self.big, ca.NTT, w_form, fout))
        E.conv2d(self.d_x, d_w, self.d_bbig, self.B, *self.big, ca.NTT, fout, d_y, d_work, w_form=w_form)
        E.sync()
        out = E.download(d_y, (nbytes // 8,))
        d_y.free(); d_work.free()
        return out

    def boxed(self, fin=None, fout=None, d_x=None):
        E, ca = self.E, self.ca
        fin, fout = ca.NTT if fin is None else fin, ca.NTT if fout is None else fout
        d_y, nbytes = self._out(fout)
        wb = E.conv2d_box_forms_work_bytes(self.B, *self.base, *self.box, fin, ca.NTTL1, fout)
        assert wb > 0
        d_work = E.alloc(wb)
        E.conv2d_box(self.d_x if d_x is None else d_x, self.d_wl, self.d_bbig, self.B, *self.base, *self.box, fin, fout, d_y, d_work)
        E.sync()
        out = E.download(d_y, (nbytes // 8,))
        d_y.free(); d_work.free()
        return out

    def limb_of(self, rows):
        E, ca = self.E, self.ca
        d_ref = E.alloc(self.nb_limb); E.L.crc_memset(E.c, E.p(d_ref), 0, self.nb_limb, E.stream)
        E.limb_pack_tensor(E.upload(rows), ca.NTT, self.B, self.base[7], self.xo, self.yo, d_ref)
        E.sync()
        return E.download(d_ref, (self.nb_limb // 8,))


def make(E, ca, base, box, B, seed, values=None):
    zd, xd, yd, xs, ys, xf, yf, nf = base
    rng = np.random.default_rng(seed)
    return Boxed(E, ca, base, box, B, rand_rows(rng, (B, xd, yd, 2), values), rand_rows(rng, (nf, xf, yf)), rand_rows(rng, (nf,)))


@pytest.fixture(scope="module")
def tiny(eng):
    """PlainModelTiny's layer on two images and its reference on the vector-ALU kernel, shared and left unchanged"""
    E, ca = eng
    L = make(E, ca, TINY, (2, 2), 2, 901)
    assert L.big == (1, 28, 28, 2, 2, 8, 8, 32) and (L.xo, L.yo) == (11, 11) and 2 * L.xo * L.yo == 242
    return L, L.enlarged(ca.NTT)


def test_tiny_shape_rows(eng, tiny):
    E, ca = eng
    L, want = tiny
    assert E.plan_mac(*L.big, 2) == ca.NTTL1 and E.limb_conv1_form(*L.big) == 1             # 64 taps: the plane-major form
    assert np.array_equal(L.enlarged(ca.NTTL1), want)
    assert np.array_equal(L.boxed(), want)


def test_tiny_shape_limb_tensor(eng, tiny):
    E, ca = eng
    L, want = tiny
    ref = L.limb_of(want)
    assert np.array_equal(L.enlarged(ca.NTTL1, ca.NTTLC), ref)
    assert np.array_equal(L.boxed(fout=ca.NTTLC), ref)


BOUNDARY = {
    "all-q-1": lambda q: [q - 1],
    "all-0": lambda q: [0],
    # the centred representative changes sign between q // 2 and q // 2 + 1; sums of two and four of them wrap around q
    "centring": lambda q: [q // 2, q // 2 + 1, q // 2 - 1, (q + 1) // 2 + 1],
}


@pytest.mark.parametrize("kind", list(BOUNDARY))
def test_tiny_shape_boundary_operands(eng, kind):
    E, ca = eng
    L = make(E, ca, TINY, (2, 2), 2, 902, BOUNDARY[kind])
    want = L.enlarged(ca.NTT)
    assert np.array_equal(L.enlarged(ca.NTTL1), want)
    assert np.array_equal(L.boxed(), want), kind
    assert np.array_equal(L.boxed(fout=ca.NTTLC), L.limb_of(want)), kind


@pytest.mark.parametrize("box", [(1, 2), (2, 1)], ids=["1x2", "2x1"])
def test_boxes_in_one_direction(eng, box):
    """28 x 26 and 26 x 28 summed images; the enlarged windows are 6 x 8 and 8 x 6 (48 taps: plane-major)"""
    E, ca = eng
    L = make(E, ca, TINY, box, 2, 903 + box[0])
    want = L.enlarged(ca.NTT)
    assert np.array_equal(L.enlarged(ca.NTTL1), want)
    assert np.array_equal(L.boxed(), want), box
    assert np.array_equal(L.boxed(fout=ca.NTTLC), L.limb_of(want)), box


def test_odd_base_window(eng):
    """3 x 3 / 1 on 14 x 14 with a 2 x 2 box: a 13 x 13 summed image (an odd width: one padding pixel per row), taps read one by one (no pairs)"""
    E, ca = eng
    L = make(E, ca, (1, 14, 14, 1, 1, 3, 3, 32), (2, 2), 2, 905)
    assert L.big == (1, 14, 14, 1, 1, 4, 4, 32) and (L.xo, L.yo) == (11, 11)
    want = L.enlarged(ca.NTT)
    assert np.array_equal(L.enlarged(ca.NTTL1), want)
    assert np.array_equal(L.boxed(), want)
    assert np.array_equal(L.boxed(fout=ca.NTTLC), L.limb_of(want))


def test_packed_and_coefficient_inputs(eng, tiny):
    E, ca = eng
    L, want = tiny
    zd, xd, yd = TINY[:3]
    d_xp = E.upload(L.x); E.pack28(d_xp, L.B * xd * yd * 2 * E.k)
    assert np.array_equal(L.boxed(fin=ca.NTTP, d_x=d_xp), want), "28-bit packed input"
    m28 = np.uint64((1 << 28) - 1)
    assert np.array_equal(L.boxed(fin=ca.NTTP, fout=ca.NTTP, d_x=d_xp), (want & m28) | ((want >> np.uint64(28)) << np.uint64(32))), "packed input and output"
    d_xc = E.upload(L.x); E.ntt_inv(d_xc, L.B * xd * yd)
    assert np.array_equal(L.boxed(fin=ca.COEFF, d_x=d_xc), want), "coefficient-form input"
    assert np.array_equal(L.boxed(fin=ca.COEFF, fout=ca.NTTLC, d_x=d_xc), L.limb_of(want)), "coefficient-form input, limb tensor"


def test_multi_pass_ragged_image_count(eng, request):
    """three images with conv1_pass_bytes at 0.4 of the whole work space: passes of one image"""
    E, ca = eng
    request.addfinalizer(lambda: E.set_tuning("conv1_pass_bytes", 0))
    L = make(E, ca, TINY, (2, 2), 3, 906)
    want = L.enlarged(ca.NTT)
    ref_limb = L.limb_of(want)
    whole = E.conv2d_box_forms_work_bytes(3, *TINY, 2, 2, ca.NTT, ca.NTTL1, ca.NTT)
    E.set_tuning("conv1_pass_bytes", whole * 2 // 5)
    assert E.conv2d_box_forms_work_bytes(3, *TINY, 2, 2, ca.NTT, ca.NTTL1, ca.NTT) < whole * 3 // 5
    assert np.array_equal(L.boxed(), want)
    assert np.array_equal(L.boxed(fout=ca.NTTLC), ref_limb)
    d_xc = E.upload(L.x); E.ntt_inv(d_xc, 3 * 28 * 28)
    assert np.array_equal(L.boxed(fin=ca.COEFF, d_x=d_xc), want)


# ---- the network through the C++ classes and through the Python twin ------------------------------------------------------------------------------------------
CONV1 = "pool1_features.conv1+pool1"


def run_netgeom_box(name, batch, env=None):
    """test_host netgeom: the fused layers' geometry, the box every conv / dense layer carries AFTER the forward (a layer that fell back to its enlarged window
    reports 1 x 1), the outputs"""
    g = load_net_golden(name)
    O, sk, pk, evk, img, x = make_inputs(g)
    d = tempfile.mkdtemp()
    np.array([g["n"], len(g["q"]), g["t"]] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    evk.tofile(os.path.join(d, "evk.u64")); x.tofile(os.path.join(d, "net_in.u64"))
    h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
    out = subprocess.run([DRIVER, "netgeom", g["model"], h5, d, str(batch), "0"], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    geom = {l[2]: tuple(int(v) for v in l[3:]) for l in lines if l and l[0] == "geom"}
    box = {l[2]: tuple(int(v) for v in l[3:]) for l in lines if l and l[0] == "box"}
    return g, geom, box, np.fromfile(os.path.join(d, "out.u64"), dtype=np.uint64).reshape(batch, -1)


@pytest.mark.parametrize("env,geometry,box1", [(None, HOISTED, (2, 2)), ({"CRC_CONV1_BOX": "0"}, HOISTED, (1, 1)), ({"CRC_HOIST_POOL": "0"}, FOLDED, (1, 1))],
                         ids=["box", "no-box", "no-hoist"])
def test_tiny256_digest_three_ways(env, geometry, box1):
    """the reference's digest all three ways; the first two report the same hoisted geometry, and only the first runs conv1 + pool1 boxed -- still boxed after the
    forward: no silent fall-back to the enlarged window"""
    g, geom, box, out = run_netgeom_box("tiny256", 3, env=env)
    for name, want in geometry.items():
        assert geom[name] == want, (name, geom)
    assert box[CONV1] == box1, box
    assert all(v == (1, 1) for k_, v in box.items() if k_ != CONV1), box
    for b in range(3):
        assert sha(out[b]) == g["out_sha256"], (env, b)


@pytest.mark.parametrize("boxed", [True, False], ids=["box", "no-box"])
def test_python_twin_fuses_the_same_way(boxed):
    """netrun.fuse() asks crc_plan_conv1_box like Network::fuse(): conv1 + pool1 keeps its 6 x 6 weights (36 taps in the one-channel form), carries the 2 x 2 box and
    reports the 8 x 8 map; under conv1_box = 0 it runs the enlarged window.  Either way the reference's digest -- the same ciphertexts as the C++ classes"""
    import crcnn_amd as ca
    from crcnn_amd.netrun import Network
    g = load_net_golden("tiny256")
    O, sk, pk, evk, img, x = make_inputs(g)
    E = ca.Engine(g["n"], g["q"], g["t"], device=0)
    try:
        E.set_tuning("conv1_box", 1 if boxed else 0)
        net = Network(E, g["model"], h5_path=os.path.join(GOLD, "models", g["model"] + ".h5"), resident=True, d_evk=E.upload(evk))
        net.fuse()
        kind, name, a, p, ishape, oshape = net.plan[0]
        assert (kind, name) == ("conv", CONV1) and tuple(a[k_] for k_ in ("zd", "xd", "yd", "xs", "ys", "xf", "yf", "nf")) == HOISTED[CONV1] and oshape == (32, 11, 11)
        assert p.get("box") == ((2, 2) if boxed else None)
        net.prepare(2)
        assert net.plan[0][3]["w_form"] == ca.NTTL1 and net.plan[0][3]["out_form"] == ca.NTTLC
        d_out = net.forward(E.upload(np.ascontiguousarray(np.repeat(x[None], 2, axis=0))), 2)
        out = E.download(d_out, (2, 1, 10, 1, 2, E.k, E.n))
        assert sha(out[0]) == g["out_sha256"] and sha(out[1]) == g["out_sha256"]
    finally:
        E.close()
