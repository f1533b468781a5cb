"""GPU exactness of the boxed forward transform (crc_ntt_fwd_box: the bxf x byf window of coefficient-form ciphertexts summed while the transform loads its row)
and of the one-channel layer that uses it (crc_conv2d_box_forms on coefficient-form input, tuning key box_ntt).

The kernel alone, bit for bit against crc_ntt_fwd of EVERY input ciphertext summed mod q in numpy (at most nine terms below 2^55: the sums fit 64 bits):
rings 2048 (k = 1), 4096 (2), 8192 (3), 16384 (2) -- every form of the load loop, scalar loads at 16384 --, 3 images of 7 x 6 pixels (row counts that are no
multiple of 8 or of the XCD group), boxes 2 x 2 / 2, 1 x 2, 2 x 1, 3 x 3 / 1 (nine terms) and 2 x 2 / 3, both block orders, operands random, all q - 1 (nine
of them: the largest sum the reduction sees), all 0 and around q / 2; the input is unchanged, and rows of the output buffer past the result keep their 0xff.
n = 1024 and a 10-term box answer CRC_ERR_UNSUPPORTED, and at n = 1024 the boxed layer on coefficient-form input still equals its NTT-form-input result (the
fall-back).  The layer: PlainModelTiny's conv1 with the 2 x 2 box on three coefficient-form images, box_ntt = 0 (transform all, staged box), 1 and 2 -- identical
rows and an identical limb tensor, in one pass and in passes of one image."""
import numpy as np
import pytest

from test_gpu_conv1_box import Boxed

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4
Q4096 = [0x7fffffff380001, 0x3fffffff000001]
RINGS = {2048: [0x3fffffff000001], 4096: Q4096, 8192: [0x7fffffff380001, 0x7ffffffef00001, 0x3fffffff000001], 16384: [0x7fffffff380001, 0x7ffffffef00001]}
B, XD, YD = 3, 7, 6
BOXES = [(2, 2, 2, 2), (1, 2, 1, 1), (2, 1, 1, 1), (3, 3, 1, 1), (2, 2, 3, 3)]              # bxf, byf, xs, ys
KINDS = {
    "random": None,
    "all-q-1": lambda q: [q - 1],
    "all-0": lambda q: [0],
    "around-half": lambda q: [q // 2, q // 2 + 1, q // 2 - 1, (q + 1) // 2 + 1],
}
TINY = (1, 28, 28, 2, 2, 6, 6, 32)


def rand_rows(rng, lead, n, Q, values=None):
    """canonical residues [lead][k][n]: uniform, or drawn from values(q)"""
    out = np.empty(lead + (len(Q), n), dtype=np.uint64)
    for i, q in enumerate(Q):
        if values is None:
            out[..., i, :] = rng.integers(0, q, size=lead + (n,), dtype=np.uint64)
        else:
            v = np.array(values(q), dtype=np.uint64)
            out[..., i, :] = v[rng.integers(0, len(v), size=lead + (n,))]
    return out


@pytest.fixture(scope="module", params=list(RINGS), ids=lambda n: f"n{n}")
def ring(request):
    import crcnn_amd as ca
    n = request.param
    E = ca.Engine(n, RINGS[n], 1 << 20, device=0)
    yield E, ca, n, RINGS[n]
    E.set_tuning("box_ntt", 1)
    E.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_against_summed_transforms(ring, kind):
    E, ca, n, Q = ring
    k = len(Q)
    x = rand_rows(np.random.default_rng(1200 + n), (B, XD, YD, 2), n, Q, KINDS[kind])
    d_x = E.upload(x)
    d_t = E.upload(x); E.ntt_fwd(d_t, B * XD * YD)
    each = E.download(d_t, x.shape)                                  # the transform of every input ciphertext: the reference, computed once and left unchanged
    d_t.free()
    qcol = np.array(Q, dtype=np.uint64).reshape(1, 1, 1, 1, k, 1)
    d_y = E.alloc(x.nbytes)
    for bxf, byf, xs, ys in BOXES:
        xdo, ydo = XD - (bxf - 1) * xs, YD - (byf - 1) * ys
        assert xdo >= 1 and ydo >= 1
        want = np.zeros((B, xdo, ydo, 2, k, n), dtype=np.uint64)
        for a in range(bxf):
            for bb in range(byf):
                want += each[:, a * xs:a * xs + xdo, bb * ys:bb * ys + ydo]
        want %= qcol
        for order in (1, 2):
            E.set_tuning("box_ntt", order)
            E.L.crc_memset(E.c, E.p(d_y), 0xff, x.nbytes, E.stream)
            E.ntt_fwd_box(d_x, d_y, B, XD, YD, bxf, byf, xs, ys)
            got = E.download(d_y, (x.size,))
            assert np.array_equal(got[:want.size], want.reshape(-1)), (n, kind, (bxf, byf, xs, ys), order)
            assert np.all(got[want.size:] == np.uint64(0xffffffffffffffff)), ("rows past the result written", n, (bxf, byf, xs, ys), order)
    assert np.array_equal(E.download(d_x, x.shape), x), "the input changed"
    d_x.free(); d_y.free()


def test_ten_terms_unsupported(ring):
    E, ca, n, Q = ring
    d_x, d_y = E.alloc(B * XD * YD * 2 * len(Q) * n * 8), E.alloc(B * XD * YD * 2 * len(Q) * n * 8)
    for bxf, byf in ((2, 5), (5, 2)):
        with pytest.raises(ca.CrcError) as e:
            E.ntt_fwd_box(d_x, d_y, B, XD, YD, bxf, byf, 1, 1)
        assert e.value.status == UNSUPPORTED
    d_x.free(); d_y.free()


def layer(E, ca, n, Q, nimg, seed):
    rng = np.random.default_rng(seed)
    zd, xd, yd, xs, ys, xf, yf, nf = TINY
    return Boxed(E, ca, TINY, (2, 2), nimg, rand_rows(rng, (nimg, xd, yd, 2), n, Q), rand_rows(rng, (nf, xf, yf), n, Q), rand_rows(rng, (nf,), n, Q))


def test_ring_1024_unsupported_and_fallback():
    import crcnn_amd as ca
    n = 1024
    E = ca.Engine(n, Q4096, 1 << 20, device=0)
    try:
        d_x, d_y = E.alloc(B * XD * YD * 2 * 2 * n * 8), E.alloc(B * XD * YD * 2 * 2 * n * 8)
        with pytest.raises(ca.CrcError) as e:
            E.ntt_fwd_box(d_x, d_y, B, XD, YD, 2, 2, 2, 2)
        assert e.value.status == UNSUPPORTED
        # the layer does not ask for what the ring does not have: coefficient-form input still runs, through the transform of every input and the staged box
        L = layer(E, ca, n, Q4096, 1, 1301)
        want = L.boxed()
        d_xc = E.upload(L.x); E.ntt_inv(d_xc, 28 * 28)
        assert np.array_equal(L.boxed(fin=ca.COEFF, d_x=d_xc), want)
    finally:
        E.close()


def test_layer_identical_under_every_setting():
    """PlainModelTiny's conv1 + box on three coefficient-form images at n = 2048: box_ntt = 0 is the sequence the layer ran before it had the boxed transform"""
    import crcnn_amd as ca
    n, Q = 2048, RINGS[2048]
    E = ca.Engine(n, Q, 1 << 20, device=0)
    try:
        L = layer(E, ca, n, Q, 3, 1302)
        d_xc = E.upload(L.x); E.ntt_inv(d_xc, 3 * 28 * 28)
        whole = E.conv2d_box_forms_work_bytes(3, *TINY, 2, 2, ca.COEFF, ca.NTTL1, ca.NTT)
        for passes in ("one pass", "passes of one image"):
            if passes != "one pass":
                E.set_tuning("conv1_pass_bytes", whole * 2 // 5)
                assert E.conv2d_box_forms_work_bytes(3, *TINY, 2, 2, ca.COEFF, ca.NTTL1, ca.NTT) < whole * 3 // 5
            E.set_tuning("box_ntt", 0)
            rows0, limb0 = L.boxed(fin=ca.COEFF, d_x=d_xc), L.boxed(fin=ca.COEFF, fout=ca.NTTLC, d_x=d_xc)
            if passes == "one pass":
                assert np.array_equal(rows0, L.boxed()), "coefficient-form and NTT-form input differ before the boxed transform is even on"
            for order in (1, 2):
                E.set_tuning("box_ntt", order)
                assert np.array_equal(L.boxed(fin=ca.COEFF, d_x=d_xc), rows0), (passes, order)
                assert np.array_equal(L.boxed(fin=ca.COEFF, fout=ca.NTTLC, d_x=d_xc), limb0), (passes, order)
    finally:
        E.close()
