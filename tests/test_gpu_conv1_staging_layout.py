"""The limb result of the one-channel matrix-core convolution (kernels_mfma1.hip) is staged in LDS in the consumer's own layout and leaves as one linear copy, and
the pixel-major kernel reads a row's window and staging offsets from a per-workgroup table (crcnn_amd/csrc/conv1_rowtab.h; tests/cpp/conv1_rowtab_check.cpp walks
the table on the CPU).  Here the bytes: every case runs the layer to a limb tensor (CRC_NTTLC) and to canonical residues under conv1_form = 1 and = 2, asserts
through limb_conv1_form which form ran, and compares bit for bit with an exact integer convolution in numpy (test_gpu_conv1_pixel_major.exact_conv) and with the
limb tensor as tests/test_gpu_limb.py states the form (np_limb_tensor).  The output buffer is pre-filled with 0x55 and compared WHOLE -- the tensor's tail behind
the last image included --, so a stray or a missing 16-byte piece shows.

Shapes: one partial tile (8 rows), exactly one tile (16 rows), five tiles and a ragged sixth over three images (waves with one and with two tiles, both image
buffers, staging reuse), the shipped 26 x 26 geometry (242 rows, four tiles per wave), an odd window (two 8-byte reads per K group), and two flat consumers (5
and 20 filters; the second runs the plane-major kernel whatever is asked for: 49 taps).  Operands: uniform residues and the edge set {0, 1, (q-1)/2, (q+1)/2,
q-1}.  One run in sub-batches (conv1_pass_bytes: images land at b0 > 0 of the tensor)."""
import numpy as np
import pytest

import test_gpu_conv1_pixel_major as pm
from test_gpu_limb import np_limb_tensor

pytestmark = pytest.mark.gpu

N = 128
Q = [0x7fffffff380001, 0x3fffffff000001]
assert pm.Q == Q                                     # exact_conv reduces by these

SHAPES = [
    # xd, yd, xs, ys, xf, yf, nf, B  (zd = 1)          forms the shape takes under conv1_form = 1, 2
    ((3, 3, 1, 1, 2, 2, 32, 2), (1, 2)),           # 8 rows: one partial tile
    ((3, 5, 1, 1, 2, 2, 32, 2), (1, 2)),           # 16 rows: exactly one tile
    ((8, 7, 1, 1, 2, 2, 32, 3), (1, 2)),           # 84 rows: five tiles and a ragged sixth; three images
    ((26, 26, 2, 2, 6, 6, 32, 2), (1, 2)),         # the shipped geometry: 242 rows, four tiles per wave
    ((9, 9, 2, 2, 3, 3, 32, 2), (1, 2)),           # odd window: the two-ds_read_b64 path
    ((8, 7, 1, 1, 2, 2, 5, 3), (1, 2)),            # flat consumer
    ((28, 28, 2, 2, 7, 7, 20, 2), (1, 1)),         # flat consumer, 49 taps: plane-major under either setting
]


@pytest.fixture(scope="module")
def eng():
    import crcnn_amd as ca
    E = ca.Engine(N, Q, 1 << 20, device=0)
    yield E, ca
    E.set_tuning("conv1_form", 0); E.set_tuning("conv1_pass_bytes", 0)
    E.close()


def draw(rng, lead, edge):
    out = np.empty(lead + (len(Q), N), dtype=np.uint64)
    for i, q in enumerate(Q):
        if edge:
            out[..., i, :] = rng.choice(np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 1], dtype=np.uint64), size=lead + (N,))
        else:
            out[..., i, :] = rng.integers(0, q, size=lead + (N,), dtype=np.uint64)
    return out


_CASES = {}


def case(shape, edge):
    """operands and the exact results of a case, computed once and shared by the forms: canonical rows and the whole expected limb buffer's defined bytes"""
    key = (shape, edge)
    if key not in _CASES:
        xd, yd, xs, ys, xf, yf, nf, B = shape
        rng = np.random.default_rng(xd * 1000 + yd * 100 + nf * 3 + B + edge)
        x, w, bias = draw(rng, (B, xd, yd, 2), edge), draw(rng, (nf, xf, yf), edge), draw(rng, (nf,), edge)
        want = pm.exact_conv(x, w, bias, xs, ys)                                       # [B][F][xo][yo][2][k][n]
        if want.size <= 200_000:
            assert np.array_equal(want, pm.exact_conv_python(x, w, bias, xs, ys))
        xo, yo = want.shape[2:4]
        limb = np_limb_tensor(want.reshape(B, nf, xo * yo, 2, len(Q), N), Q, dense=False)
        for a in (x, w, bias, want, limb):
            a.setflags(write=False)
        _CASES[key] = (x, w, bias, want, limb)
    return _CASES[key]


def run(E, ca, shape, x, w, bias, form, expect_form, fout):
    """the layer under conv1_form = form into a buffer pre-filled with 0x55: the whole buffer, as bytes"""
    xd, yd, xs, ys, xf, yf, nf, B = shape
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    E.set_tuning("conv1_form", form)
    assert E.limb_conv1_supported(1, xd, yd, xs, ys, xf, yf, nf)
    assert E.limb_conv1_form(1, xd, yd, xs, ys, xf, yf, nf) == expect_form, (shape, form)
    d_x, d_w, d_b = E.upload(x), E.upload(w), E.upload(bias)
    d_wl = E.alloc(E.limb_conv1_weights_bytes())
    E.limb_conv1_pack_weights(d_w, nf, xf, yf, d_wl)
    nbytes = E.limb_tensor_bytes(B, nf, xo, yo) if fout == ca.NTTLC else B * nf * xo * yo * 2 * E.k * E.n * 8
    d_y = E.alloc(nbytes)
    E.L.crc_memset(E.c, E.p(d_y), 0x55, nbytes, E.stream)
    d_work = E.alloc(E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL1, fout))
    E.conv2d(d_x, d_wl, d_b, B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, fout, d_y, d_work, w_form=ca.NTTL1)
    E.sync()
    out = E.download(d_y, (nbytes,), dtype=np.int8)
    for d in (d_x, d_w, d_b, d_wl, d_y, d_work):
        d.free()
    return out


def expected_buffer(limb, nbytes):
    """the limb tensor's images (a flat image's round-up to 16 bytes is zero, as crc_limb_pack_tensor leaves it), 0x55 behind them"""
    buf = np.full(nbytes, 0x55, dtype=np.int8)
    assert limb.size <= nbytes
    buf[:limb.size] = limb.reshape(-1)
    return buf


def check_limb(got, limb, what):
    want = expected_buffer(limb, got.size)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} bytes differ, 16-byte pieces {sorted(set((bad // 16).tolist()))[:8]} .. of {got.size // 16}")


@pytest.mark.parametrize("edge", [False, True], ids=["uniform", "edge"])
@pytest.mark.parametrize("which", [0, 1], ids=["form1", "form2"])
@pytest.mark.parametrize("shape,forms", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 8 else None)
def test_conv1_limb_result_whole_buffer(eng, shape, forms, which, edge):
    E, ca = eng
    x, w, bias, want, limb = case(shape, edge)
    got = run(E, ca, shape, x, w, bias, which + 1, forms[which], ca.NTTLC)
    check_limb(got, limb, (shape, which + 1, edge))
    rows = run(E, ca, shape, x, w, bias, which + 1, forms[which], ca.NTT)
    assert np.array_equal(rows.view(np.uint64), want.reshape(-1)), (shape, which + 1, edge, "canonical residues")


def test_conv1_limb_result_sub_batches(eng, request):
    """conv1_pass_bytes at a third of the whole work space: three images in passes of one (b0 = 0, 1, 2 of the tensor), both forms, whole buffer"""
    E, ca = eng
    shape = (26, 26, 2, 2, 6, 6, 32, 3)
    xd, yd, xs, ys, xf, yf, nf, B = shape
    x, w, bias, want, limb = case(shape, False)
    request.addfinalizer(lambda: E.set_tuning("conv1_pass_bytes", 0))
    for form in (1, 2):
        E.set_tuning("conv1_form", form); E.set_tuning("conv1_pass_bytes", 0)
        whole = E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL1, ca.NTTLC)
        E.set_tuning("conv1_pass_bytes", whole // 3)
        assert E.conv2d_forms_work_bytes(B, 1, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL1, ca.NTTLC) < whole // 2
        check_limb(run(E, ca, shape, x, w, bias, form, form, ca.NTTLC), limb, (shape, form, "sub-batches"))
        rows = run(E, ca, shape, x, w, bias, form, form, ca.NTT)
        assert np.array_equal(rows.view(np.uint64), want.reshape(-1)), (form, "canonical residues in sub-batches")
