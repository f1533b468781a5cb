"""Every entry point that carves its work space stays inside what its crc_*_work_bytes function reports.  Each call runs on the middle of a buffer
[4096 guard bytes][W = the size function's answer under the call's tuning][4096 guard bytes] filled with 0xA5 -- with d_work at the first byte behind the front
guard, then 8 bytes further (an unaligned pointer, which the entry points accept by design; aligned up, the work space then ends exactly at the back guard) --
and must leave both guards as they were and write the result of the same call on a separate, generous, zero-filled work buffer.  The results themselves are
pinned to the oracle by the other GPU tests; this one pins the bounds.  A wrong layout shows as a changed guard or a changed result, not as a fault."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
Q = [0x7fffffff380001, 0x3fffffff000001]
GUARD, FILL = 4096, 0xA5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_n256_k2_t20.npz")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def make_engine(request, n):
    import crcnn_amd as ca
    E = ca.Engine(n, Q, 1 << 20, device=0)

    def restore():
        E.set_tuning("sq_chunk", 0); E.set_tuning("conv1_pass_bytes", 0)
        E.close()
    request.addfinalizer(restore)
    return E, ca


@pytest.fixture(scope="module")
def eng256(request):
    return make_engine(request, 256)


@pytest.fixture(scope="module")
def eng1024(request):
    return make_engine(request, 1024)


def residues(torch, E, rows, seed):
    """[rows][k][n] uniform residues on the device: ciphertext polynomials, weights and bias rows alike"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    out = torch.empty((rows, E.k, E.n), dtype=torch.int64, device="cuda")
    for i, q in enumerate(E.q):
        out[:, i] = torch.randint(0, int(q), (rows, E.n), dtype=torch.int64, device="cuda", generator=g)
    return out


def check_bounds(torch, E, W, call, out):
    """call(d_work) enqueues the entry point; out: the tensor it writes"""
    assert W > 0

    def run(d_work):
        out.zero_(); torch.cuda.synchronize()
        call(d_work)
        E.sync(); torch.cuda.synchronize()
        return out.clone()
    spacious = torch.zeros(2 * W + (1 << 20), dtype=torch.uint8, device="cuda")
    want = run(spacious.data_ptr())
    for shift in (0, 8):
        buf = torch.full((GUARD + W + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        got = run(buf.data_ptr() + GUARD + shift)
        assert bool((buf[:GUARD] == FILL).all()), ("write in front of the work space", shift)
        assert bool((buf[GUARD + W:] == FILL).all()), ("write behind the work space", shift)
        assert torch.equal(got, want), ("result depends on the work buffer", shift)


# ---- flat activations: 5 ciphertexts, one pass (sq_chunk 0) and three passes of 2, 2, 1 (sq_chunk 2) -----------------------------------------------------------
@pytest.fixture(scope="module")
def flat(torch, eng256):
    E, ca = eng256
    evk = torch.from_numpy(np.load(GOLD)["evk"].view(np.int64)).cuda()
    return dict(x=residues(torch, E, 5 * 2, 1), y=residues(torch, E, 5 * 2, 2), evk=evk, out=torch.empty((5 * 2, E.k, E.n), dtype=torch.int64, device="cuda"),
                p2=E.poly2_rows(0.25, 0.5, 0.125), p3=E.poly3_rows(0.5, 0.25, 0.5, 0.125))


@pytest.mark.parametrize("sq_chunk", [0, 2])
@pytest.mark.parametrize("forms", ["coeff", "ntt"])
@pytest.mark.parametrize("op", ["square_relin", "poly2_relin", "multiply_relin", "poly3_relin"])
def test_flat_activation_stays_inside_its_work_space(torch, eng256, flat, op, forms, sq_chunk):
    E, ca = eng256
    f = ca.NTT if forms == "ntt" else ca.COEFF
    E.set_tuning("sq_chunk", sq_chunk)
    x, y, evk, out = (flat[k].data_ptr() for k in ("x", "y", "evk", "out"))
    assert all(r is not None for r in flat["p2"] + flat["p3"])
    if op == "square_relin":
        W, call = E.square_relin_work_bytes(5), lambda w: E.square_relin(x, 5, evk, out, w, in_form=f, out_form=f)
    elif op == "poly2_relin":
        W, call = E.poly2_relin_work_bytes(5), lambda w: E.poly2_relin(x, 5, evk, *flat["p2"], out, w, in_form=f, out_form=f)
    elif op == "multiply_relin":
        W, call = E.multiply_relin_work_bytes(5), lambda w: E.multiply_relin(x, y, 5, evk, out, w, in_form=f, out_form=f)
    else:
        W, call = E.poly3_relin_work_bytes(5), lambda w: E.poly3_relin(x, 5, evk, *flat["p3"], out, w, in_form=f, out_form=f)
    check_bounds(torch, E, W, call, flat["out"])


# ---- pooled activations: two 4 x 4 planes, window 2 x 2 stride 1; both planes in one pass (sq_chunk 0) and one plane per pass (sq_chunk 16) --------------------
@pytest.mark.parametrize("sq_chunk", [0, 16])
@pytest.mark.parametrize("in_form", ["coeff", "ntt"])
@pytest.mark.parametrize("op", ["square_pool_relin", "poly2_pool_relin"])
def test_pooled_activation_stays_inside_its_work_space(torch, eng256, flat, op, in_form, sq_chunk):
    E, ca = eng256
    fin = ca.NTT if in_form == "ntt" else ca.COEFF
    geom = (1, 2, 4, 4, 1, 1, 2, 2)                 # B, zd, xd, yd, xs, ys, xf, yf
    assert E.square_pool_relin_supported(2, 2) and E.poly2_pool_relin_supported(2, 2)
    E.set_tuning("sq_chunk", sq_chunk)
    x = residues(torch, E, 32 * 2, 3)
    out = torch.empty((2 * 3 * 3 * 2, E.k, E.n), dtype=torch.int64, device="cuda")
    evk = flat["evk"].data_ptr()
    if op == "square_pool_relin":
        W, call = E.square_pool_relin_work_bytes(*geom), lambda w: E.square_pool_relin(x.data_ptr(), *geom, evk, out.data_ptr(), w, in_form=fin, out_form=ca.NTT)
    else:
        rows = E.poly2_rows(0.25, 0.5, 0.125, window=4)
        assert all(r is not None for r in rows)
        W, call = E.poly2_pool_relin_work_bytes(*geom), lambda w: E.poly2_pool_relin(x.data_ptr(), *geom, evk, *rows, out.data_ptr(), w, in_form=fin, out_form=ca.NTT)
    check_bounds(torch, E, W, call, out)


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------------------------------
def conv_case(torch, E, ca, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, w_form, out_form, seed, pass_third=False):
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    x = residues(torch, E, B * zd * xd * yd * 2, seed); w = residues(torch, E, nf * zd * xf * yf, seed + 1); bias = residues(torch, E, nf, seed + 2)
    d_w = w
    if w_form == ca.NTTL:
        d_w = torch.zeros(E.limb_weights_bytes(nf, zd, xf, yf), dtype=torch.uint8, device="cuda")
        E.limb_pack_weights(w.data_ptr(), nf, zd, xf, yf, d_w.data_ptr())
    elif w_form == ca.NTTL1:
        assert E.limb_conv1_supported(zd, xd, yd, xs, ys, xf, yf, nf)
        d_w = torch.zeros(E.limb_conv1_weights_bytes(), dtype=torch.uint8, device="cuda")
        E.limb_conv1_pack_weights(w.data_ptr(), nf, xf, yf, d_w.data_ptr())
    E.sync()
    args = (B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, w_form, out_form)
    if pass_third:                                  # several internal passes: the work space of a pass is a third of the whole batch's
        E.set_tuning("conv1_pass_bytes", 0)
        E.set_tuning("conv1_pass_bytes", E.conv2d_forms_work_bytes(*args) // 3)
    W = E.conv2d_forms_work_bytes(*args)
    out_bytes = E.limb_tensor_bytes(B, nf, xo, yo) if out_form == ca.NTTLC else B * nf * xo * yo * 2 * E.k * E.n * 8
    out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    check_bounds(torch, E, W, lambda d_work: E.conv2d(x.data_ptr(), d_w.data_ptr(), bias.data_ptr(), B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form,
                                                      out.data_ptr(), d_work, w_form=w_form), out)
    return W


def test_vector_alu_conv_stays_inside_its_work_space(torch, eng1024):
    E, ca = eng1024
    conv_case(torch, E, ca, 2, 2, 4, 4, 1, 1, 2, 2, 3, ca.COEFF, ca.NTT, ca.COEFF, 10)


def test_limb_gemm_conv_stays_inside_its_work_space(torch, eng1024):
    E, ca = eng1024
    conv_case(torch, E, ca, 1, 20, 5, 7, 2, 1, 3, 2, 50, ca.COEFF, ca.NTTL, ca.COEFF, 20)          # ragged: channel and filter padding, the flat limb form


@pytest.mark.parametrize("forms", ["coeff-to-ntt", "ntt-to-limb"])
def test_one_channel_conv_stays_inside_its_work_space(torch, eng1024, forms):
    E, ca = eng1024
    fin, fout = (ca.COEFF, ca.NTT) if forms == "coeff-to-ntt" else (ca.NTT, ca.NTTLC)
    try:
        E.set_tuning("conv1_pass_bytes", 0)
        whole = E.conv2d_forms_work_bytes(5, 1, 28, 28, 2, 2, 6, 6, 32, fin, ca.NTTL1, fout)
        W = conv_case(torch, E, ca, 5, 1, 28, 28, 2, 2, 6, 6, 32, fin, ca.NTTL1, fout, 30, pass_third=True)
        assert W < whole                            # the five images did take more than one pass
    finally:
        E.set_tuning("conv1_pass_bytes", 0)
