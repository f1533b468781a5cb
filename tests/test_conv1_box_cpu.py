"""The box of the one-channel convolution (crc_conv2d_box_forms, crc_plan_conv1_box) without a GPU.

The reduction helper against 128-bit arithmetic (tests/cpp/box_sum_check.cpp).

The algebra on the CPU oracle at n = 256, k = 2: a convolution with a window sum folded into its weights (W * box, the bias times the box's size) equals the
base convolution of the window sums of its input, ciphertext for ciphertext -- 2 x 2, 1 x 2 and 2 x 1 boxes at the layer's stride, and a 3 x 3 / 1 base window.

The plan query on host-only engines: yes for PlainModelTiny's pair, no under conv1_box = 0, for a base window of more than 40 taps, for 17-20 filters and for a
layer that is not one-channel; the fused plan keeps the geometry of the map the layer computes."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import crcnn_amd as ca
from benchkit import geometry
from netcommon import load_net_golden
from oracle import orc
from test_hoist_pool_cpu import bias_rows, conv_rows, fold_pool, host_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_sum_reduction_against_int128():
    exe = os.path.join(tempfile.mkdtemp(), "box_sum_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "box_sum_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    assert int(out.split()[1]) > 400_000


# ---- the algebra ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setting():
    g = load_net_golden("tiny256")
    O = orc.Oracle(g["n"], g["q"], g["t"])
    assert O.n == 256 and O.k == 2
    sk, pk = O.keygen(41)
    rng = np.random.RandomState(6)
    x = O.encrypt_many(pk, O.encode_many(rng.uniform(-1, 1, size=(1, 16, 16)).astype(np.float32)).reshape(1, 16, 16, O.n), 900)
    enc = lambda a: O.encode_many(np.asarray(a, dtype=np.float32)).reshape(np.shape(a) + (O.n,))
    return O, rng, enc, x


def box_sum(O, x, bxf, byf, xs, ys):
    """x [1][xd][yd][2][k][n] ciphertexts -> the window sums (r, c) = sum of x(r + a xs, c + b ys), a < bxf, b < byf, mod q"""
    xd, yd = x.shape[1:3]
    xdo, ydo = xd - (bxf - 1) * xs, yd - (byf - 1) * ys
    acc = np.zeros((1, xdo, ydo) + x.shape[3:], dtype=object)
    for a in range(bxf):
        for b in range(byf):
            acc += x[:, a * xs:a * xs + xdo, b * ys:b * ys + ydo].astype(object)
    out = np.empty(acc.shape, dtype=np.uint64)
    for i, q in enumerate(O.q):
        out[..., i, :] = (acc[..., i, :] % q).astype(np.uint64)
    return out


@pytest.mark.parametrize("xf,xs,bxf,byf", [(6, 2, 2, 2), (6, 2, 1, 2), (6, 2, 2, 1), (3, 1, 2, 2)], ids=["6x6s2-box2x2", "6x6s2-box1x2", "6x6s2-box2x1", "3x3s1-box2x2"])
def test_boxed_input_equals_enlarged_window(setting, xf, xs, bxf, byf):
    O, rng, enc, x = setting
    w, b = O.plains_to_ntt(enc(rng.normal(0, 0.3, size=(3, 1, xf, xf)))), bias_rows(O, enc(rng.normal(0, 0.1, size=3)))
    w_big, b_big = fold_pool(O, w, b, xs, xs, bxf, byf, None)
    assert w_big.shape[2:4] == ((bxf - 1) * xs + xf, (byf - 1) * xs + xf)
    for i, q in enumerate(O.q):
        assert np.array_equal(b_big[:, i], ((b[:, i].astype(object) * (bxf * byf)) % q).astype(np.uint64))
    want = conv_rows(O, x, w_big, b_big, xs, xs)
    got = conv_rows(O, box_sum(O, x, bxf, byf, xs, xs), w, b_big, xs, xs)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------------
TINY_BASE = (1, 28, 28, 2, 2, 6, 6, 32)


def test_plan_boxes_tiny_conv1(monkeypatch):
    T = host_engine("tiny4096")
    assert T.limb_conv1_box_supported(*TINY_BASE, 2, 2) is True
    assert T.plan_conv1_box(*TINY_BASE, 2, 2, 128) is True
    assert T.plan_conv1_box(*TINY_BASE, 2, 2, 0) is True
    # the fused plan reports the map the layer computes, with or without the box
    geo = lambda a: tuple(a[k] for k in ("zd", "xd", "yd", "xs", "ys", "xf", "yf", "nf"))
    plan = geometry.fused_plan(T, "PlainModelTiny")
    assert plan[0][1] == "pool1_features.conv1+pool1" and geo(plan[0][2]) == (1, 28, 28, 2, 2, 8, 8, 32) and plan[0][4] == (32, 11, 11)
    T.close()
    # conv1_box = 0 (a context reads its tuning from the environment when it is made)
    monkeypatch.setenv("CRC_CONV1_BOX", "0")
    T0 = host_engine("tiny4096")
    assert T0.plan_conv1_box(*TINY_BASE, 2, 2, 128) is False
    assert T0.limb_conv1_box_supported(*TINY_BASE, 2, 2) is True
    plan0 = geometry.fused_plan(T0, "PlainModelTiny")
    assert [(pl[1], dict(pl[2]), pl[4]) for pl in plan0] == [(pl[1], dict(pl[2]), pl[4]) for pl in plan]
    T0.close()


def test_plan_refuses():
    T = host_engine("tiny4096")
    assert T.plan_conv1_box(*TINY_BASE, 2, 2, 128, matrix_cores=False) is False
    assert T.plan_conv1_box(*TINY_BASE, 1, 1, 128) is False                              # no box at all
    # a base window of more than 40 taps runs on the plane-major kernel, which takes no box
    assert T.plan_mac(1, 28, 28, 2, 2, 7, 7, 32, 128) == ca.NTTL1 and T.plan_mac(1, 26, 26, 2, 2, 7, 7, 32, 128) == ca.NTTL1
    assert T.plan_conv1_box(1, 28, 28, 2, 2, 7, 7, 32, 2, 2, 128) is False
    assert T.limb_conv1_box_supported(1, 28, 28, 2, 2, 7, 7, 32, 2, 2) is False
    # 17-20 filters keep the plane-major kernel's packed second filter group
    for nf in (17, 20):
        assert T.plan_conv1_box(1, 28, 28, 2, 2, 6, 6, nf, 2, 2, 128) is False
    assert T.plan_conv1_box(1, 28, 28, 2, 2, 6, 6, 16, 2, 2, 128) is True
    # not a one-channel layer
    assert T.plan_conv1_box(2, 28, 28, 2, 2, 6, 6, 32, 2, 2, 128) is False
    assert T.plan_conv1_box(32, 12, 12, 1, 1, 5, 5, 64, 2, 2, 128) is False
    # more than nine terms
    assert T.limb_conv1_box_supported(1, 14, 14, 1, 1, 3, 3, 32, 3, 3) is True
    assert T.limb_conv1_box_supported(1, 14, 14, 1, 1, 3, 3, 32, 2, 5) is False
    # the work space of a boxed layer is the summed image's
    assert T.conv2d_box_forms_work_bytes(4, *TINY_BASE, 2, 2, ca.NTT, ca.NTTL1, ca.NTTLC) == T.conv2d_forms_work_bytes(4, 1, 26, 26, 2, 2, 6, 6, 32, ca.NTT, ca.NTTL1, ca.NTTLC)
    assert T.conv2d_box_forms_work_bytes(4, *TINY_BASE, 1, 1, ca.NTT, ca.NTTL1, ca.NTT) == T.conv2d_forms_work_bytes(4, *TINY_BASE, ca.NTT, ca.NTTL1, ca.NTT)
    assert T.conv2d_box_forms_work_bytes(4, 1, 28, 28, 2, 2, 7, 7, 32, 2, 2, ca.NTT, ca.NTTL1, ca.NTT) == 0
    T.close()
