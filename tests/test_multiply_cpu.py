"""The ciphertext x ciphertext multiply and the `poly3` layer, CPU side.  tests/bfv_multiply_model.py -- Evaluator::multiply restated in Python integers over
SEAL's own auxiliary base -- is pinned to the reference by SEAL's recorded squares; its products commute, decrypt to the product of the plaintexts, and carry the
defining sequence of `poly3 NAME c3 c2 c1 c0` to the cubic; both hosts parse, print and refuse the line alike.  No GPU work."""
import glob
import os
import subprocess

import numpy as np
import pytest

from bfv_multiply_model import MultiplyModel, golden_pairs, golden_products, plain_negacyclic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DRIVER = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")
SETS = sorted(glob.glob(os.path.join(GOLD, "ops_*.npz")))
CUBIC = os.path.join(GOLD, "activations", "cubic.net")
QUADS = [(1, 0, 0, 0), (-0.004, 0, 0.197, 0.5), (0.125, 0.25, 0.5, -1)]


def load(path):
    from oracle import orc
    g = dict(np.load(path))
    return os.path.basename(path), g, orc.Oracle(int(g["n"]), [int(v) for v in g["q"]], int(g["t"]))


@pytest.mark.parametrize("path", SETS, ids=[os.path.basename(s)[:-4] for s in SETS])
def test_model_of_x_x_is_the_reference_square(path):
    """model(x, x) == ref_sq, SEAL's own Evaluator::square output, and == Oracle.square, for every ciphertext of the set"""
    name, g, O = load(path)
    M = MultiplyModel(O)
    for i, x in enumerate(g["ct_in"]):
        got = M.multiply(x, x)
        assert np.array_equal(got, g["ref_sq"][i]), (name, i)
        assert np.array_equal(got, O.square(x)), (name, i)


@pytest.mark.parametrize("path", SETS, ids=[os.path.basename(s)[:-4] for s in SETS])
def test_model_commutes(path):
    name, g, O = load(path)
    x, y, _, _ = golden_pairs(g, O)
    assert len(x) >= 2
    prod = golden_products(name, g, O)
    M = MultiplyModel(O)
    for i in range(len(x)):
        assert not np.array_equal(x[i], y[i])
        assert np.array_equal(M.multiply(y[i], x[i]), prod[i]), (name, i)


def test_products_decrypt_to_the_product_of_the_plaintexts():
    """on every set whose ref_budget_relin (SEAL's own record after one multiplication) is at least 10 bits: decrypt(relinearize(model(x, y))) is the negacyclic
    product of the two plaintext polynomials mod t, coefficient for coefficient.  At least three of the six sets qualify"""
    ran = 0
    for path in SETS:
        name, g, O = load(path)
        if int(np.min(g["ref_budget_relin"])) < 10:
            continue
        x, y, mx, my = golden_pairs(g, O)
        prod = golden_products(name, g, O)
        for i in range(len(x)):
            r = O.relinearize(prod[i], g["evk"])
            assert np.array_equal(O.decrypt(g["sk"], r), plain_negacyclic(mx[i], my[i], int(g["t"]))), (name, i)
            assert O.noise_budget(g["sk"], r) > 0
        ran += 1
    assert ran >= 3, ran


def poly3_sequence(O, M, evk, x, quad):
    """the layer's definition, per ciphertext in coefficient form, on float32 coefficients"""
    c3, c2, c1, c0 = (float(np.float32(v)) for v in quad)
    s = O.relinearize(O.square(x), evk)
    r = O.relinearize(M.multiply(s, x), evk)
    if c3 != 1.0:
        r = O.multiply_plain(r, O.encode(c3)[0])
    if c2 != 0.0:
        r = O.add(r, O.multiply_plain(s, O.encode(c2)[0]))
    if c1 != 0.0:
        r = O.add(r, O.multiply_plain(x, O.encode(c1)[0]))
    if c0 != 0.0:
        r = O.add_plain(r, O.encode(c0)[0])
    return r


def test_the_defining_sequence_of_poly3_decodes_to_the_cubic():
    """(4096, SEAL's two default moduli, t = 2^16): every (input, quadruple) decodes to the cubic of the float32 coefficients within 1e-4 and keeps at least 10
    bits of noise budget -- the two figures tests/test_gpu_poly.py uses for `poly`; (1, 0, 0, 0) is x^3"""
    from oracle import orc
    n, q, t = 4096, [0x7fffffff380001, 0x3fffffff000001], 1 << 16
    O = orc.Oracle(n, q, t)
    M = MultiplyModel(O)
    sk, pk = O.keygen(1)
    evk = O.gen_evk(2, sk)
    xs = np.array([1.5, -2.75], dtype=np.float32)
    cts = O.encrypt_many(pk, O.encode_many(xs), 7)
    for quad in QUADS:
        f3, f2, f1, f0 = (float(np.float32(v)) for v in quad)
        for x, ct in zip(xs, cts):
            r = poly3_sequence(O, M, evk, ct, quad)
            v = float(x)
            want = f3 * v ** 3 + f2 * v * v + f1 * v + f0
            got, budget = O.decrypt_value(sk, r), O.noise_budget(sk, r)
            print(f"poly3 {quad} at x = {v}: decoded {got!r}, expected {want!r}, budget {budget}")
            assert abs(got - want) <= 1e-4, (quad, v, got, want)
            assert budget >= 10, (quad, v, budget)
            if quad == (1, 0, 0, 0):
                assert abs(got - v ** 3) <= 1e-4


# ---- the description line in both hosts -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(DRIVER):
        if not os.path.exists(os.path.join(ROOT, "crcnn_amd", "lib", "libcrcnn_hip.so")):
            pytest.fail("libcrcnn_hip.so is missing: run __graft_entry__.build()")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crcnn_amd", "host")])
    return DRIVER


def cpp_describe(driver, what):
    return subprocess.run([driver, "describe", what], capture_output=True, text=True)


NUMBERS = ["0.1997", "1", "-1.5", "1e-3", "-2.5E2", "3.4028234e38", "1e-45", "16777217", ".5", "5.", "+0.25"]


def test_cpp_and_python_print_the_same_canonical_form(driver, tmp_path):
    from crcnn_amd import netrun
    d = netrun.load_description(CUBIC)
    assert [k for k, _, _ in d] == ["poly3", "avgpool"] and d.input_shape == (2, 3, 3)
    assert d[0] == ("poly3", "act", dict(c3=float(np.float32(-0.004)), c2=0.0, c1=float(np.float32(0.197)), c0=0.5))
    want = netrun.format_description(d)
    assert want == "input 2 3 3\npoly3 act -0.00400000019 0 0.196999997 0.5\navgpool p stride 1 1 window 2 2\n"
    out = cpp_describe(driver, CUBIC)
    assert out.returncode == 0, out.stderr
    assert out.stdout == want
    # the round trip is exact in both hosts
    back = netrun.parse_description(want)
    assert list(back) == list(d) and back.threads == d.threads and netrun.format_description(back) == want
    canon = tmp_path / "canon.net"
    canon.write_text(want)
    out = cpp_describe(driver, str(canon))
    assert out.returncode == 0 and out.stdout == want
    # float32 rounding and %.9g printing as on the poly line, `threads` included
    lines = ["input 1 4 4"] + [f"poly3 p{i} {t} {t} 0 {t} threads {i + 2}" for i, t in enumerate(NUMBERS)]
    text = "\n".join(lines) + "\n"
    d = netrun.parse_description(text)
    for (kind, name, a), ln in zip(d, lines[1:]):
        t = ln.split()[2]
        assert kind == "poly3" and a == dict(c3=float(np.float32(float(t))), c2=float(np.float32(float(t))), c1=0.0, c0=float(np.float32(float(t))))
    want = netrun.format_description(d)
    path = tmp_path / "numbers.net"
    path.write_text(text)
    out = cpp_describe(driver, str(path))
    assert out.returncode == 0, out.stderr
    assert out.stdout == want and netrun.format_description(netrun.parse_description(want)) == want


GOOD = "input 1 28 28\nconv pool1_features.conv1 stride 2 2 filter 5 5 filters 20\n"
MALFORMED = {
    "three-numbers": (GOOD + "poly3 act1 0.5 0.25 1\n", 3),
    "five-numbers": (GOOD + "poly3 act1 0.5 0.25 1 2 3\n", 3),
    "c3-zero": (GOOD + "poly3 act1 0 1 1 0.5\n", 3),
    "c3-negative-zero": (GOOD + "poly3 act1 -0.0 1 1 0.5\n", 3),
    "c3-rounds-to-zero": (GOOD + "poly3 act1 1e-60 1 1 0.5\n", 3),
    "nan": (GOOD + "poly3 act1 nan 1 1 0.5\n", 3),
    "nan-in-c0": (GOOD + "\npoly3 act1 1 1 1 NaN\n", 4),
    "inf": (GOOD + "poly3 act1 1 1 inf 0\n", 3),
    "overflows-float32": (GOOD + "poly3 act1 1 1e39 0 0\n", 3),
    "hex-float": (GOOD + "poly3 act1 0x1p-2 0 0 0\n", 3),
    "not-a-number": (GOOD + "poly3 act1 0.5 x 1 1\n", 3),
    "missing-name": (GOOD + "poly3\n", 3),
    "threads-without-count": (GOOD + "poly3 act1 1 0 0 0 threads\n", 3),
    "after-dense": (GOOD + "fc f 10\npoly3 act1 1 0 0 0\n", 4),
    "poly-with-four-numbers": (GOOD + "poly act1 0.5 0.25 1 2\n", 3),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_poly3_lines_are_rejected_with_their_line(driver, case, tmp_path):
    from crcnn_amd import netrun
    text, line = MALFORMED[case]
    path = tmp_path / "bad.net"
    path.write_text(text)
    with pytest.raises(ValueError, match=rf"^line {line}: ") as err:
        netrun.load_description(str(path))
    out = cpp_describe(driver, str(path))
    assert out.returncode == 10 and out.stdout == "", (out.stdout, out.stderr)
    assert out.stderr.startswith(f"exception: line {line}: "), out.stderr
    # the same message from both hosts
    assert out.stderr.strip() == "exception: " + str(err.value), (out.stderr, str(err.value))
