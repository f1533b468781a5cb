"""The polynomial activation layer `poly NAME c2 c1 c0` (c2 x^2 + c1 x + c0; INTEGRATION.md "Network descriptions"), CPU side: both hosts parse the line to the
same float32 coefficients, print the same canonical form and refuse the same malformed lines; the float forward of the C++ host walks it; and the Evaluator
sequence that DEFINES the layer -- relinearize(square(x)), multiply_plain by encode(c2), add multiply_plain(x, encode(c1)), add_plain encode(c0) -- decodes to
the polynomial and leaves noise budget, on the CPU oracle.  No GPU work."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")
MODELS = os.path.join(ROOT, "tests", "golden", "models")
ACT = os.path.join(ROOT, "tests", "golden", "activations")
FILES = [os.path.join(ACT, "approx_poly.net"), os.path.join(ACT, "approx_poly_square.net")]
H5 = os.path.join(MODELS, "ApproxPlainModel.h5")
TRIPLES = [(1, 0, 0), (0.25, 0.5, 0.125), (0.1997, 0.5002, 0.1992), (-0.125, -1.5, 2)]


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(DRIVER):
        if not os.path.exists(os.path.join(ROOT, "crcnn_amd", "lib", "libcrcnn_hip.so")):
            pytest.fail("libcrcnn_hip.so is missing: run __graft_entry__.build()")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crcnn_amd", "host")])
    return DRIVER


def cpp_describe(driver, what, h5=None):
    return subprocess.run([driver, "describe", what] + ([h5] if h5 else []), capture_output=True, text=True)


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


@pytest.mark.parametrize("path", FILES, ids=[stem(f) for f in FILES])
def test_cpp_and_python_print_the_same_canonical_form(driver, path, tmp_path):
    from crcnn_amd import netrun
    d = netrun.load_description(path, H5)
    want = netrun.format_description(d)
    for h5 in (None, H5):
        out = cpp_describe(driver, path, h5)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want
    # the round trip is exact in both hosts
    back = netrun.parse_description(want)
    assert list(back) == list(d) and back.threads == d.threads and netrun.format_description(back) == want
    canon = tmp_path / "canon.net"
    canon.write_text(want)
    out = cpp_describe(driver, str(canon))
    assert out.returncode == 0 and out.stdout == want
    # everything but the activation line is ApproxPlainModel
    ref = netrun.format_description(netrun.load_description("ApproxPlainModel")).splitlines()
    assert [l for l in want.splitlines() if not l.startswith("poly")] == [l for l in ref if not l.startswith("square")]


def test_poly_line_details():
    from crcnn_amd import netrun
    d = netrun.load_description(FILES[0])
    assert [k for k, _, _ in d] == ["conv", "avgpool", "bn", "conv", "poly", "avgpool", "bn", "fc", "fc"]
    kind, name, a = d[4]
    assert name == "act1" and d.threads[4] == 50
    # the coefficients are the float32 nearest to the decimal text, held as Python floats
    assert a == dict(c2=float(np.float32(0.1997)), c1=float(np.float32(0.5002)), c0=float(np.float32(0.1992)))
    assert a["c2"] != 0.1997                      # (0.1997 is no float32: the parse rounds)
    assert "poly act1 0.199699998 0.500199974 0.199200004 threads 50" in netrun.format_description(d)
    sq = netrun.load_description(FILES[1])
    assert sq[4][2] == dict(c2=1.0, c1=0.0, c0=0.0) and "poly act1 1 0 0 threads 50" in netrun.format_description(sq)
    # shapes unchanged; a poly layer may come first, and may be followed by anything a square may
    t = netrun.parse_description("input 2 4 4\npoly p -0.125 -1.5 2\npool q stride 2 2 window 2 2\nfc f 3\n")
    assert t[0] == ("poly", "p", dict(c2=-0.125, c1=-1.5, c0=2.0)) and t[1][2] == dict(xd=4, yd=4, zd=2, xs=2, ys=2, xf=2, yf=2) and t.threads[0] is None


# decimal texts whose nearest double and nearest float32 differ in interesting ways: plain decimals, exponents, a halfway-looking case, denormal-range and signs
NUMBERS = ["0.1997", "0.5002", "0.1992", "1", "-1.5", "2", "0.1", "1e-3", "-2.5E2", "3.4028234e38", "1.17549435e-38", "1e-45", "16777217", "0.30000001192092896",
           ".5", "5.", "+0.25", "-0", "1.00000005960464477539"]


def test_both_hosts_parse_the_same_float32(driver, tmp_path):
    from crcnn_amd import netrun
    lines = ["input 1 4 4"] + [f"poly p{i} {t} {t} {t}" for i, t in enumerate(NUMBERS) if float(np.float32(float(t))) != 0.0]
    # (a zero is allowed for c1 and c0 only)
    lines += [f"poly z{i} 1 {t} {t}" for i, t in enumerate(NUMBERS) if float(np.float32(float(t))) == 0.0]
    text = "\n".join(lines) + "\n"
    d = netrun.parse_description(text)
    for (kind, name, a), ln in zip(d, lines[1:]):
        tok = ln.split()
        for key, t in zip(("c2", "c1", "c0"), tok[2:]):
            assert a[key] == float(np.float32(float(t))) and np.float32(a[key]) == np.float32(float(t)), (ln, a)
    want = netrun.format_description(d)
    path = tmp_path / "numbers.net"
    path.write_text(text)
    out = cpp_describe(driver, str(path))
    assert out.returncode == 0, out.stderr
    assert out.stdout == want
    # %.9g of a float32 reads back as that float32: the canonical text is a fixed point of both hosts
    assert netrun.format_description(netrun.parse_description(want)) == want
    for ln in want.splitlines()[1:]:
        for t in ln.split()[2:5]:
            assert np.float32(float(t)) == np.float32(float("%.9g" % np.float32(float(t))))


GOOD = "input 1 28 28\nconv pool1_features.conv1 stride 2 2 filter 5 5 filters 20\n"
MALFORMED = {
    "no-numbers": (GOOD + "poly act1\n", 3),
    "two-numbers": (GOOD + "poly act1 0.5 0.25\n", 3),
    "four-numbers": (GOOD + "poly act1 0.5 0.25 1 2\n", 3),
    "not-a-number": (GOOD + "poly act1 0.5 x 1\n", 3),
    "hex-float": (GOOD + "poly act1 0x1p-2 0 0\n", 3),
    "underscore": (GOOD + "poly act1 1_0 0 0\n", 3),
    "c2-zero": (GOOD + "poly act1 0 1 0.5\n", 3),
    "c2-negative-zero": (GOOD + "poly act1 -0.0 1 0.5\n", 3),
    "c2-rounds-to-zero": (GOOD + "poly act1 1e-60 1 0.5\n", 3),
    "nan": (GOOD + "poly act1 nan 1 0.5\n", 3),
    "nan-in-c0": (GOOD + "\npoly act1 1 1 NaN\n", 4),
    "inf": (GOOD + "poly act1 1 inf 0\n", 3),
    "overflows-float32": (GOOD + "poly act1 1 1e39 0\n", 3),
    "missing-name": (GOOD + "poly\n", 3),
    "threads-without-count": (GOOD + "poly act1 1 0 0 threads\n", 3),
    "after-dense": (GOOD + "fc f 10\npoly act1 1 0 0\n", 4),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_poly_lines_are_rejected_with_their_line(driver, case, tmp_path):
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


def float_forward(desc, W, img):
    """float64 forward of a description with a poly layer (the forward of tests/test_topology_cpu.py plus the polynomial, on the float32 coefficients)"""
    x = img.astype(np.float64).reshape(desc.input_shape)
    for kind, name, a in desc:
        if kind == "conv":
            w = W[name + ".weight"].astype(np.float64).reshape(a["nf"], a["zd"], a["xf"], a["yf"]); b = W[name + ".bias"].astype(np.float64)
            xo, yo = (a["xd"] - a["xf"]) // a["xs"] + 1, (a["yd"] - a["yf"]) // a["ys"] + 1
            y = np.zeros((a["nf"], xo, yo))
            for i in range(xo):
                for j in range(yo):
                    y[:, i, j] = (w * x[None, :, i * a["xs"]:i * a["xs"] + a["xf"], j * a["ys"]:j * a["ys"] + a["yf"]]).sum(axis=(1, 2, 3)) + b
            x = y
        elif kind == "avgpool":
            xo, yo = (a["xd"] - a["xf"]) // a["xs"] + 1, (a["yd"] - a["yf"]) // a["ys"] + 1
            y = np.zeros((a["zd"], xo, yo))
            for i in range(xo):
                for j in range(yo):
                    y[:, i, j] = x[:, i * a["xs"]:i * a["xs"] + a["xf"], j * a["ys"]:j * a["ys"] + a["yf"]].sum(axis=(1, 2))
            x = y / (a["xf"] * a["yf"])
        elif kind == "bn":
            x = (x - W[name + ".running_mean"].astype(np.float64)[:, None, None]) / np.sqrt(W[name + ".running_var"].astype(np.float64) + 1e-5)[:, None, None]
        elif kind == "square":
            x = x * x
        elif kind == "poly":
            x = a["c2"] * x * x + a["c1"] * x + a["c0"]
        elif kind == "fc":
            x = (W[name + ".weight"].astype(np.float64).reshape(a["out_dim"], a["in_dim"]) @ x.reshape(-1) + W[name + ".bias"].astype(np.float64)).reshape(1, -1, 1)
        else:
            raise AssertionError(kind)
    return x.reshape(-1)


def run_labels(driver, model, images):
    out = subprocess.run([driver, "labels", model, H5, images], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    labels = [int(l.split()[2]) for l in out.stdout.splitlines() if l.startswith("label")]
    logits = np.array([[float(v) for v in l.split()[2:]] for l in out.stdout.splitlines() if l.startswith("logits")])
    return labels, logits


@pytest.mark.parametrize("path", FILES, ids=[stem(f) for f in FILES])
def test_plain_model_forward_walks_the_poly_layer(driver, path, tmp_path):
    """`test_host labels` (plainModelForward, float32 activations) against a float64 forward written here, within 1e-3 of the largest logit: the bound
    tests/test_topology_cpu.py uses for the same comparison (float32 storage rounds by 6e-8 per value; ten layers amplify that by far less than 10^4)"""
    from crcnn_amd import binding, netrun, synth
    imgs = np.stack([synth.normalize(synth.synth_image(i)).reshape(-1) for i in range(6)]).astype(np.float32)
    imgs.tofile(str(tmp_path / "images.f32"))
    W = {nm: binding.h5_read(H5, nm) for nm in binding.h5_list(H5) if not nm.endswith("num_batches_tracked")}
    desc = netrun.load_description(path, H5)
    want = [float_forward(desc, W, im) for im in imgs]
    labels, logits = run_labels(driver, path, str(tmp_path / "images.f32"))
    assert labels == [int(np.argmax(v)) for v in want]
    assert logits.shape == (len(imgs), 10)
    for g_, w_ in zip(logits, want):
        assert np.abs(g_ - w_).max() <= 1e-3 * np.abs(w_).max(), (path, g_, w_)
    if stem(path) == "approx_poly_square":
        # 1 x^2 + 0 x + 0 is the Square layer: ApproxPlainModel's labels, and its float32 logits to the last bit
        ref_labels, ref_logits = run_labels(driver, "ApproxPlainModel", str(tmp_path / "images.f32"))
        assert labels == ref_labels and np.array_equal(logits, ref_logits)
        assert len(set(labels)) > 1
    else:
        # the fitted polynomial is another function than x^2: the logits must move by more than the comparison's bound
        _, ref_logits = run_labels(driver, "ApproxPlainModel", str(tmp_path / "images.f32"))
        assert np.abs(logits - ref_logits).max() > 1e-2 * np.abs(ref_logits).max()


def oracle_poly(O, x, evk, c2, c1, c0):
    """the layer's definition, per ciphertext in coefficient form: the Evaluator sequence of INTEGRATION.md on float32 coefficients"""
    c2, c1, c0 = (float(np.float32(v)) for v in (c2, c1, c0))
    s = O.relinearize(O.square(x), evk)
    if c2 != 1.0:
        s = O.multiply_plain(s, O.encode(c2)[0])
    if c1 != 0.0:
        s = O.add(s, O.multiply_plain(x, O.encode(c1)[0]))
    if c0 != 0.0:
        s = O.add_plain(s, O.encode(c0)[0])
    return s


def test_the_defining_sequence_decodes_to_the_polynomial():
    """(4096, SEAL's two default moduli, t = 2^29), keygen seed 1, evaluation-key seed 2, encryption seed 7: every (input, triple) decodes to
    c2 x^2 + c1 x + c0 within 1e-4 (the bound of tests/test_abi_cpu.py for decoded values) and keeps at least 10 bits of noise budget.  This pins the
    definition the device code is compared with bit for bit (tests/test_gpu_poly.py), not the device code"""
    from oracle import orc
    n, q, t = 4096, [0x7fffffff380001, 0x3fffffff000001], 1 << 29
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(1)
    evk = O.gen_evk(2, sk)
    xs = np.array([0, 1, -2.75, 3.1415927, 17.5, -0.0625], dtype=np.float32)
    cts = O.encrypt_many(pk, O.encode_many(xs), 7)
    worst, budget = 0.0, 1 << 30
    for c2, c1, c0 in TRIPLES:
        f2, f1, f0 = (float(np.float32(v)) for v in (c2, c1, c0))
        for x, ct in zip(xs, cts):
            s = oracle_poly(O, ct, evk, c2, c1, c0)
            want = f2 * float(x) * float(x) + f1 * float(x) + f0
            got = O.decrypt_value(sk, s)
            print(f"poly {c2} {c1} {c0} at x = {float(x)}: decoded {got!r}, expected {want!r}, budget {O.noise_budget(sk, s)}")
            worst = max(worst, abs(got - want)); budget = min(budget, O.noise_budget(sk, s))
            assert abs(got - want) <= 1e-4, (c2, c1, c0, float(x), got, want)
            assert O.noise_budget(sk, s) >= 10, (c2, c1, c0, float(x), O.noise_budget(sk, s))
            if (c2, c1, c0) == (1, 0, 0):
                assert np.array_equal(s, O.relinearize(O.square(ct), evk))
    print("largest decode error", worst, "smallest budget", budget)
