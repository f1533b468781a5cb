"""Network description files (INTEGRATION.md "Network descriptions"), CPU side: the Python parser (crcnn_amd/netrun.py) and the C++ one
(NetworkDescription in crcnn_amd/host, driven through `test_host describe` / `test_host labels`) read the same format, apply the same checks and print
the same canonical form; the three built-in descriptions are the three hard-coded topologies; the float forward walks a description.  No GPU work."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")
MODELS = os.path.join(ROOT, "tests", "golden", "models")
BUILTIN = ["PlainModelTiny", "ApproxPlainModel", "PlainModelWoPad"]
FILES = sorted(glob.glob(os.path.join(ROOT, "crcnn_amd", "models", "*.net")) + glob.glob(os.path.join(ROOT, "tests", "golden", "topologies", "*.net")))
# the model file whose weights a description's layers name
H5_OF = {"PlainModelTiny": "PlainModelTiny", "ApproxPlainModel": "ApproxPlainModel", "PlainModelWoPad": "PlainModelWoPad", "approx_padded": "ApproxPlainModel",
         "tiny_refresh": "PlainModelTiny"}


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(DRIVER):
        if not os.path.exists(os.path.join(ROOT, "crcnn_amd", "lib", "libcrcnn_hip.so")):
            pytest.fail("libcrcnn_hip.so is missing: run __graft_entry__.build()")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crcnn_amd", "host")])
    return DRIVER


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def h5_of(path):
    return os.path.join(MODELS, H5_OF[stem(path)] + ".h5")


def cpp_describe(driver, what, h5=None):
    return subprocess.run([driver, "describe", what] + ([h5] if h5 else []), capture_output=True, text=True)


def test_every_description_file_is_covered():
    assert len(FILES) >= 5 and all(stem(f) in H5_OF for f in FILES), FILES
    assert sorted(stem(f) for f in FILES if os.sep + "models" + os.sep in f and "golden" not in f) == sorted(BUILTIN)


@pytest.mark.parametrize("name", BUILTIN)
def test_builtin_descriptions_are_the_hard_coded_topologies(name):
    from crcnn_amd import netrun
    d = netrun.parse_description(open(os.path.join(netrun.MODELS_DIR, name + ".net")).read())
    assert list(d) == netrun.TOPOLOGIES[name]
    assert d.input_shape == (1, 28, 28) and d.layer_before_reenc == -1
    # the thread counts CnnBuilder::buildNetworkByName has always passed to the reference's constructors (printLayerStructure shows them)
    th = {"PlainModelTiny": [32, None, 64, None, 42, 42], "ApproxPlainModel": [40, None, None, 50, 50, None, None, 40, 50],
          "PlainModelWoPad": [40, None, None, 40, 40, None, None, 40, 40]}[name]
    assert d.threads == th
    assert list(netrun.load_description(name)) == netrun.TOPOLOGIES[name]


@pytest.mark.parametrize("path", FILES, ids=[stem(f) for f in FILES])
def test_cpp_and_python_print_the_same_canonical_form(driver, path):
    from crcnn_amd import netrun
    want = netrun.format_description(netrun.load_description(path, h5_of(path)))
    for h5 in (None, h5_of(path)):
        out = cpp_describe(driver, path, h5)
        assert out.returncode == 0, out.stderr
        assert out.stdout == want
    if stem(path) in BUILTIN:           # the copy compiled into the library is the file
        out = cpp_describe(driver, stem(path))
        assert out.returncode == 0 and out.stdout == want


@pytest.mark.parametrize("path", FILES, ids=[stem(f) for f in FILES])
def test_describe_and_parse_round_trip(driver, path, tmp_path):
    from crcnn_amd import netrun
    d = netrun.load_description(path)
    text = netrun.format_description(d)
    back = netrun.parse_description(text)
    assert list(back) == list(d) and back.input_shape == d.input_shape and back.layer_before_reenc == d.layer_before_reenc and back.threads == d.threads
    assert netrun.format_description(back) == text
    # a plain (kind, name, args) list -- what TOPOLOGIES holds -- is described too
    assert list(netrun.parse_description(netrun.format_description(list(d)))) == list(d)
    canon = tmp_path / "canon.net"
    canon.write_text(text)
    out = cpp_describe(driver, str(canon))
    assert out.returncode == 0 and out.stdout == text


def test_description_details():
    from crcnn_amd import netrun
    d = netrun.load_description(os.path.join(ROOT, "tests", "golden", "topologies", "approx_padded.net"))
    kinds = [k for k, _, _ in d]
    assert kinds == ["conv", "avgpool", "bn", "pad", "conv", "square", "avgpool", "bn", "fc", "fc"]
    assert d[3] == ("pad", "pad1", dict(zd=20, xd=11, yd=11, px=1, py=1))
    assert d[4][2] == dict(xd=13, yd=13, zd=20, xs=2, ys=2, xf=3, yf=3, nf=50)
    assert d[6][2] == dict(xd=6, yd=6, zd=50, xs=1, ys=1, xf=3, yf=3) and d[8][2] == dict(in_dim=800, out_dim=500)
    r = netrun.load_description(os.path.join(ROOT, "tests", "golden", "topologies", "tiny_refresh.net"))
    assert r.layer_before_reenc == 4 and r[4][1] == "classifier.fc3" and list(r) == netrun.TOPOLOGIES["PlainModelTiny"]
    # comments, blank lines and free spacing; asymmetric pads per dimension; another input shape
    t = netrun.parse_description("# head\n\ninput 3 9 7   # rgb\n  pad  p  2 0\nconv c stride 1 2 filter 3 3 filters 4 threads 7\nrefresh\nsquare s\nfc f 5\n")
    assert t.input_shape == (3, 9, 7) and t.layer_before_reenc == 2 and t.threads == [None, 7, None, None]
    assert t[0][2] == dict(zd=3, xd=9, yd=7, px=2, py=0) and t[1][2] == dict(xd=13, yd=7, zd=3, xs=1, ys=2, xf=3, yf=3, nf=4)
    assert t[3][2] == dict(in_dim=4 * 11 * 3, out_dim=5)


GOOD = "input 1 28 28\nconv pool1_features.conv1 stride 2 2 filter 5 5 filters 20\navgpool pool1 stride 1 1 window 2 2\nbn pool1_features.norm1\n"
# (text, line the message must name, model file to check dataset sizes against or None)
MALFORMED = {
    "unknown-kind": (GOOD + "relu act\n", 5, None),
    "unknown-token": (GOOD + "square act1 fast\n", 5, None),
    "unknown-token-after-values": (GOOD + "conv pool2_features.conv2 stride 2 2 filter 3 3 filters 50 dilation 2\n", 5, None),
    "threads-on-a-pool": ("input 1 28 28\npool p stride 1 1 window 2 2 threads 4\n", 2, None),
    "missing-input-line": ("conv c stride 1 1 filter 3 3 filters 2\n", 1, None),
    "filter-larger-than-input": (GOOD + "conv pool2_features.conv2 stride 1 1 filter 12 3 filters 50\n", 5, None),
    "window-larger-than-input": (GOOD + "avgpool p stride 1 1 window 2 12\n", 5, None),
    # 5 x 5 input, stride 3, window 2: the reference sizes two outputs per dimension and fills one (tests/test_gpu_layers.py::test_shape_validation)
    "stride-remainder": ("input 1 5 5\npool p stride 3 3 window 2 2\n", 2, None),
    "stride-remainder-conv": ("input 1 5 5\n\nconv c stride 3 3 filter 2 2 filters 1\n", 3, None),
    "weight-count": (GOOD.replace("filters 20", "filters 21"), 2, "ApproxPlainModel"),
    # 10 filters of 5 x 10 are conv1's 500 weights, but not its 20 biases
    "bias-count": ("input 1 28 28\nconv pool1_features.conv1 stride 2 2 filter 5 10 filters 10\n", 2, "ApproxPlainModel"),
    "batchnorm-count": (GOOD + "bn pool2_features.norm2\n", 5, "ApproxPlainModel"),
    "dense-weight-count": (GOOD + "fc classifier.fc3 500\n", 5, "ApproxPlainModel"),
    "missing-dataset": (GOOD + "bn pool9_features.norm9\n", 5, "ApproxPlainModel"),
    "second-refresh": (GOOD + "refresh\nsquare a\nrefresh\nsquare b\n", 7, None),
    "second-refresh-in-a-row": (GOOD + "refresh\nrefresh\nsquare a\n", 6, None),
    "refresh-at-the-end": (GOOD + "refresh\n", 5, None),
    "conv-after-dense": (GOOD + "fc f 10\nconv c stride 1 1 filter 1 1 filters 2\n", 6, None),
    "pool-after-dense": (GOOD + "fc f 10\npool p stride 1 1 window 1 1\n", 6, None),
    "pad-after-dense": (GOOD + "fc f 10\npad p 1 1\n", 6, None),
    "negative-pad": (GOOD + "pad p -1 1\n", 5, None),
    "no-layers": ("input 1 28 28\n# nothing\n", 2, None),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_descriptions_are_rejected_with_their_line(driver, case, tmp_path):
    from crcnn_amd import netrun
    text, line, model = MALFORMED[case]
    h5 = os.path.join(MODELS, model + ".h5") if model else None
    path = tmp_path / "bad.net"
    path.write_text(text)
    with pytest.raises(ValueError, match=rf"^line {line}: "):
        netrun.load_description(str(path), h5)
    out = cpp_describe(driver, str(path), h5)
    assert out.returncode == 10 and out.stdout == "", (out.stdout, out.stderr)
    assert out.stderr.startswith(f"exception: line {line}: "), out.stderr
    if model:           # without the model file the same text is a valid description: it is the dataset that disagrees
        assert netrun.parse_description(text) and cpp_describe(driver, str(path)).returncode == 0


def test_unknown_model_is_neither_builtin_nor_a_file(driver):
    from crcnn_amd import netrun
    with pytest.raises(ValueError):
        netrun.load_description("PlainModelHuge")
    out = cpp_describe(driver, "PlainModelHuge")
    assert out.returncode == 10 and "unknown model PlainModelHuge" in out.stderr


def float_forward(desc, W, img):
    """float64 forward of a description, zero padding included (benchkit.plain.plain_forward walks TOPOLOGIES[name] only)"""
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
        elif kind in ("pool", "avgpool"):
            xo, yo = (a["xd"] - a["xf"]) // a["xs"] + 1, (a["yd"] - a["yf"]) // a["ys"] + 1
            y = np.zeros((a["zd"], xo, yo))
            for i in range(xo):
                for j in range(yo):
                    y[:, i, j] = x[:, i * a["xs"]:i * a["xs"] + a["xf"], j * a["ys"]:j * a["ys"] + a["yf"]].sum(axis=(1, 2))
            x = y / (a["xf"] * a["yf"]) if kind == "avgpool" else y
        elif kind == "bn":
            x = (x - W[name + ".running_mean"].astype(np.float64)[:, None, None]) / np.sqrt(W[name + ".running_var"].astype(np.float64) + 1e-5)[:, None, None]
        elif kind == "square":
            x = x * x
        elif kind == "pad":
            x = np.pad(x, ((0, 0), (a["px"], a["px"]), (a["py"], a["py"])))
        elif kind == "fc":
            x = (W[name + ".weight"].astype(np.float64).reshape(a["out_dim"], a["in_dim"]) @ x.reshape(-1) + W[name + ".bias"].astype(np.float64)).reshape(1, -1, 1)
    return x.reshape(-1)


@pytest.mark.parametrize("path", [f for f in FILES if stem(f) != "tiny_refresh"], ids=[stem(f) for f in FILES if stem(f) != "tiny_refresh"])
def test_plain_model_forward_walks_the_description(driver, path, tmp_path):
    """plainModelForward -- the labels PlainModulusSearch compares the encrypted predictions with -- from a description: for the three built-in models the labels
    benchkit.plain.plain_forward gives (the float forward tests/test_gpu_host_cpp.py::test_cpp_plain_modulus_search pins the search's labels to), by name and
    by file; for the padded variant the labels of the float forward of its own description"""
    from benchkit.plain import plain_forward
    from crcnn_amd import binding, netrun, synth
    imgs = np.stack([synth.normalize(synth.synth_image(i)).reshape(-1) for i in range(6)]).astype(np.float32)
    imgs.tofile(str(tmp_path / "images.f32"))
    h5 = h5_of(path)
    W = {nm: binding.h5_read(h5, nm) for nm in binding.h5_list(h5) if not nm.endswith("num_batches_tracked")}
    desc = netrun.load_description(path, h5)
    logits = [float_forward(desc, W, im) for im in imgs]
    want = [int(np.argmax(v)) for v in logits]
    name = stem(path)
    if name in BUILTIN:
        assert want == [int(np.argmax(plain_forward(name, W, im.reshape(28, 28)))) for im in imgs]
        assert len(set(want)) > 1       # trained models on different digits: the labels are not one constant
    for model in [path] + ([name] if name in BUILTIN else []):
        out = subprocess.run([driver, "labels", model, h5, str(tmp_path / "images.f32")], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert [int(l.split()[2]) for l in out.stdout.splitlines() if l.startswith("label")] == want
        # the logits themselves: plainModelForward keeps every activation in float32 (relative rounding 6e-8 per stored value, sums accumulated in double), the
        # comparison forward is float64.  Ten layers, one squaring and two batch norms amplify that by far less than 10^4, so 1e-3 of the largest logit is a
        # generous bound -- and a misplaced pad, a wrong window or a wrong reshape order moves the logits by their own size
        got = np.array([[float(v) for v in l.split()[2:]] for l in out.stdout.splitlines() if l.startswith("logits")])
        assert got.shape == (len(imgs), 10)
        for g_, w_ in zip(got, logits):
            assert np.abs(g_ - w_).max() <= 1e-3 * np.abs(w_).max(), (model, g_, w_)
