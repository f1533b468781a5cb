"""GPU side of the network descriptions: crc_pad (pad_kernel) against its definition, the three models built from their description files against the compiled
reference's per-layer digests (through the C++ classes and through netrun), a padded variant of ApproxPlainModel against the CPU oracle layer by layer --
unfused, fused and NTT-resident, in both hosts --, a description with a refresh point against the published configuration's golden, and bench_host on the
path of a description file.  (The reference's fourth model file, PlainModel.h5, is 2.4 MiB and stays out of the tree: the padded variant carries the
coverage of the pad layer.)"""
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs, model_weights, sha, sha_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crcnn_amd", "lib")
DRIVER = os.path.join(LIB, "test_host")
TOPO = os.path.join(GOLD, "topologies")
BUILTIN = {"tiny256": "PlainModelTiny", "approx256": "ApproxPlainModel", "wopad256": "PlainModelWoPad"}
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def builtin_file(model):
    return os.path.join(ROOT, "crcnn_amd", "models", model + ".net")


# ---- 1. crc_pad ---------------------------------------------------------------------------------------------------------------------------------------
# n = 256: half a block copies one row in one step; 1024: the one-vector loop twice; 4096 and 16384: the four-vector loop (twice / eight times)
@pytest.mark.parametrize("n", [256, 1024, 4096, 16384])
@pytest.mark.parametrize("form", ["coeff", "ntt"])
def test_pad_interior_is_the_input_and_the_border_is_zero(n, form):
    import crcnn_amd as ca
    E = ca.Engine(n, Q2, 1 << 20, device=0)
    f = ca.COEFF if form == "coeff" else ca.NTT
    B, zd, xd, yd = 3, 2, 3, 4
    px0, px1, py0, py1 = 1, 2, 0, 3
    xo, yo = xd + px0 + px1, yd + py0 + py1
    rng = np.random.default_rng(n + f)
    x = np.stack([rng.integers(0, q, size=(B, zd, xd, yd, 2, n), dtype=np.uint64) for q in Q2], axis=5)       # canonical residues [..][2][k][n]
    assert x.shape == (B, zd, xd, yd, 2, 2, n)
    d_x = E.upload(x)
    out_bytes = B * zd * xo * yo * 2 * E.k * n * 8
    d_y = E.alloc(out_bytes + 4096)           # a guard behind the tensor: nothing may be written there
    E.L.crc_memset(E.c, d_y.ptr, 0xA5, out_bytes + 4096, E.stream)
    E.pad(d_x, B, zd, xd, yd, px0, px1, py0, py1, f, d_y)
    y = E.download(d_y, (B, zd, xo, yo, 2, E.k, n))
    guard = E.download(d_y.ptr + out_bytes, (512,))
    assert np.array_equal(y[:, :, px0:px0 + xd, py0:py0 + yd], x)
    border = np.ones((xo, yo), dtype=bool); border[px0:px0 + xd, py0:py0 + yd] = False
    assert border.sum() == xo * yo - xd * yd and not y[:, :, border].any()
    assert (guard == 0xA5A5A5A5A5A5A5A5).all()
    assert np.array_equal(E.download(d_x, x.shape), x)            # the input is left alone
    # a zero pad is a plain copy
    d_c = E.alloc(x.nbytes)
    E.L.crc_memset(E.c, d_c.ptr, 0xA5, x.nbytes, E.stream)
    E.pad(d_x, B, zd, xd, yd, 0, 0, 0, 0, f, d_c)
    assert np.array_equal(E.download(d_c, x.shape), x)
    # one side only, the other dimension: the offsets are per side
    d_1 = E.alloc(B * zd * xd * (yd + 1) * 2 * E.k * n * 8)
    E.pad(d_x, B, zd, xd, yd, 0, 0, 1, 0, f, d_1)
    y1 = E.download(d_1, (B, zd, xd, yd + 1, 2, E.k, n))
    assert np.array_equal(y1[:, :, :, 1:], x) and not y1[:, :, :, 0].any()
    E.close()


def test_pad_refuses_invalid_arguments():
    import crcnn_amd as ca
    E = ca.Engine(256, Q2, 1 << 20, device=0)
    B, zd, xd, yd = 2, 1, 2, 2
    ctb = 2 * E.k * E.n * 8
    d_x = E.alloc(B * zd * 4 * 4 * ctb * 2); d_y = E.alloc(B * zd * 4 * 4 * ctb)
    INVALID = -1

    def refused(*args):
        with pytest.raises(ca.CrcError) as e:
            E.pad(*args)
        return e.value.status

    for pads in [(-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -2)]:
        assert refused(d_x, B, zd, xd, yd, *pads, ca.COEFF, d_y) == INVALID
    assert refused(None, B, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_y) == INVALID
    assert refused(d_x, B, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, None) == INVALID
    assert refused(d_x, B, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_x) == INVALID                       # in place
    assert refused(d_x, B, zd, xd, yd, 1, 1, 1, 1, ca.NTT, d_x.ptr + ctb) == INVALID               # d_y starts inside d_x
    assert refused(d_x.ptr + B * zd * 16 * ctb - ctb, B, zd, xd, yd, 1, 1, 1, 1, ca.NTT, d_x) == INVALID      # d_x starts inside d_y's last ciphertext
    assert refused(d_x, B, zd, xd, yd, 0, 0, 0, 0, ca.COEFF, d_x) == INVALID                       # a zero pad is a copy, not a no-op: still not in place
    assert refused(d_x.ptr + 8, B, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_y) == INVALID               # 16-byte accesses
    for form in (ca.NTTP, ca.NTTL, 17):
        assert refused(d_x, B, zd, xd, yd, 1, 1, 1, 1, form, d_y) == INVALID                       # canonical rows only
    assert refused(d_x, B, 0, xd, yd, 1, 1, 1, 1, ca.COEFF, d_y) == INVALID
    assert refused(d_x, -1, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_y) == INVALID
    # adjacent buffers are fine: d_y right behind d_x
    E.pad(d_x, B, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_x.ptr + B * zd * xd * yd * ctb)
    E.pad(d_x, 0, zd, xd, yd, 1, 1, 1, 1, ca.COEFF, d_y)                                             # an empty batch is no work
    E.sync()
    E.close()


# ---- shared drivers -------------------------------------------------------------------------------------------------------------------------------------
def write_inputs(g, d, with_keys=False):
    O, sk, pk, evk, img, x = make_inputs(g)
    np.array([g["n"], len(g["q"]), g["t"]] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    evk.tofile(os.path.join(d, "evk.u64")); x.tofile(os.path.join(d, "net_in.u64"))
    if with_keys:
        sk.tofile(os.path.join(d, "sk.u64")); pk.tofile(os.path.join(d, "pk.u64"))
    return O, sk, evk, x


def cpp_build(g, desc, h5, batch=3):
    """test_host build: layer by layer, NTT-resident, fused, fused on a batch -- one built network"""
    d = tempfile.mkdtemp()
    write_inputs(g, d)
    out = subprocess.run([DRIVER, "build", desc, h5, d, str(batch)], capture_output=True, text=True)
    assert out.returncode == 0 and "build ok" in out.stdout and "describe-ok" in out.stdout, (out.stdout[-1500:], out.stderr[-2500:])
    layers = [l.split() for l in out.stdout.splitlines() if l.startswith("layer ")]
    fused = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("fused")][0]
    return d, layers, fused


def py_run(g, desc, h5, resident, fuse, batch=1):
    """netrun.Network on a description; returns (plan after fusing, per-layer tensors of image 0 when not resident, output [batch][...])"""
    import crcnn_amd as ca
    from crcnn_amd.netrun import Network
    O, sk, pk, evk, img, x = make_inputs(g)
    E = ca.Engine(g["n"], g["q"], g["t"], device=0)
    net = Network(E, desc, h5_path=h5, resident=resident, d_evk=E.upload(evk), fuse_pool=fuse)
    net.prepare(batch)
    d_x = E.upload(np.ascontiguousarray(np.repeat(x[None], batch, axis=0)))
    tensors = {}

    def timer(i, lname, kind, phase):
        if phase == 1 and not resident:
            tensors[i] = E.download(net.buf[net.slots[i]], tuple(net.plan[i][5]) + (2, E.k, E.n))
    d_out = net.forward(d_x, batch, timer=timer)
    out = E.download(d_out, (batch,) + tuple(net.out_shape) + (2, E.k, E.n))
    plan = [(pl[0], pl[1]) for pl in net.plan]
    E.close()
    return plan, tensors, out


# ---- 2. the three models from their description files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BUILTIN))
def test_cpp_network_from_description_file_matches_the_reference(name):
    g = load_net_golden(name)
    model = BUILTIN[name]
    d, layers, fused = cpp_build(g, builtin_file(model), os.path.join(GOLD, "models", model + ".h5"))
    assert len(layers) == len(g["layers"])
    for i, L in enumerate(g["layers"]):
        assert sha(np.fromfile(os.path.join(d, f"layer_{i}.u64"), dtype=np.uint64)) == L["sha256"], (name, i, L["name"])
    assert sha(np.fromfile(os.path.join(d, "out_unfused.u64"), dtype=np.uint64)) == g["out_sha256"]
    assert sha(np.fromfile(os.path.join(d, "out_fused.u64"), dtype=np.uint64)) == g["out_sha256"]
    batch = np.fromfile(os.path.join(d, "out_fused_batch.u64"), dtype=np.uint64).reshape(3, -1)
    assert all(sha(batch[b]) == g["out_sha256"] for b in range(3))
    assert len(fused) < len(layers)              # fuse() still folds the built-in models
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("name", sorted(BUILTIN))
def test_netrun_network_from_description_file_matches_the_reference(name):
    import crcnn_amd as ca
    from crcnn_amd.netrun import Network
    g = load_net_golden(name)
    model = BUILTIN[name]
    h5 = os.path.join(GOLD, "models", model + ".h5")
    O, sk, pk, evk, img, x = make_inputs(g)
    E = ca.Engine(g["n"], g["q"], g["t"], device=0)
    net = Network(E, builtin_file(model), h5_path=h5, resident=False, d_evk=E.upload(evk))
    net.prepare(1)
    digests = {}

    def timer(i, lname, kind, phase):
        if phase == 1:
            digests[i] = sha_device(E, net.buf[net.slots[i]], int(np.prod(net.plan[i][5])) * 2 * E.k * E.n * 8)
    out = E.download(net.forward(E.upload(x[None]), 1, timer=timer), (1, 10, 1, 2, E.k, E.n))
    E.close()
    for i, L in enumerate(g["layers"]):
        assert digests[i] == L["sha256"], (name, i, L["name"])
    assert sha(out) == g["out_sha256"]
    plan, _, outf = py_run(g, builtin_file(model), h5, resident=True, fuse=True, batch=2)
    assert len(plan) < len(g["layers"])
    assert sha(outf[0]) == g["out_sha256"] and sha(outf[1]) == g["out_sha256"]


# ---- 3. a padded network against the oracle -------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_layers(g, desc_path, model):
    """every layer's tensor of the description from the CPU oracle's reference-order loops; `pad` inserts all-zero ciphertexts"""
    from crcnn_amd.netrun import load_description
    if desc_path in _ORACLE:
        return _ORACLE[desc_path]
    O, sk, pk, evk, img, x = make_inputs(g)
    W = model_weights(model)
    enc = lambda a: O.encode_many(np.asarray(a, dtype=np.float32)).reshape(np.shape(a) + (O.n,))
    t, outs = x, []
    for kind, name, a in load_description(desc_path):
        if kind == "conv":
            t = O.conv(t, O.plains_to_ntt(enc(W[name + ".weight"].reshape(a["nf"], a["zd"], a["xf"], a["yf"]))), enc(W[name + ".bias"]), a["xs"], a["ys"], threads=8)
        elif kind == "fc":
            flat = np.ascontiguousarray(t).reshape(a["in_dim"], 1, 1, 2, O.k, O.n)
            t = O.conv(flat, O.plains_to_ntt(enc(W[name + ".weight"].reshape(a["out_dim"], a["in_dim"], 1, 1))), enc(W[name + ".bias"]), 1, 1,
                       threads=8).reshape(1, a["out_dim"], 1, 2, O.k, O.n)
        elif kind in ("pool", "avgpool"):
            t = O.pool(t, a["xs"], a["ys"], a["xf"], a["yf"], div_plain=O.encode(1.0 / (a["xf"] * a["yf"]))[0] if kind == "avgpool" else None, threads=8)
        elif kind == "bn":
            t = O.bn(t, enc(W[name + ".running_mean"]), enc(np.float32(1.0 / np.sqrt(W[name + ".running_var"].astype(np.float64) + 0.00001))), threads=8)
        elif kind == "square":
            t = O.square_layer(t, evk, threads=8)
        elif kind == "pad":
            t = np.pad(np.asarray(t), ((0, 0), (a["px"], a["px"]), (a["py"], a["py"]), (0, 0), (0, 0), (0, 0)))
        else:
            raise AssertionError(kind)
        outs.append(np.ascontiguousarray(t))
    _ORACLE[desc_path] = outs
    return outs


PADDED = os.path.join(TOPO, "approx_padded.net")
APPROX_H5 = os.path.join(GOLD, "models", "ApproxPlainModel.h5")


def test_padded_network_cpp_equals_the_oracle():
    g = load_net_golden("approx256")
    want = oracle_layers(g, PADDED, "ApproxPlainModel")
    shapes = [w.shape[:3] for w in want]
    assert shapes[3] == (20, 13, 13) and shapes[4] == (50, 6, 6) and shapes[6] == (50, 4, 4) and shapes[-1] == (1, 10, 1)
    d, layers, fused = cpp_build(g, PADDED, APPROX_H5)
    assert len(layers) == len(want) == 10
    for i, w in enumerate(want):
        got = np.fromfile(os.path.join(d, f"layer_{i}.u64"), dtype=np.uint64)
        assert tuple(int(v) for v in layers[i][4:7]) == w.shape[:3], layers[i]
        assert np.array_equal(got, w.reshape(-1)), (i, layers[i])
    final = want[-1].reshape(-1)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_unfused.u64"), dtype=np.uint64), final)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_fused.u64"), dtype=np.uint64), final)
    batch = np.fromfile(os.path.join(d, "out_fused_batch.u64"), dtype=np.uint64).reshape(3, -1)
    assert all(np.array_equal(batch[b], final) for b in range(3))
    # fuse() folded what it may (conv1 + pool1, norm2 into fc3) and nothing across the pad: bn(0) is not 0, so norm1 stays a layer of its own in front of it
    assert "pad1" in fused and "pool1_features.norm1" in fused and "pool2_features.conv2" in fused, fused
    assert fused.index("pool1_features.norm1") + 1 == fused.index("pad1") == fused.index("pool2_features.conv2") - 1
    assert len(fused) < len(layers)
    shutil.rmtree(d, ignore_errors=True)


def test_padded_network_netrun_equals_the_oracle():
    g = load_net_golden("approx256")
    want = oracle_layers(g, PADDED, "ApproxPlainModel")
    plan, tensors, out = py_run(g, PADDED, APPROX_H5, resident=False, fuse=False)
    assert [k for k, _ in plan] == ["conv", "avgpool", "bn", "pad", "conv", "square", "avgpool", "bn", "fc", "fc"]
    for i, w in enumerate(want):
        assert np.array_equal(tensors[i], w), (i, plan[i])
    assert np.array_equal(out[0], want[-1])
    plan, _, out = py_run(g, PADDED, APPROX_H5, resident=True, fuse=False, batch=2)
    assert len(plan) == 10 and np.array_equal(out[0], want[-1]) and np.array_equal(out[1], want[-1])
    plan, _, out = py_run(g, PADDED, APPROX_H5, resident=True, fuse=True, batch=2)
    assert np.array_equal(out[0], want[-1]) and np.array_equal(out[1], want[-1])
    names = [nm for _, nm in plan]
    assert len(plan) < 10 and ("pad", "pad1") in plan and ("bn", "pool1_features.norm1") in plan and ("conv", "pool2_features.conv2") in plan, plan
    assert names.index("pool1_features.norm1") + 1 == names.index("pad1") == names.index("pool2_features.conv2") - 1


# ---- 5. a description with a refresh point --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unfused", "fused-batch"])
def test_description_with_refresh_reproduces_the_published_configuration(case):
    """tests/golden/topologies/tiny_refresh.net says where the client-side refresh sits; test_host netr is told -1 and takes the description's point.  Checked as
    tests/test_gpu_host_cpp.py checks the built-in model with the refresh point on its command line: digests in front of the refresh, the floats the client saw,
    the decrypted outputs behind it, the remaining budget"""
    name = "tiny2048r"
    g = load_net_golden(name)
    batch, fuse = {"unfused": (1, False), "fused-batch": (5, True)}[case]
    d = tempfile.mkdtemp()
    write_inputs(g, d, with_keys=True)
    h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
    out = subprocess.run([DRIVER, "netr", os.path.join(TOPO, "tiny_refresh.net"), h5, d, str(batch), "-1", "1" if fuse else "0", "0"], capture_output=True, text=True)
    assert out.returncode == 0 and "netr ok" in out.stdout, out.stderr[-2000:]
    n = g["n"]
    if not fuse:
        for i in range(g["layer_before_reenc"]):
            assert sha(np.fromfile(os.path.join(d, f"pre_{i}.u64"), dtype=np.uint64)) == g["layers"][i]["sha256"], (name, i)
        assert not os.path.exists(os.path.join(d, f"pre_{g['layer_before_reenc']}.u64"))
    want_fl = np.array(g["reenc_floats_bits"], dtype=np.uint32)
    fl = np.fromfile(os.path.join(d, "reenc_floats.f32"), dtype=np.uint32).reshape(batch, -1)
    assert all(np.array_equal(fl[b], want_fl) for b in range(batch))
    want_dec = np.load(os.path.join(GOLD, f"net_{name}_dec.npz"))["dec"]
    assert sha(want_dec) == g["dec_sha256"]
    dec = np.fromfile(os.path.join(d, "dec.u64"), dtype=np.uint64).reshape(batch, 10, n)
    assert all(np.array_equal(dec[b], want_dec) for b in range(batch))
    bud = np.fromfile(os.path.join(d, "budget.u64"), dtype=np.uint64).reshape(batch, 10)
    assert int(bud.min()) >= min(g["budget"]) - 2 and int(bud.max()) <= max(g["budget"]) + 2, (bud, g["budget"])
    shutil.rmtree(d, ignore_errors=True)


def test_netrun_refuses_a_refresh_point():
    import crcnn_amd as ca
    from crcnn_amd.netrun import Network
    E = ca.Engine(256, Q2, 1 << 20, device=0)
    with pytest.raises(ValueError, match="refresh"):
        Network(E, os.path.join(TOPO, "tiny_refresh.net"), h5_path=os.path.join(GOLD, "models", "PlainModelTiny.h5"))
    E.close()


# ---- 6. bench_host on the path of a description ---------------------------------------------------------------------------------------------------------
def test_bench_host_takes_a_description_file():
    g = load_net_golden("tiny256")
    O, sk, pk, evk, img, x = make_inputs(g)
    d = tempfile.mkdtemp()
    x.tofile(os.path.join(d, "in.u64"))
    h5 = os.path.join(GOLD, "models", "PlainModelTiny.h5")
    outs = {}
    for tag, model in (("name", "PlainModelTiny"), ("file", builtin_file("PlainModelTiny"))):
        cmd = [os.path.join(LIB, "bench_host"), f"model={model}", f"h5={h5}", f"n={g['n']}", f"k={len(g['q'])}", f"t={g['t']}", "q=" + ",".join(str(v) for v in g["q"]),
               f"inputs={os.path.join(d, 'in.u64')}", "distinct=1", "batch=4", "chunk=2", "steps=1", "warmup=0", f"outputs={os.path.join(d, tag + '.u64')}"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-2000:])
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert line["last_timed_launch_identical_to_first"] is True
        outs[tag] = np.fromfile(os.path.join(d, tag + ".u64"), dtype=np.uint64)
    assert sha(outs["name"]) == g["out_sha256"] and sha(outs["file"]) == g["out_sha256"]
    assert np.array_equal(outs["name"], outs["file"])
    shutil.rmtree(d, ignore_errors=True)
