"""GPU side of the ciphertext x ciphertext multiply (crc_multiply, crc_multiply_relin_forms) and of the degree-3 activation built on it (crc_poly3_relin_forms,
Poly3Layer, netrun's `poly3`): bit for bit against tests/bfv_multiply_model.py -- Evaluator::multiply restated in Python integers over SEAL's own auxiliary base,
pinned to SEAL's recorded squares by tests/test_multiply_cpu.py -- and, for the layer, against its defining Evaluator sequence on oracle + model."""
import glob
import os

import numpy as np
import pytest

from bfv_multiply_model import MultiplyModel, golden_pairs, golden_products, plain_negacyclic
from netcommon import GOLD

pytestmark = pytest.mark.gpu
SETS = sorted(glob.glob(os.path.join(GOLD, "ops_*.npz")))
INVALID = -1
FILL = 0xFFFFFFFFFFFFFFFF
# the default kernels; the plain (round-4) fp64 kernels; the reference-order square chain and key switch (SEAL's 61-bit auxiliary base); the fp64 row kernels
# with 4 and 5 stages per LDS pass (mul64_inv_kernel<4, 16> and <5, 32>, which no other selection reaches)
CONFIGS = {"default": [], "no-wave": [("f64_wave", 0)], "reference-order": [("sq_path", 1), ("relin_path", 1)], "radix-16": [("f64_radix", 4)],
           "radix-32": [("f64_radix", 5)]}
RESET = [("f64_wave", -1), ("sq_path", 0), ("relin_path", 0), ("f64_radix", 0), ("sq_chunk", 0)]
QUADS = [(1, 0, 0, 0), (-0.004, 0, 0.197, 0.5), (0.125, 0.25, 0.5, -1), (-2, 0.375, 0, 0)]


def f32(v):
    return float(np.float32(v))


def configure(E, name):
    for k, v in RESET + CONFIGS[name]:
        E.set_tuning(k, v)


def forms(ca):
    return [(ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT), (ca.NTT, ca.COEFF), (ca.COEFF, ca.NTT)]


@pytest.fixture(scope="module", params=SETS, ids=[os.path.basename(s)[:-4] for s in SETS])
def gs(request):
    import crcnn_amd as ca
    from oracle import orc
    g = dict(np.load(request.param))
    q = [int(x) for x in g["q"]]
    E = ca.Engine(int(g["n"]), q, int(g["t"]), device=0)
    O = orc.Oracle(int(g["n"]), q, int(g["t"]))
    yield os.path.basename(request.param), g, E, O
    E.close()


def fill(E, d, nbytes):
    E.L.crc_memset(E.c, E.p(d), 0xff, nbytes, E.stream)


def test_multiply_op_level_equals_the_model(gs):
    """crc_multiply == model (size 3); crc_multiply_relin_forms == Oracle.relinearize(model): four form combinations x three kernel selections; swapped arguments
    and d_y == d_x (the square, which reaches SEAL's ref_relin); inputs untouched, result buffers pre-filled with 0xff"""
    import crcnn_amd as ca
    name, g, E, O = gs
    x, y, _, _ = golden_pairs(g, O)
    cnt = len(x)
    prod = golden_products(name, g, O)
    relin = np.stack([O.relinearize(prod[i], g["evk"]) for i in range(cnt)])
    d_evk = E.upload(g["evk"])
    d_x, d_y = E.upload(x), E.upload(y)
    d_xn, d_yn = E.upload(x), E.upload(y); E.ntt_fwd(d_xn, cnt); E.ntt_fwd(d_yn, cnt)
    xn, yn = E.download(d_xn, x.shape), E.download(d_yn, y.shape)
    d_o3 = E.alloc(prod.nbytes); d_o = E.alloc(x.nbytes); d_s = E.alloc(x.nbytes)
    d_w = E.alloc(max(E.multiply_relin_work_bytes(cnt), E.square_relin_work_bytes(cnt)))
    for cfg in CONFIGS:
        configure(E, cfg)
        fill(E, d_o3, prod.nbytes)
        E.multiply(d_x, d_y, cnt, d_o3, d_w)
        assert np.array_equal(E.download(d_o3, prod.shape), prod), (cfg, "multiply")
        fill(E, d_o3, prod.nbytes)
        E.multiply(d_y, d_x, cnt, d_o3, d_w)
        assert np.array_equal(E.download(d_o3, prod.shape), prod), (cfg, "multiply, swapped")
        for fin, fout in forms(ca):
            a, b = (d_xn, d_yn) if fin == ca.NTT else (d_x, d_y)
            fill(E, d_o, x.nbytes)
            E.multiply_relin(a, b, cnt, d_evk, d_o, d_w, in_form=fin, out_form=fout)
            raw = E.download(d_o, x.shape)
            fill(E, d_o, x.nbytes)
            E.multiply_relin(b, a, cnt, d_evk, d_o, d_w, in_form=fin, out_form=fout)
            assert np.array_equal(E.download(d_o, x.shape), raw), (cfg, fin, fout, "swapped")
            if fout == ca.NTT:
                E.ntt_inv(d_o, cnt)
            assert np.array_equal(E.download(d_o, x.shape), relin), (cfg, fin, fout)
            # d_y == d_x is the square
            fill(E, d_o, x.nbytes); fill(E, d_s, x.nbytes)
            E.multiply_relin(a, a, cnt, d_evk, d_o, d_w, in_form=fin, out_form=fout)
            E.square_relin(a, cnt, d_evk, d_s, d_w, in_form=fin, out_form=fout)
            sq = E.download(d_s, x.shape)
            assert np.array_equal(E.download(d_o, x.shape), sq), (cfg, fin, fout, "square")
            if fout == ca.COEFF:
                assert np.array_equal(sq[:len(g["ct_in"])], g["ref_relin"]), (cfg, fin, fout, "ref_relin")
    configure(E, "default")
    assert np.array_equal(E.download(d_x, x.shape), x) and np.array_equal(E.download(d_y, y.shape), y)
    assert np.array_equal(E.download(d_xn, x.shape), xn) and np.array_equal(E.download(d_yn, y.shape), yn)


def test_multiply_pass_boundaries():
    """n = 256, five pairs, two ciphertexts per internal pass: the result of the one-pass run"""
    import crcnn_amd as ca
    E = ca.Engine(256, [0x7fffffff380001, 0x3fffffff000001], 1 << 20, device=0)
    sk, pk = E.keygen(5); d_evk = E.upload(E.gen_evk(6, sk))
    cnt = 5
    pl, _ = E.encode(np.linspace(-2, 2, 2 * cnt).astype(np.float32))
    cts = E.encrypt(pk, pl, 77)
    d_x, d_y = E.upload(cts[:cnt]), E.upload(cts[cnt:])
    nb = cts[:cnt].nbytes
    d_o = E.alloc(nb); d_o3 = E.alloc(nb // 2 * 3)
    d_w = E.alloc(E.multiply_relin_work_bytes(cnt))
    res = {}
    for chunk in (0, 2):
        E.set_tuning("sq_chunk", chunk)
        for cfg in CONFIGS:
            for k, v in CONFIGS[cfg]:
                E.set_tuning(k, v)
            fill(E, d_o, nb); fill(E, d_o3, nb // 2 * 3)
            E.multiply_relin(d_x, d_y, cnt, d_evk, d_o, d_w)
            E.multiply(d_x, d_y, cnt, d_o3, d_w)
            res[(chunk, cfg)] = (E.download(d_o, cts[:cnt].shape), E.download(d_o3, (cnt, 3, E.k, E.n)))
            for k, v in RESET[:4]:                 # (everything but sq_chunk)
                E.set_tuning(k, v)
    E.set_tuning("sq_chunk", 0)
    for cfg in CONFIGS:
        assert np.array_equal(res[(2, cfg)][0], res[(0, "default")][0]) and np.array_equal(res[(2, cfg)][1], res[(0, "default")][1]), cfg
    assert not (res[(0, "default")][0] == FILL).all()
    E.close()


# the rings the wave-local kernels cover; the moduli are prefixes of SEAL's defaults for the ring
RINGS = [(4096, 2, 1 << 16, 2), (8192, 3, 1 << 30, 2), (16384, 4, 1 << 30, 1)]


@pytest.mark.parametrize("n,k,t,pairs", RINGS, ids=[f"n{r[0]}" for r in RINGS])
def test_multiply_on_the_wave_local_rings(n, k, t, pairs):
    """keys and ciphertexts from the oracle: device == model, the default selection and f64_wave = 0 give equal bytes, the decrypted product is exact and the
    oracle finds budget left"""
    import crcnn_amd as ca
    from oracle import orc
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(31); evk = O.gen_evk(32, sk)
    vals = np.array([1.5, -0.75, 0.625, 2.25][:2 * pairs], dtype=np.float32)
    pl = O.encode_many(vals)
    cts = O.encrypt_many(pk, pl, 900)
    x, y = np.ascontiguousarray(cts[:pairs]), np.ascontiguousarray(cts[pairs:])
    M = MultiplyModel(O)
    prod = np.stack([M.multiply(x[i], y[i]) for i in range(pairs)])
    relin = np.stack([O.relinearize(prod[i], evk) for i in range(pairs)])
    d_x, d_y, d_evk = E.upload(x), E.upload(y), E.upload(evk)
    d_o3 = E.alloc(prod.nbytes); d_o = E.alloc(x.nbytes)
    d_w = E.alloc(E.multiply_relin_work_bytes(pairs))
    got = {}
    # (beyond the two selections that must agree: the reference-order chain and the 64-bit transforms without their wave-local form reach the other
    # instantiations of the product prologue at these rings)
    for cfg in ("default", "no-wave", "reference-order", "ntt-wave-off"):
        configure(E, cfg if cfg in CONFIGS else "default")
        E.set_tuning("ntt_wave", 0 if cfg == "ntt-wave-off" else -1)
        fill(E, d_o3, prod.nbytes); fill(E, d_o, x.nbytes)
        E.multiply(d_x, d_y, pairs, d_o3, d_w)
        E.multiply_relin(d_x, d_y, pairs, d_evk, d_o, d_w)
        got[cfg] = (E.download(d_o3, prod.shape), E.download(d_o, x.shape))
    configure(E, "default"); E.set_tuning("ntt_wave", -1)
    assert np.array_equal(got["default"][0], prod) and np.array_equal(got["default"][1], relin)
    for cfg in got:
        assert np.array_equal(got[cfg][0], got["default"][0]) and np.array_equal(got[cfg][1], got["default"][1]), cfg
    for i in range(pairs):
        assert np.array_equal(O.decrypt(sk, got["default"][1][i]), plain_negacyclic(pl[i], pl[pairs + i], t)), i
        assert O.noise_budget(sk, got["default"][1][i]) > 0
    E.close()


def poly3_sequence(O, M, evk, x, quad):
    """the defining Evaluator sequence of poly3 on oracle + model"""
    c3, c2, c1, c0 = (f32(v) for v in quad)
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


@pytest.mark.parametrize("name", ["ops_n256_k2_t20", "ops_n256_k3_t30"])
def test_poly3_op_level_equals_the_defining_sequence(name):
    import crcnn_amd as ca
    from oracle import orc
    g = dict(np.load(os.path.join(GOLD, name + ".npz")))
    q = [int(v) for v in g["q"]]
    E = ca.Engine(int(g["n"]), q, int(g["t"]), device=0); O = orc.Oracle(int(g["n"]), q, int(g["t"]))
    M = MultiplyModel(O)
    cts = np.ascontiguousarray(g["ct_in"]); cnt = len(cts)
    d_evk = E.upload(g["evk"])
    d_x = E.upload(cts); d_xn = E.upload(cts); E.ntt_fwd(d_xn, cnt)
    d_o = E.alloc(cts.nbytes); d_s = E.alloc(cts.nbytes); d_u = E.alloc(cts.nbytes)
    d_w = E.alloc(max(E.poly3_relin_work_bytes(cnt), E.multiply_relin_work_bytes(cnt), E.square_relin_work_bytes(cnt)))
    for quad in QUADS:
        want = np.stack([poly3_sequence(O, M, g["evk"], cts[i], quad) for i in range(cnt)])
        rows = E.poly3_rows(*quad)
        assert [r is None for r in rows] == [f32(quad[0]) == 1.0, f32(quad[1]) == 0.0, f32(quad[2]) == 0.0, f32(quad[3]) == 0.0]
        for cfg in CONFIGS:
            configure(E, cfg)
            for fin, fout in forms(ca):
                a = d_xn if fin == ca.NTT else d_x
                fill(E, d_o, cts.nbytes)
                E.poly3_relin(a, cnt, d_evk, *rows, d_o, d_w, in_form=fin, out_form=fout)
                raw = E.download(d_o, cts.shape)
                if quad == (1, 0, 0, 0):
                    E.square_relin(a, cnt, d_evk, d_s, d_w, in_form=fin, out_form=fin)
                    E.multiply_relin(d_s, a, cnt, d_evk, d_u, d_w, in_form=fin, out_form=fout)
                    assert np.array_equal(raw, E.download(d_u, cts.shape)), (cfg, fin, fout, "x^3")
                if fout == ca.NTT:
                    E.ntt_inv(d_o, cnt)
                assert np.array_equal(E.download(d_o, cts.shape), want), (quad, cfg, fin, fout)
    configure(E, "default")
    assert np.array_equal(E.download(d_x, cts.shape), cts)
    E.close()


def test_multiply_entry_points_refuse_invalid_arguments():
    """null pointers, a bad dbc, packed and limb forms, a result that overlaps an input (refused for all three calls, in place included): the status, and nothing
    written"""
    import crcnn_amd as ca
    E = ca.Engine(256, [0x7fffffff380001, 0x3fffffff000001], 1 << 20, device=0)
    sk, pk = E.keygen(3); d_evk = E.upload(E.gen_evk(4, sk))
    cnt = 4
    ctb = 2 * E.k * E.n * 8
    pl, _ = E.encode(np.linspace(-1, 1, 2 * cnt).astype(np.float32))
    cts = E.encrypt(pk, pl, 9)
    d_x, d_y = E.upload(cts[:cnt]), E.upload(cts[cnt:])
    d_o = E.alloc(cnt * ctb * 3 // 2)
    d_w = E.alloc(max(E.poly3_relin_work_bytes(cnt), E.multiply_relin_work_bytes(cnt)))
    rows = E.poly3_rows(0.125, 0.25, 0.5, -1)
    E.L.crc_memset(E.c, E.p(d_o), 0xA5, cnt * ctb * 3 // 2, E.stream)

    def status(fn, *args, **kw):
        with pytest.raises(ca.CrcError) as e:
            fn(*args, **kw)
        return e.value.status

    mu, mr, p3 = E.multiply, E.multiply_relin, E.poly3_relin
    for args in [(None, d_y, cnt, d_o, d_w), (d_x, None, cnt, d_o, d_w), (d_x, d_y, cnt, None, d_w), (d_x, d_y, cnt, d_o, None)]:
        assert status(mu, *args) == INVALID
    for args in [(None, d_y, cnt, d_evk, d_o, d_w), (d_x, None, cnt, d_evk, d_o, d_w), (d_x, d_y, cnt, None, d_o, d_w), (d_x, d_y, cnt, d_evk, None, d_w),
                 (d_x, d_y, cnt, d_evk, d_o, None)]:
        assert status(mr, *args) == INVALID
    for args in [(None, cnt, d_evk, *rows, d_o, d_w), (d_x, cnt, None, *rows, d_o, d_w), (d_x, cnt, d_evk, *rows, None, d_w), (d_x, cnt, d_evk, *rows, d_o, None)]:
        assert status(p3, *args) == INVALID
    for form in (ca.NTTP, ca.NTTL, 17, -1):
        assert status(mr, d_x, d_y, cnt, d_evk, d_o, d_w, in_form=form) == INVALID
        assert status(mr, d_x, d_y, cnt, d_evk, d_o, d_w, out_form=form) == INVALID
        assert status(p3, d_x, cnt, d_evk, *rows, d_o, d_w, in_form=form) == INVALID
        assert status(p3, d_x, cnt, d_evk, *rows, d_o, d_w, out_form=form) == INVALID
    for dbc in (0, 61):
        assert status(mr, d_x, d_y, cnt, d_evk, d_o, d_w, dbc=dbc) == INVALID
        assert status(p3, d_x, cnt, d_evk, *rows, d_o, d_w, dbc=dbc) == INVALID
        assert E.multiply_relin_work_bytes(cnt, dbc=dbc) == 0 and E.poly3_relin_work_bytes(cnt, dbc=dbc) == 0
    # the overlap decision: a result that shares memory with an input is refused, in place or shifted
    x0 = cts[:cnt].copy()
    assert status(mu, d_x, d_y, cnt, d_x, d_w) == INVALID and status(mu, d_x, d_y, cnt, d_y, d_w) == INVALID
    assert status(mr, d_x, d_y, cnt, d_evk, d_x, d_w) == INVALID and status(mr, d_x, d_y, cnt, d_evk, d_y, d_w) == INVALID
    assert status(mr, d_x, d_y, cnt, d_evk, d_y.ptr + ctb, d_w) == INVALID
    assert status(mr, d_x, d_x, cnt, d_evk, d_x, d_w) == INVALID
    assert status(p3, d_x, cnt, d_evk, *rows, d_x, d_w) == INVALID and status(p3, d_x, cnt, d_evk, *rows, d_x.ptr + ctb, d_w) == INVALID
    assert np.array_equal(E.download(d_x, x0.shape), x0) and np.array_equal(E.download(d_y, x0.shape), cts[cnt:])
    assert (E.download(d_o, (cnt * ctb * 3 // 16,)) == 0xA5A5A5A5A5A5A5A5).all()
    for bad in [(0, 1, 1, 1), (-0.0, 1, 0, 0), (1e-46, 1, 0, 0), (float("nan"), 0, 0, 0), (1, float("inf"), 0, 0), (1, 0, 0, 1e39)]:
        with pytest.raises(ValueError):
            E.poly3_rows(*bad)
    # ... and the same arguments, valid, run
    mu(d_x, d_y, cnt, d_o, d_w); mr(d_x, d_y, cnt, d_evk, d_o, d_w); p3(d_x, cnt, d_evk, *rows, d_o, d_w)
    E.sync()
    assert not (E.download(d_o, (cnt * ctb // 8,)) == 0xA5A5A5A5A5A5A5A5).all()
    E.close()


# ---- a network in both hosts ---------------------------------------------------------------------------------------------------------------------------------
CUBIC = os.path.join(GOLD, "activations", "cubic.net")          # input 2 3 3 / poly3 act -0.004 0 0.197 0.5 / avgpool p stride 1 1 window 2 2: no weights
ANY_H5 = os.path.join(GOLD, "models", "ApproxPlainModel.h5")     # (the hosts want a model file; the description reads no dataset of it)
NET_PARAMS = (256, [0x7fffffff380001, 0x3fffffff000001], 1 << 20)
_NET = {}


def cubic_oracle_walk():
    """keys, the 18 input ciphertexts and every layer's tensor of cubic.net from the defining sequence (oracle + model) and Oracle.pool; computed once"""
    if not _NET:
        from oracle import orc
        from crcnn_amd.netrun import load_description
        n, q, t = NET_PARAMS
        O = orc.Oracle(n, q, t)
        M = MultiplyModel(O)
        sk, pk = O.keygen(41); evk = O.gen_evk(42, sk)
        desc = load_description(CUBIC)
        vals = np.linspace(-1.75, 1.75, 18).astype(np.float32)
        x = O.encrypt_many(pk, O.encode_many(vals).reshape(2, 3, 3, n), 4300)
        kind, _, a = desc[0]
        assert kind == "poly3"
        flat = x.reshape(18, 2, O.k, n)
        act = np.stack([poly3_sequence(O, M, evk, flat[i], (a["c3"], a["c2"], a["c1"], a["c0"])) for i in range(18)]).reshape(x.shape)
        p = desc[1][2]
        pooled = np.ascontiguousarray(O.pool(act, p["xs"], p["ys"], p["xf"], p["yf"], div_plain=O.encode(1.0 / (p["xf"] * p["yf"]))[0]))
        assert pooled.shape[:3] == (2, 2, 2)
        _NET.update(O=O, evk=evk, x=x, want=[act, pooled])
    return _NET


def test_poly3_network_cpp_equals_the_oracle(tmp_path):
    import subprocess
    from test_gpu_topology import DRIVER
    w = cubic_oracle_walk()
    n, q, t = NET_PARAMS
    d = str(tmp_path)
    np.array([n, len(q), t] + q, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    w["evk"].tofile(os.path.join(d, "evk.u64")); w["x"].tofile(os.path.join(d, "net_in.u64"))
    out = subprocess.run([DRIVER, "build", CUBIC, ANY_H5, d, "3"], capture_output=True, text=True)
    assert out.returncode == 0 and "build ok" in out.stdout and "describe-ok" in out.stdout, (out.stdout[-1500:], out.stderr[-2500:])
    layers = [l.split() for l in out.stdout.splitlines() if l.startswith("layer ")]
    fused = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("fused")][0]
    assert [l[2] for l in layers] == ["poly3", "avgpool"]
    for i, want in enumerate(w["want"]):
        assert np.array_equal(np.fromfile(os.path.join(d, f"layer_{i}.u64"), dtype=np.uint64), want.reshape(-1)), i
    final = w["want"][-1].reshape(-1)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_unfused.u64"), dtype=np.uint64), final)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_fused.u64"), dtype=np.uint64), final)
    batch = np.fromfile(os.path.join(d, "out_fused_batch.u64"), dtype=np.uint64).reshape(3, -1)
    assert all(np.array_equal(batch[b], final) for b in range(3))
    assert fused == ["act", "p"]                   # fuse() left poly3 a layer of its own


def test_poly3_network_netrun_equals_the_oracle():
    import crcnn_amd as ca
    from crcnn_amd.netrun import Network
    w = cubic_oracle_walk()
    n, q, t = NET_PARAMS
    E = ca.Engine(n, q, t, device=0)
    d_evk = E.upload(w["evk"])
    for resident, fuse, batch in [(False, False, 1), (True, False, 1), (True, True, 3)]:
        net = Network(E, CUBIC, h5_path=ANY_H5, resident=resident, d_evk=d_evk, fuse_pool=fuse)
        net.prepare(batch)
        d_x = E.upload(np.ascontiguousarray(np.repeat(w["x"][None], batch, axis=0)))
        tensors = {}

        def timer(i, lname, kind, phase):
            if phase == 1 and not resident:
                tensors[i] = E.download(net.buf[net.slots[i]], tuple(net.plan[i][5]) + (2, E.k, E.n))
        d_out = net.forward(d_x, batch, timer=timer)
        if net.out_form == ca.NTT:          # (a resident network that ends in a pooling layer hands its result over as it stands)
            E.ntt_inv(d_out, batch * int(np.prod(net.out_shape)))
        out = E.download(d_out, (batch,) + tuple(net.out_shape) + (2, E.k, E.n))
        assert [(pl[0], pl[1]) for pl in net.plan] == [("poly3", "act"), ("avgpool", "p")], net.plan
        for i, tns in tensors.items():
            assert np.array_equal(tns, w["want"][i]), (i, resident)
        if not resident:
            assert sorted(tensors) == [0, 1]
        assert all(np.array_equal(out[b], w["want"][-1]) for b in range(batch)), (resident, fuse, batch)
    E.close()


def test_cpp_multiply_relin_equals_the_model(tmp_path):
    """multiplyRelin of the C++ host on a golden set's pairs, coefficient form and NTT-resident: Oracle.relinearize(model); unequal forms or shapes, a packed
    result form and an empty tensor are std::invalid_argument"""
    import subprocess
    import crcnn_amd as ca
    from oracle import orc
    from test_gpu_topology import DRIVER
    name = "ops_n256_k2_t20.npz"
    g = dict(np.load(os.path.join(GOLD, name)))
    q = [int(v) for v in g["q"]]; n, t = int(g["n"]), int(g["t"])
    O = orc.Oracle(n, q, t)
    x, y, _, _ = golden_pairs(g, O)
    prod = golden_products(name, g, O)
    want = np.stack([O.relinearize(prod[i], g["evk"]) for i in range(len(x))])
    d = str(tmp_path)
    np.array([n, len(q), t] + q, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    g["evk"].tofile(os.path.join(d, "evk.u64")); x.tofile(os.path.join(d, "mul_x.u64")); y.tofile(os.path.join(d, "mul_y.u64"))
    out = subprocess.run([DRIVER, "multiply", d, str(len(x))], capture_output=True, text=True)
    assert out.returncode == 0 and "multiply ok refused 4" in out.stdout, (out.stdout[-1500:], out.stderr[-2500:])
    assert np.array_equal(np.fromfile(os.path.join(d, "mul_cc.u64"), dtype=np.uint64), want.reshape(-1))
    E = ca.Engine(n, q, t, device=0)
    d_n = E.upload(np.fromfile(os.path.join(d, "mul_nn.u64"), dtype=np.uint64).reshape(want.shape)); E.ntt_inv(d_n, len(x))
    assert np.array_equal(E.download(d_n, want.shape), want)
    E.close()
