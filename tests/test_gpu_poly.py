"""GPU side of the polynomial activation c2 x^2 + c1 x + c0 (crc_poly2_relin_forms / crc_poly2_pool_relin_forms, PolyLayer / PolyPoolLayer, netrun's `poly`):
everything bit for bit against the Evaluator sequence that defines the layer, run on the CPU oracle --
    s = relinearize(square(x)); s = multiply_plain(s, encode(c2)); s = add(s, multiply_plain(x, encode(c1))); s = add_plain(s, encode(c0))
-- at the op level (every golden parameter set, every combination of forms, the fused tail and poly2_tail_kernel, the wave-local and the round-4 fp64 kernels,
the reference-order square and key switch), pooled (oracle poly -> Oracle.pool, sum and average), as a network in both hosts, and the refusals."""
import glob
import os
import shutil

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs, model_weights, sha
from test_gpu_topology import cpp_build, py_run

pytestmark = pytest.mark.gpu
SETS = sorted(glob.glob(os.path.join(GOLD, "ops_*.npz")))
ACT = os.path.join(GOLD, "activations")
APPROX_H5 = os.path.join(GOLD, "models", "ApproxPlainModel.h5")
# the four triples of the definition's CPU check, one with only c1 = 0 and one with only c0 = 0
TRIPLES = [(1, 0, 0), (0.25, 0.5, 0.125), (0.1997, 0.5002, 0.1992), (-0.125, -1.5, 2), (0.75, 0, -0.5), (-2, 0.375, 0)]
INVALID, UNSUPPORTED = -1, -4


def f32(v):
    return float(np.float32(v))


class OraclePoly:
    """the defining sequence on the CPU oracle; relinearize(square(x)) of a ciphertext is computed once and shared by the triples"""

    def __init__(self, O, evk):
        self.O, self.evk, self.sq = O, evk, {}

    def one(self, key, x, triple):
        O = self.O
        c2, c1, c0 = (f32(v) for v in triple)
        if key not in self.sq:
            self.sq[key] = O.relinearize(O.square(x), self.evk)
        s = self.sq[key]
        if c2 != 1.0:
            s = O.multiply_plain(s, O.encode(c2)[0])
        if c1 != 0.0:
            s = O.add(s, O.multiply_plain(x, O.encode(c1)[0]))
        if c0 != 0.0:
            s = O.add_plain(s, O.encode(c0)[0])
        return s

    def tensor(self, tag, x, triple):
        x = np.ascontiguousarray(x)
        flat = x.reshape((-1,) + x.shape[-3:])
        return np.stack([self.one((tag, i), flat[i], triple) for i in range(len(flat))]).reshape(x.shape)


# (tuning name, value) lists: the default; the separate tail; the round-4 fp64 kernels (CRC_F64_WAVE=0) with either tail; the reference-order square and key switch
CONFIGS = {
    "default": [],
    "separate-tail": [("poly_tail", 1)],
    "no-wave": [("f64_wave", 0)],
    "no-wave-separate-tail": [("f64_wave", 0), ("poly_tail", 1)],
    "reference-order": [("sq_path", 1), ("relin_path", 1)],
}
RESET = [("poly_tail", 0), ("f64_wave", -1), ("sq_path", 0), ("relin_path", 0)]


def configure(E, name):
    for k, v in RESET + CONFIGS[name]:
        E.set_tuning(k, v)


@pytest.fixture(scope="module", params=SETS, ids=[os.path.basename(s)[:-4] for s in SETS])
def gs(request):
    import crcnn_amd as ca
    from oracle import orc
    g = dict(np.load(request.param))
    q = [int(x) for x in g["q"]]
    E = ca.Engine(int(g["n"]), q, int(g["t"]), device=0)
    yield g, E, OraclePoly(orc.Oracle(int(g["n"]), q, int(g["t"])), g["evk"])
    E.close()


def test_poly_op_level_equals_the_oracle_sequence(gs):
    """crc_poly2_relin_forms on the golden's ciphertexts: six triples x four form combinations x five kernel selections, each the oracle's ciphertexts in the
    requested form; (1, 0, 0) is crc_square_relin_forms' result as well"""
    import crcnn_amd as ca
    g, E, OP = gs
    cts = np.ascontiguousarray(g["ct_in"]); nct = len(cts)
    d_evk = E.upload(g["evk"])
    d_x = E.upload(cts); d_xn = E.upload(cts); E.ntt_fwd(d_xn, nct)
    xn = E.download(d_xn, cts.shape)
    d_y = E.alloc(cts.nbytes); d_s = E.alloc(cts.nbytes)
    d_w = E.alloc(max(E.poly2_relin_work_bytes(nct), E.square_relin_work_bytes(nct)))
    for triple in TRIPLES:
        want = OP.tensor("ops", cts, triple)
        rows = E.poly2_rows(*triple)
        assert [r is None for r in rows] == [f32(triple[0]) == 1.0, f32(triple[1]) == 0.0, f32(triple[2]) == 0.0]
        for cfg in CONFIGS:
            configure(E, cfg)
            for fin, fout in [(ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT), (ca.NTT, ca.COEFF), (ca.COEFF, ca.NTT)]:
                E.L.crc_memset(E.c, E.p(d_y), 0xff, cts.nbytes, E.stream)
                E.poly2_relin(d_xn if fin == ca.NTT else d_x, nct, d_evk, *rows, d_y, d_w, in_form=fin, out_form=fout)
                got_raw = E.download(d_y, cts.shape)
                if triple == (1, 0, 0):
                    E.square_relin(d_xn if fin == ca.NTT else d_x, nct, d_evk, d_s, d_w, in_form=fin, out_form=fout)
                    assert np.array_equal(got_raw, E.download(d_s, cts.shape)), ("square", cfg, fin, fout)
                if fout == ca.NTT:
                    E.ntt_inv(d_y, nct)
                assert np.array_equal(E.download(d_y, cts.shape), want), (triple, cfg, fin, fout)
    configure(E, "default")
    assert np.array_equal(E.download(d_x, cts.shape), cts) and np.array_equal(E.download(d_xn, cts.shape), xn)       # the inputs are left alone


# the rings the wave-local fp64 kernels cover (n = 4096, 8192, 16384) and n = 256; the moduli are prefixes of SEAL's defaults for the ring
RINGS = [(256, [0x7fffffff380001, 0x3fffffff000001], 1 << 20), (4096, None, 1 << 29), (8192, 3, 1 << 30), (16384, 4, 1 << 30)]
WINDOWS = [(2, 2, 1, 1), (3, 3, 1, 1), (2, 2, 2, 2)]          # (xf, yf, xs, ys): CrCNN's overlapping 2 x 2 / 1, 3 x 3 / 1, the decimating 2 x 2 / 2


@pytest.mark.parametrize("n,q,t", RINGS, ids=[f"n{r[0]}" for r in RINGS])
def test_poly_pooled_equals_oracle_poly_then_pool(n, q, t):
    """crc_poly2_pool_relin_forms == oracle poly -> Oracle.pool (sum, and average with its divisor), three windows, every triple; the default selection in all
    four form combinations, the other selections NTT to NTT.  A window the pooled key switch cannot hold is refused with CRC_ERR_UNSUPPORTED"""
    import crcnn_amd as ca
    from oracle import orc
    if not isinstance(q, list):
        q = ca.default_coeff_modulus_128(n)[:q]
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(21); evk = O.gen_evk(22, sk)
    OP = OraclePoly(O, evk)
    B, zd, xd, yd = (2, 2, 4, 4) if n <= 4096 else (1, 2, 4, 4)
    cnt = B * zd * xd * yd
    vals = np.random.default_rng(n).uniform(-2, 2, size=cnt).astype(np.float32)
    x = O.encrypt_many(pk, O.encode_many(vals).reshape(B, zd, xd, yd, n), 500)
    d_evk = E.upload(evk)
    d_x = E.upload(x); d_xn = E.upload(x); E.ntt_fwd(d_xn, cnt)
    triples = TRIPLES if n <= 4096 else TRIPLES[2:5]
    ran = 0
    for xf, yf, xs, ys in WINDOWS:
        xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
        ocnt = B * zd * xo * yo
        oshape = (B, zd, xo, yo, 2, E.k, n)
        d_y = E.alloc(ocnt * 2 * E.k * n * 8)
        if not E.poly2_pool_relin_supported(xf, yf):
            assert not E.square_pool_relin_supported(xf, yf)
            rows = E.poly2_rows(0.5, 0.5, 0.5, window=xf * yf)
            d_w = E.alloc(1 << 20)
            with pytest.raises(ca.CrcError) as e:
                E.poly2_pool_relin(d_xn, B, zd, xd, yd, xs, ys, xf, yf, d_evk, *rows, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT)
            assert e.value.status == UNSUPPORTED
            continue
        assert E.square_pool_relin_supported(xf, yf)
        d_w = E.alloc(E.poly2_pool_relin_work_bytes(B, zd, xd, yd, xs, ys, xf, yf))
        divp, _ = E.encode(np.array([1.0 / (xf * yf)]), dtype=np.float64)
        d_div = E.alloc(E.k * n * 8); E.plain_to_ntt(E.upload(divp), 1, d_div)
        for triple in triples:
            act = OP.tensor("pool", x, triple)
            for avg in (False, True):
                want = np.stack([np.asarray(O.pool(act[b], xs, ys, xf, yf, div_plain=O.encode(1.0 / (xf * yf))[0] if avg else None)) for b in range(B)])
                rows = E.poly2_rows(*triple, window=xf * yf, d_div=d_div if avg else None)
                for cfg in ("default", "separate-tail", "no-wave", "no-wave-separate-tail"):
                    configure(E, cfg)
                    forms = [(ca.NTT, ca.NTT), (ca.COEFF, ca.COEFF), (ca.NTT, ca.COEFF), (ca.COEFF, ca.NTT)] if cfg == "default" else [(ca.NTT, ca.NTT)]
                    for fin, fout in forms:
                        E.L.crc_memset(E.c, E.p(d_y), 0xff, ocnt * 2 * E.k * n * 8, E.stream)
                        E.poly2_pool_relin(d_xn if fin == ca.NTT else d_x, B, zd, xd, yd, xs, ys, xf, yf, d_evk, *rows, d_y, d_w, in_form=fin, out_form=fout)
                        if fout == ca.NTT:
                            E.ntt_inv(d_y, ocnt)
                        assert np.array_equal(E.download(d_y, oshape), want), (n, (xf, yf, xs, ys), triple, avg, cfg, fin, fout)
                        ran += 1
        configure(E, "default")
    assert ran > 0 and np.array_equal(E.download(d_x, x.shape), x)
    # the fitted polynomial still decrypts where the parameters leave room (the toy ring is for bit-exactness only)
    if n >= 4096:
        c2, c1, c0 = (f32(v) for v in TRIPLES[2])
        act = OP.tensor("pool", x, TRIPLES[2])
        got = O.decrypt_value(sk, act[0, 0, 0, 0]); v = float(vals[0])
        assert abs(got - (c2 * v * v + c1 * v + c0)) < 1e-4 and O.noise_budget(sk, act[0, 0, 0, 0]) >= 10
    E.close()


# ---- the network ------------------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_layers(g, desc_path, model):
    """every layer's tensor of the description from the CPU oracle's reference-order loops (the walk of tests/test_gpu_topology.py, with the poly layer)"""
    from crcnn_amd.netrun import load_description
    if desc_path in _ORACLE:
        return _ORACLE[desc_path]
    O, sk, pk, evk, img, x = make_inputs(g)
    W = model_weights(model)
    OP = OraclePoly(O, evk)
    enc = lambda a: O.encode_many(np.asarray(a, dtype=np.float32)).reshape(np.shape(a) + (O.n,))
    t, outs = x, []
    for li, (kind, name, a) in enumerate(load_description(desc_path)):
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
        elif kind == "poly":
            t = OP.tensor(li, t, (a["c2"], a["c1"], a["c0"]))
        else:
            raise AssertionError(kind)
        outs.append(np.ascontiguousarray(t))
    _ORACLE[desc_path] = outs
    return outs


POLY_NET = os.path.join(ACT, "approx_poly.net")
SQUARE_NET = os.path.join(ACT, "approx_poly_square.net")


def test_poly_network_cpp_equals_the_oracle():
    g = load_net_golden("approx256")
    want = oracle_layers(g, POLY_NET, "ApproxPlainModel")
    assert [w.shape[:3] for w in want][3:6] == [(50, 5, 5), (50, 5, 5), (50, 4, 4)]
    # the activation is not the square: the oracle's tensors differ from ApproxPlainModel's from the poly layer on
    assert sha(want[3]) == g["layers"][3]["sha256"] and sha(want[4]) != g["layers"][4]["sha256"]
    d, layers, fused = cpp_build(g, POLY_NET, APPROX_H5)
    assert len(layers) == len(want) == 9
    for i, w in enumerate(want):
        got = np.fromfile(os.path.join(d, f"layer_{i}.u64"), dtype=np.uint64)
        assert tuple(int(v) for v in layers[i][4:7]) == w.shape[:3], layers[i]
        assert np.array_equal(got, w.reshape(-1)), (i, layers[i])
    final = want[-1].reshape(-1)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_unfused.u64"), dtype=np.uint64), final)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_fused.u64"), dtype=np.uint64), final)
    batch = np.fromfile(os.path.join(d, "out_fused_batch.u64"), dtype=np.uint64).reshape(3, -1)
    assert all(np.array_equal(batch[b], final) for b in range(3))
    # fuse() paired the activation with its pooling -- one PolyPoolLayer -- and left no poly or pool2 layer of its own
    assert [nm for nm in fused if "act1" in nm] == ["act1+pool2"] and "pool2" not in fused, fused
    assert len(fused) < len(layers)
    shutil.rmtree(d, ignore_errors=True)


def test_poly_network_netrun_equals_the_oracle():
    g = load_net_golden("approx256")
    want = oracle_layers(g, POLY_NET, "ApproxPlainModel")
    plan, tensors, out = py_run(g, POLY_NET, APPROX_H5, resident=False, fuse=False)
    assert [k for k, _ in plan] == ["conv", "avgpool", "bn", "conv", "poly", "avgpool", "bn", "fc", "fc"]
    for i, w in enumerate(want):
        assert np.array_equal(tensors[i], w), (i, plan[i])
    assert np.array_equal(out[0], want[-1])
    plan, _, out = py_run(g, POLY_NET, APPROX_H5, resident=True, fuse=False, batch=2)
    assert len(plan) == 9 and np.array_equal(out[0], want[-1]) and np.array_equal(out[1], want[-1])
    plan, _, out = py_run(g, POLY_NET, APPROX_H5, resident=True, fuse=True, batch=3)
    assert all(np.array_equal(out[b], want[-1]) for b in range(3))
    assert [p for p in plan if "act1" in p[1]] == [("polypool", "act1+pool2")] and len(plan) < 9, plan


def test_poly_1_0_0_network_gives_the_reference_digests():
    """approx_poly_square.net is ApproxPlainModel with its Square written as a polynomial: the compiled reference's per-layer digests, in both hosts"""
    g = load_net_golden("approx256")
    d, layers, fused = cpp_build(g, SQUARE_NET, APPROX_H5)
    assert len(layers) == len(g["layers"])
    for i, L in enumerate(g["layers"]):
        assert sha(np.fromfile(os.path.join(d, f"layer_{i}.u64"), dtype=np.uint64)) == L["sha256"], (i, L["name"])
    for f in ("out_unfused.u64", "out_fused.u64"):
        assert sha(np.fromfile(os.path.join(d, f), dtype=np.uint64)) == g["out_sha256"]
    batch = np.fromfile(os.path.join(d, "out_fused_batch.u64"), dtype=np.uint64).reshape(3, -1)
    assert all(sha(batch[b]) == g["out_sha256"] for b in range(3))
    assert "act1+pool2" in fused
    shutil.rmtree(d, ignore_errors=True)
    plan, tensors, out = py_run(g, SQUARE_NET, APPROX_H5, resident=False, fuse=False)
    for i, L in enumerate(g["layers"]):
        assert sha(tensors[i]) == L["sha256"], (i, L["name"])
    plan, _, out = py_run(g, SQUARE_NET, APPROX_H5, resident=True, fuse=True, batch=2)
    assert sha(out[0]) == g["out_sha256"] and sha(out[1]) == g["out_sha256"] and ("polypool", "act1+pool2") in plan


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_poly_entry_points_refuse_invalid_arguments():
    """null pointers, bad forms, a window larger than its input, a result that overlaps the NTT-form input the P1 term reads, an unsupported window: the status,
    and nothing written (the result buffer keeps its fill pattern)"""
    import crcnn_amd as ca
    E = ca.Engine(256, [0x7fffffff380001, 0x3fffffff000001], 1 << 20, device=0)
    sk, pk = E.keygen(3); d_evk = E.upload(E.gen_evk(4, sk))
    B, zd, xd, yd = 1, 2, 3, 3
    cnt = B * zd * xd * yd
    ctb = 2 * E.k * E.n * 8
    pl, _ = E.encode(np.linspace(-1, 1, cnt).astype(np.float32))
    d_x = E.upload(E.encrypt(pk, pl, 9)); E.ntt_fwd(d_x, cnt)
    d_y = E.alloc(cnt * ctb); d_w = E.alloc(max(E.poly2_relin_work_bytes(cnt), E.poly2_pool_relin_work_bytes(B, zd, xd, yd, 1, 1, 2, 2)))
    rows = E.poly2_rows(0.25, 0.5, 0.125)
    prow = E.poly2_rows(0.25, 0.5, 0.125, window=4)
    E.L.crc_memset(E.c, E.p(d_y), 0xA5, cnt * ctb, E.stream)

    def status(fn, *args, **kw):
        with pytest.raises(ca.CrcError) as e:
            fn(*args, **kw)
        return e.value.status

    un = E.poly2_relin
    assert status(un, None, cnt, d_evk, *rows, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(un, d_x, cnt, None, *rows, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(un, d_x, cnt, d_evk, *rows, None, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(un, d_x, cnt, d_evk, *rows, d_y, None, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    for form in (ca.NTTP, ca.NTTL, 17, -1):
        assert status(un, d_x, cnt, d_evk, *rows, d_y, d_w, in_form=form, out_form=ca.NTT) == INVALID
        assert status(un, d_x, cnt, d_evk, *rows, d_y, d_w, in_form=ca.NTT, out_form=form) == INVALID
    assert status(un, d_x, cnt, d_evk, *rows, d_y, d_w, dbc=0, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(un, d_x, cnt, d_evk, *rows, d_x, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID                       # in place with a P1 term
    assert status(un, d_x, cnt, d_evk, *rows, d_x.ptr + ctb, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    po = E.poly2_pool_relin
    ok = (B, zd, xd, yd, 1, 1, 2, 2)
    assert status(po, None, *ok, d_evk, *prow, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(po, d_x, *ok, None, *prow, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(po, d_x, *ok, d_evk, *prow, None, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    assert status(po, d_x, *ok, d_evk, *prow, d_y, None, in_form=ca.NTT, out_form=ca.NTT) == INVALID
    for form in (ca.NTTP, 17):
        assert status(po, d_x, *ok, d_evk, *prow, d_y, d_w, in_form=form, out_form=ca.NTT) == INVALID
        assert status(po, d_x, *ok, d_evk, *prow, d_y, d_w, in_form=ca.NTT, out_form=form) == INVALID
    for geom in [(B, zd, xd, yd, 1, 1, 4, 2), (B, zd, xd, yd, 1, 1, 2, 4), (B, zd, xd, yd, 0, 1, 2, 2), (B, zd, xd, yd, 1, 1, 0, 2), (B, 0, xd, yd, 1, 1, 2, 2),
                 (-1, zd, xd, yd, 1, 1, 2, 2)]:
        assert status(po, d_x, *geom, d_evk, *prow, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID, geom
    assert status(po, d_x, *ok, d_evk, *prow, d_x, d_w, in_form=ca.NTT, out_form=ca.NTT) == INVALID                       # the result inside the input
    # what the pooled key switch cannot hold is refused like crc_square_pool_relin_forms refuses it: a 9 x 9 window (more than 64 ciphertexts), the reference-order paths
    assert not E.poly2_pool_relin_supported(9, 9) and not E.square_pool_relin_supported(9, 9)
    E.set_tuning("relin_path", 1)
    assert not E.poly2_pool_relin_supported(2, 2)
    assert status(po, d_x, *ok, d_evk, *prow, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT) == UNSUPPORTED
    E.set_tuning("relin_path", 0)
    assert E.poly2_pool_relin_supported(2, 2)
    assert E.poly2_relin_work_bytes(cnt, dbc=0) == 0 and E.poly2_pool_relin_work_bytes(B, zd, xd, yd, 1, 1, 4, 4) == 0
    with pytest.raises(ca.CrcError):
        E.set_tuning("poly_tails", 1)
    # no refused call wrote anything
    assert (E.download(d_y, (cnt * ctb // 8,)) == 0xA5A5A5A5A5A5A5A5).all()
    # the host-side helper refuses what the description parsers refuse
    for bad in [(0, 1, 1), (float("nan"), 0, 0), (1, float("inf"), 0)]:
        with pytest.raises(ValueError):
            E.poly2_rows(*bad)
    # ... and the same arguments, valid, run
    po(d_x, *ok, d_evk, *prow, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT)
    un(d_x, cnt, d_evk, *rows, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT)
    E.sync()
    E.close()
