"""The client-side activation on the GPU: slots_act_kernel (crc_slots_act_dev) bit for bit against its host twin -- which tests/test_slots_act_cpu.py holds against
the integer model --, crc_slots_refresh_act[_sym]_dev against the three public calls it is defined as, and slot-batched networks with `client_relu` /
`client_maxpool` layers through the host classes against tests/slots_act_model.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import slots_act_model as am
from test_gpu_slots_rescale import DIVISORS, GUARD, Q1, Q2, ring_cases, rows_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = os.path.join(ROOT, "tests", "golden", "slots")
PLANES, XD, YD = 3, 5, 4
# 1 x 1 (60 output rows), 2 x 2 / 2 (12), 3 x 3 / 1 (18: overlapping windows, and more than one XCD group of 16)
WINDOWS = [(XD, YD, 1, 1, 1, 1), (XD, YD, 2, 2, 2, 2), (XD, YD, 1, 1, 3, 3)]
ALL_ONES = np.uint64(0xffffffffffffffff)


@pytest.mark.parametrize("case", range(8))
def test_device_act_equals_the_host_twin(case):
    import crcnn_amd as ca
    n, t = ring_cases()[case]
    E = ca.Engine(n, Q1, t, device=0)
    H = ca.Engine(n, Q1, t, device=-1)
    assert E.slots_supported
    rows_in = PLANES * XD * YD
    cap = min(1000, (t - 1) // 2)
    for D in DIVISORS:
        rows = rows_for(H, n, t, D, rows_in, 13 * n + D % 1000)
        d_in = E.upload(rows)
        for w in WINDOWS:
            xo, yo = am.out_dims(w)
            count = PLANES * xo * yo
            words = count * n
            for relu, c in ((0, 0), (1, cap)) + (((0, cap), (1, 0)) if D == 3 else ()):
                want = H.slots_act(rows, PLANES, w, D, relu, c)
                d_out = E.alloc((words + GUARD) * 8); E.L.crc_memset(E.c, d_out.ptr, 0xff, (words + GUARD) * 8, E.stream)
                E.slots_act_dev(d_in, PLANES, w, D, relu, c, d_out)
                got = E.download(d_out, (words + GUARD,))
                assert np.array_equal(got[:words].reshape(count, n), want), (n, t, D, w, relu, c, "out of place")
                assert (got[words:] == ALL_ONES).all(), (n, t, D, w, "guard words")
                assert np.array_equal(E.download(d_in, (rows_in, n)), rows), (n, t, D, w, "the input was written")
            if w[4:] == (1, 1):
                assert np.array_equal(H.slots_act(rows, PLANES, w, D, 0, 0), H.slots_rescale(rows, D))
                d_io = E.upload(rows)
                E.slots_act_dev(d_io, PLANES, w, D, 1, cap, d_io)
                assert np.array_equal(E.download(d_io, (rows_in, n)), H.slots_act(rows, PLANES, w, D, 1, cap)), (n, t, D, "in place")
            else:
                # any overlap of the two tensors is refused and nothing is written: the same pointer, the output inside the input, the input inside the output
                d_big = E.alloc((rows_in + count) * n * 8)
                call = lambda i, o: E.L.crc_slots_act_dev(E.c, i, PLANES, *w, D, 1, cap, o, None)
                assert call(d_in.ptr, d_in.ptr) == -1 and call(d_in.ptr, d_in.ptr + (rows_in - 1) * n * 8) == -1
                assert call(d_big.ptr + (count - 1) * n * 8, d_big.ptr) == -1 and call(d_big.ptr + count * n * 8, d_big.ptr) == 0
                assert np.array_equal(E.download(d_in, (rows_in, n)), rows)
        # a 1 x 1 window may not overlap in any other way either
        assert E.L.crc_slots_act_dev(E.c, d_in.ptr, PLANES, *WINDOWS[0], D, 0, 0, d_in.ptr + n * 8, None) == -1
    E.close(); H.close()


def test_device_refusals():
    import crcnn_amd as ca
    n = 2048
    W = WINDOWS[1]
    E = ca.Engine(n, Q1, 1 << 20, device=0)                    # no slots: CRC_ERR_PARAMETERS first
    d = E.alloc(XD * YD * n * 8 + 16); p = E.alloc(XD * YD * n * 8 + 16)
    assert E.L.crc_slots_act_dev(E.c, d.ptr, 1, *W, 3, 0, 0, p.ptr, None) == -2 and E.L.crc_slots_act_dev(E.c, d.ptr, 1, *W, 0, 5, 1 << 50, None, None) == -2
    assert E.L.crc_slots_refresh_act_dev(E.c, d.ptr, d.ptr, d.ptr, 1, *W, ca.COEFF, 0, 0, 0, 1, ca.COEFF, p.ptr, p.ptr, None) == -2
    E.close()
    t = 12289
    E = ca.Engine(n, Q1, t, device=0)
    d = E.alloc(XD * YD * n * 8 + 16); p = E.alloc(XD * YD * n * 8 + 16)
    call = lambda i, planes, w, D, relu, cap, o: E.L.crc_slots_act_dev(E.c, i, planes, *w, D, relu, cap, o, None)
    assert call(d.ptr, 1, W, 0, 0, 0, p.ptr) == -1 and call(d.ptr, 1, W, (1 << 62) + 1, 0, 0, p.ptr) == -1
    assert call(d.ptr, 1, W, 3, 2, 0, p.ptr) == -1 and call(d.ptr, 1, W, 3, 0, (t - 1) // 2 + 1, p.ptr) == -1
    assert call(d.ptr, 1, (XD, YD, 1, 1, 6, 1), 3, 0, 0, p.ptr) == -1 and call(d.ptr, 1, (XD, YD, 3, 3, 1, 1), 3, 0, 0, p.ptr) == -1
    assert call(None, 1, W, 3, 0, 0, p.ptr) == -1 and call(d.ptr, 1, W, 3, 0, 0, None) == -1
    assert call(d.ptr + 8, 1, W, 3, 0, 0, p.ptr) == -1 and call(d.ptr, 1, W, 3, 0, 0, p.ptr + 8) == -1          # misaligned
    assert call(d.ptr, 0, W, 3, 0, 0, p.ptr) == 0                                                                # no planes: no error
    E.L.crc_memset(E.c, d.ptr, 0, XD * YD * n * 8, E.stream)
    assert call(d.ptr, 1, W, 1 << 62, 1, (t - 1) // 2, p.ptr) == 0
    assert not E.download(p, (4 * n,)).any()
    assert E.slots_refresh_act_dev_work_bytes(1, W, ca.NTTP) == 0 and E.slots_refresh_act_dev_work_bytes(1, (XD, YD, 3, 3, 1, 1)) == 0
    E.close()


SETS = [(2048, Q1, 12289, 3, 100), (4096, Q2, 65537, 1 << 7, 40)]         # (n, q, t, divisor, cap)
PLANE = (4, 4, 2, 2, 2, 2)                                                # one 4 x 4 plane under a 2 x 2 / 2 window: 16 ciphertexts in, 4 out


@pytest.fixture(scope="module", params=SETS, ids=lambda s: f"n{s[0]}_t{s[2]}")
def pset(request):
    import crcnn_amd as ca
    from oracle import orc
    n, q, t, D, cap = request.param
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(5)
    count = 16
    rng = np.random.RandomState(n)
    half = (t - 1) // 2
    v = rng.randint(-half, half + 1, size=(count, n)).astype(np.int64)
    v[:, 0] = -rng.randint(1, half, size=count)                # a window whose maximum is negative
    v[:, 1] = 0
    v[0, 2:8] = [half, -half, D // 2 if D % 2 == 0 else D, cap * D, (cap + 1) * D, (cap - 1) * D]
    d_pl = E.alloc(count * n * 8)
    E.slots_compose_dev(E.upload(v), count, n, n, 1, d_pl)
    d_ct = E.alloc(count * 2 * E.k * n * 8)
    E.encrypt_dev_forms(E.upload(pk), d_pl, count, 99, ca.COEFF, d_ct, E.alloc(E.encrypt_dev_work_bytes(count)))
    ct = E.download(d_ct, (count, 2, E.k, n))
    yield dict(n=n, q=q, t=t, D=D, cap=cap, E=E, sk=sk, pk=pk, count=count, out=4, v=v, ct=ct, d_sk=E.upload(sk), d_pk=E.upload(pk))
    E.close()


def _composed(P, ct_in, fin, fout, sym, seed, relu, cap):
    """crc_decrypt_dev of the 16 -> crc_slots_act_dev -> crc_encrypt[_sym]_dev_forms of the 4"""
    E, count, out, n = P["E"], P["count"], P["out"], P["n"]
    d_pl = E.alloc(count * n * 8); d_act = E.alloc(out * n * 8)
    E.decrypt_dev(P["d_sk"], E.upload(ct_in), count, d_pl, E.alloc(E.decrypt_dev_work_bytes(count, 2, fin)), in_form=fin)
    E.slots_act_dev(d_pl, 1, PLANE, P["D"], relu, cap, d_act)
    d_out = E.alloc(out * 2 * E.k * n * 8)
    if sym:
        E.encrypt_sym_dev_forms(P["d_sk"], d_act, out, seed, fout, d_out, E.alloc(E.encrypt_sym_dev_work_bytes(out)))
    else:
        E.encrypt_dev_forms(P["d_pk"], d_act, out, seed, fout, d_out, E.alloc(E.encrypt_dev_work_bytes(out)))
    return E.download(d_out, (out, 2, E.k, n))


def _refresh(P, ct_in, fin, fout, sym, seed, relu, cap, in_place=False):
    E, out, n = P["E"], P["out"], P["n"]
    d_in = E.upload(ct_in)
    d_out = d_in if in_place else E.alloc(out * 2 * E.k * n * 8)
    if sym:
        E.slots_refresh_act_sym_dev(P["d_sk"], d_in, 1, PLANE, P["D"], relu, cap, seed, d_out, E.alloc(E.slots_refresh_act_sym_dev_work_bytes(1, PLANE, fin)),
                                    in_form=fin, out_form=fout)
    else:
        E.slots_refresh_act_dev(P["d_sk"], P["d_pk"], d_in, 1, PLANE, P["D"], relu, cap, seed, d_out, E.alloc(E.slots_refresh_act_dev_work_bytes(1, PLANE, fin)),
                                in_form=fin, out_form=fout)
    return E.download(d_out, (out, 2, E.k, n))


@pytest.mark.parametrize("sym", [False, True], ids=["public_key", "secret_key"])
def test_refresh_is_the_three_public_calls(pset, sym):
    import crcnn_amd as ca
    P = pset
    E, n, t, D, cap, count, out = P["E"], P["n"], P["t"], P["D"], P["cap"], P["count"], P["out"]
    d = E.upload(P["ct"]); E.ntt_fwd(d, count)
    forms = {ca.COEFF: P["ct"], ca.NTT: E.download(d, P["ct"].shape)}
    for fin in (ca.COEFF, ca.NTT):
        for fout in (ca.COEFF, ca.NTT):
            want = _composed(P, forms[fin], fin, fout, sym, 4242, 1, cap)
            assert np.array_equal(_refresh(P, forms[fin], fin, fout, sym, 4242, 1, cap), want), (fin, fout, "out of place")
            assert np.array_equal(_refresh(P, forms[fin], fin, fout, sym, 4242, 1, cap, in_place=True), want), (fin, fout, "d_ct_out == d_ct_in")
            assert not np.array_equal(_refresh(P, forms[fin], fin, fout, sym, 4243, 1, cap), want)         # another seed, other ciphertexts
    # the key form of the call: the same key and stream base give the same ciphertexts as the composed calls' key form
    key = bytes(range(32))
    d_in = E.upload(P["ct"]); d_o = E.alloc(out * 2 * E.k * n * 8)
    if sym:
        E.slots_refresh_act_sym_dev(P["d_sk"], d_in, 1, PLANE, D, 0, 0, 0, d_o, E.alloc(E.slots_refresh_act_sym_dev_work_bytes(1, PLANE)), key=key, stream_base=77)
    else:
        E.slots_refresh_act_dev(P["d_sk"], P["d_pk"], d_in, 1, PLANE, D, 0, 0, 0, d_o, E.alloc(E.slots_refresh_act_dev_work_bytes(1, PLANE)), key=key, stream_base=77)
    d_pl = E.alloc(count * n * 8); d_act = E.alloc(out * n * 8); d_k = E.alloc(out * 2 * E.k * n * 8)
    E.decrypt_dev(P["d_sk"], E.upload(P["ct"]), count, d_pl, E.alloc(E.decrypt_dev_work_bytes(count)))
    E.slots_act_dev(d_pl, 1, PLANE, D, 0, 0, d_act)
    if sym:
        E.encrypt_sym_dev_key_forms(P["d_sk"], d_act, out, key, 77, ca.COEFF, d_k, E.alloc(E.encrypt_sym_dev_work_bytes(out)))
    else:
        E.encrypt_dev_key_forms(P["d_pk"], d_act, out, key, 77, ca.COEFF, d_k, E.alloc(E.encrypt_dev_work_bytes(out)))
    assert np.array_equal(E.download(d_o, (out, 2, E.k, n)), E.download(d_k, (out, 2, E.k, n)))
    # what the refreshed ciphertexts decrypt to: the model's integers in every slot, for both relu values
    v4 = [[[[int(x) for x in P["v"][i * 4 + j]] for j in range(4)] for i in range(4)]]
    for relu, c in ((1, cap), (0, 0)):
        got_ct = _refresh(P, P["ct"], ca.COEFF, ca.COEFF, sym, 7, relu, c)
        d_pl = E.alloc(out * n * 8)
        E.decrypt_dev(P["d_sk"], E.upload(got_ct), out, d_pl, E.alloc(E.decrypt_dev_work_bytes(out)))
        d_v = E.alloc(out * n * 8)
        E.slots_decompose_dev(d_pl, out, n, d_v, n, 1)
        got = E.download(d_v, (out, n), dtype=np.int64)
        want_v = am.act_slots(v4, 1, PLANE, D, relu, c)[0]
        assert got.tolist() == [cell for row in want_v for cell in row]
        if relu:
            assert got.min() == 0 and got.max() == cap and (got[:, 0] == 0).all()
        else:
            assert (got[:, 0] < 0).all()
        # the output's budget is a fresh ciphertext's: the four are bit for bit fresh encryptions (above); against the 16 inputs -- fresh public-key encryptions at
        # the same parameters -- a public-key result lies within the budget's one-bit granularity, a secret-key one (less noise) is no worse
        fresh = [E.noise_budget(P["sk"], P["ct"][i]) for i in range(count)]
        after = [E.noise_budget(P["sk"], got_ct[i]) for i in range(out)]
        print("noise budget: inputs", fresh, "refreshed", after)
        assert min(after) >= min(fresh) - 1 and min(after) > 0
    # refusals of the composed call: a divisor out of range, a bad window, a form that is no ciphertext form
    d_in = E.upload(P["ct"]); d_w = E.alloc(E.slots_refresh_act_dev_work_bytes(1, PLANE))
    f = E.L.crc_slots_refresh_act_sym_dev
    assert f(E.c, P["d_sk"].ptr, d_in.ptr, 1, *PLANE, ca.COEFF, 0, 0, 0, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == -1
    assert f(E.c, P["d_sk"].ptr, d_in.ptr, 1, 4, 4, 3, 3, 1, 1, ca.COEFF, 3, 0, 0, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == -1
    assert f(E.c, P["d_sk"].ptr, d_in.ptr, 1, *PLANE, ca.NTTP, 3, 0, 0, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == -1
    assert f(E.c, P["d_sk"].ptr, d_in.ptr, 0, *PLANE, ca.COEFF, 3, 0, 0, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == 0
    assert np.array_equal(E.download(d_in, P["ct"].shape), P["ct"])


# (description under tests/golden/slots, weights, the golden whose ring and moduli the run takes, bits of the slot prime, input_bits, weight_bits).  The ledger
# at (4, 5): 2^9 in front of mp1 (D = 2), 2^13 in front of mp2 and a3 (D = 32), 2^13 at the output
NETS = [("tiny_client_maxpool.net", "PlainModelTiny", "tiny256", 20, 4, 5), ("tiny_client_relu_cap.net", "PlainModelTiny", "tiny256", 20, 4, 5)]


def _net_dir(desc, golden, t_bits, S, seed):
    import crcnn_amd as ca
    from crcnn_amd import netrun
    from netcommon import load_net_golden
    g = load_net_golden(golden)
    n = g["n"]
    t = ca.Engine.slots_prime(n, t_bits)
    assert all(t < q for q in g["q"])
    path = os.path.join(SLOTS, desc)
    layers = netrun.load_description(path)
    zd, xd, yd = layers.input_shape
    images = np.random.RandomState(seed).uniform(-1, 1, size=(S, zd, xd, yd)).astype(np.float32)
    d = tempfile.mkdtemp()
    np.array([n, len(g["q"]), t] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    return path, layers, images, t, d


@pytest.mark.parametrize("desc,model,golden,t_bits,in_bits,w_bits", NETS, ids=[n[0] for n in NETS])
def test_networks_with_client_layers(desc, model, golden, t_bits, in_bits, w_bits):
    """test_host slots_build: S = 5 images in the slots of ONE encrypted tensor through Network::forward (NTT-resident), unfused and fused, with the client's max
    pools and ReLUs on the device: every image's outputs are the integer model's, the final scale is the ledger's, both output tensors have noise budget left"""
    import re
    from netcommon import GOLD, model_weights
    S = 5
    path, layers, images, t, d = _net_dir(desc, golden, t_bits, S, 17)
    h5 = os.path.join(GOLD, "models", model + ".h5")
    out = subprocess.run([os.path.join(ROOT, "crcnn_amd", "lib", "test_host"), "slots_build", path, h5, d, str(S), str(in_bits), str(w_bits)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout, out.stderr[-300:])
    assert "describe-ok" in out.stdout and "slots_build ok" in out.stdout
    scales = am.ledger(list(layers), in_bits, w_bits)
    assert [scales[i] >> a["bits"] for i, (k, _, a) in enumerate(layers) if k in am.CLIENT] == [2, 32, 32]
    want, scale = am.network_forward(list(layers), model_weights(model), images, t, in_bits, w_bits)
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines() if " " in l)
    assert float(lines["slot_scale"]) == float(scale) == float(scales[-1])
    budgets = lines["budget"].split()
    assert int(budgets[1]) > 0 and int(budgets[3]) > 0, lines["budget"]
    for name in ("slots_unfused.i64", "slots_fused.i64"):
        got = np.fromfile(os.path.join(d, name), dtype=np.int64).reshape(S, -1)
        assert got.tolist() == want, name
    assert len({tuple(r) for r in want}) == S
    # fuse() pairs neither client layer with anything: all seven layers are still there
    assert int(re.search(r"fused: (\d+) layers removed, (\d+) left", out.stderr).group(2)) == 7


def test_client_layers_under_every_forward_plan():
    """test_host slots_act_plan: the same integers from the NTT-resident forward, a profiled forward timed with events (the layers are timed as layers, not as
    T_REENC; their producers hand over CRC_NTT; the budget behind them is larger than in front of them), two-level chunking (three tensors as a batch, one image
    per chunk), the layerwise coefficient-form forward and secret-key re-encryption; a packed output form is refused"""
    from netcommon import GOLD
    desc, model, golden, t_bits, in_bits, w_bits = NETS[1]
    S = 3
    path, layers, images, t, d = _net_dir(desc, golden, t_bits, S, 23)
    out = subprocess.run([os.path.join(ROOT, "crcnn_amd", "lib", "test_host"), "slots_act_plan", path, os.path.join(GOLD, "models", model + ".h5"), d, str(S),
                          str(in_bits), str(w_bits)], capture_output=True, text=True)
    print(out.stdout, out.stderr[-500:])
    assert out.returncode == 0 and "slots_act_plan ok" in out.stdout, out.stderr[-2000:]
    assert out.stdout.count("client layer") == 3
