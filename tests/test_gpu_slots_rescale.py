"""The slot-wise rescale on the GPU: slots_rescale_kernel (crc_slots_rescale_dev) bit for bit against its host twin -- which tests/test_slots_rescale_cpu.py holds
against the integer model --, crc_slots_refresh[_sym]_dev against the three public calls it is defined as, and slot-batched networks with `rescale` layers through
the host classes against tests/slots_rescale_model.py."""
import os

import numpy as np
import pytest

import slots_rescale_model as rm

pytestmark = pytest.mark.gpu
Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
BIG = 0x7fffffff380001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = os.path.join(ROOT, "tests", "golden", "slots")
DIVISORS = [1, 3, 1 << 7, 1 << 39]
GUARD = 8


def ring_cases():
    """the ring cases of test_gpu_slots.py: every pass structure of the row transform, the lazy and the strict butterflies"""
    import crcnn_amd as ca
    out = [(n, ca.Engine.slots_prime(n, 30)) for n in (256, 2048, 4096, 8192)]
    return out + [(256, BIG), (256, ca.Engine.slots_prime(256, 60)), (64, 257), (16384, ca.Engine.slots_prime(16384, 50))]


def rows_for(H, n, t, D, count, seed):
    """count rows of any 64-bit words (most of them >= t); row 1 composed from the extremes, 0 and the ties +-D/2, +-3D/2 that fit, row 2 the same with words >= t"""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, 1 << 63, size=(count, n), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, size=(count, n)).astype(np.uint64)
    half = (t - 1) // 2
    v = [half, -half, 0, 1, -1]
    for m in (1, 3):
        if D % 2 == 0 and m * (D // 2) <= half:
            v += [m * (D // 2), -m * (D // 2), m * (D // 2) - 1, -m * (D // 2) + 1]
    for m in (1, 2):
        if m * D <= half:
            v += [m * D, -m * D, m * D - 1, -m * D + 1]
    v = (v + [0] * n)[:n]
    rows[1] = H.slots_compose(np.array([v], dtype=np.int64), 1, n, n, 1)[0]
    rows[2] = rows[1]
    if t < (1 << 63):
        rows[2, ::3] += np.uint64(t)
    return rows


@pytest.mark.parametrize("case", range(8))
def test_device_rescale_equals_the_host_twin(case):
    import crcnn_amd as ca
    n, t = ring_cases()[case]
    E = ca.Engine(n, Q1, t, device=0)
    H = ca.Engine(n, Q1, t, device=-1)
    assert E.slots_supported
    for D in DIVISORS:
        rows = rows_for(H, n, t, D, 17, 13 * n + D % 1000)
        want = H.slots_rescale(rows, D)
        assert np.array_equal(want[1], want[2])
        for count in (3, 17):                                  # 17 crosses one XCD group of 16
            words = count * n
            d_in = E.upload(rows[:count])
            d_out = E.alloc((words + GUARD) * 8); E.L.crc_memset(E.c, d_out.ptr, 0xff, (words + GUARD) * 8, E.stream)
            E.slots_rescale_dev(d_in, count, D, d_out)
            got = E.download(d_out, (words + GUARD,))
            assert np.array_equal(got[:words].reshape(count, n), want[:count]), (n, t, D, count, "out of place")
            assert (got[words:] == np.uint64(0xffffffffffffffff)).all(), (n, t, D, count, "guard words")
            assert np.array_equal(E.download(d_in, (count, n)), rows[:count]), (n, t, D, count, "the input was written")
            E.slots_rescale_dev(d_in, count, D, d_in)
            assert np.array_equal(E.download(d_in, (count, n)), want[:count]), (n, t, D, count, "in place")
    E.close(); H.close()


def test_device_refusals():
    import crcnn_amd as ca
    n = 2048
    E = ca.Engine(n, Q1, 1 << 20, device=0)                    # no slots: CRC_ERR_PARAMETERS first
    d = E.alloc(n * 8 + 16)
    assert E.L.crc_slots_rescale_dev(E.c, d.ptr, 1, 3, d.ptr, None) == -2 and E.L.crc_slots_rescale_dev(E.c, d.ptr, 1, 0, d.ptr, None) == -2
    E.close()
    E = ca.Engine(n, Q1, 12289, device=0)
    d = E.alloc(n * 8 + 16); p = E.alloc(n * 8 + 16)
    call = lambda i, cnt, D, o: E.L.crc_slots_rescale_dev(E.c, i, cnt, D, o, None)
    assert call(d.ptr, 1, 0, p.ptr) == -1 and call(d.ptr, 1, (1 << 62) + 1, p.ptr) == -1
    assert call(None, 1, 3, p.ptr) == -1 and call(d.ptr, 1, 3, None) == -1
    assert call(d.ptr + 8, 1, 3, p.ptr) == -1 and call(d.ptr, 1, 3, p.ptr + 8) == -1          # misaligned
    assert call(d.ptr, 0, 3, p.ptr) == 0                                                       # an empty batch is no error
    E.L.crc_memset(E.c, d.ptr, 0, n * 8, E.stream)
    assert call(d.ptr, 1, 1 << 62, p.ptr) == 0
    assert not E.download(p, (n,)).any()
    E.close()


SETS = [(2048, Q1, 12289, 2, 3), (4096, Q2, 65537, -37, 1 << 7)]         # (n, q, t, scalar of the noise test, divisor)


@pytest.fixture(scope="module", params=SETS, ids=lambda s: f"n{s[0]}_t{s[2]}")
def pset(request):
    import crcnn_amd as ca
    from oracle import orc
    n, q, t, w, D = request.param
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(5)
    evk = O.gen_evk(6, sk)
    count = 3
    rng = np.random.RandomState(n)
    half = (t - 1) // 2
    v = rng.randint(-half, half + 1, size=(count, n)).astype(np.int64)
    v[0, :6] = [half, -half, 0, D // 2 if D % 2 == 0 else D, -(D // 2) if D % 2 == 0 else -D, 3 * (D // 2)]
    d_pl = E.alloc(count * n * 8)
    E.slots_compose_dev(E.upload(v), count, n, n, 1, d_pl)
    d_ct = E.alloc(count * 2 * E.k * n * 8)
    E.encrypt_dev_forms(E.upload(pk), d_pl, count, 99, ca.COEFF, d_ct, E.alloc(E.encrypt_dev_work_bytes(count)))
    ct = E.download(d_ct, (count, 2, E.k, n))
    yield dict(n=n, q=q, t=t, w=w, D=D, E=E, O=O, sk=sk, pk=pk, evk=evk, count=count, v=v, ct=ct, d_sk=E.upload(sk), d_pk=E.upload(pk))
    E.close()


def _composed(P, ct_in, fin, fout, sym, seed):
    """crc_decrypt_dev -> crc_slots_rescale_dev in place -> crc_encrypt[_sym]_dev_forms: the ciphertexts and the rescaled plaintexts"""
    E, count, n = P["E"], P["count"], P["n"]
    d_in = E.upload(ct_in)
    d_pl = E.alloc(count * n * 8)
    E.decrypt_dev(P["d_sk"], d_in, count, d_pl, E.alloc(E.decrypt_dev_work_bytes(count, 2, fin)), in_form=fin)
    E.slots_rescale_dev(d_pl, count, P["D"], d_pl)
    d_out = E.alloc(ct_in.nbytes)
    if sym:
        E.encrypt_sym_dev_forms(P["d_sk"], d_pl, count, seed, fout, d_out, E.alloc(E.encrypt_sym_dev_work_bytes(count)))
    else:
        E.encrypt_dev_forms(P["d_pk"], d_pl, count, seed, fout, d_out, E.alloc(E.encrypt_dev_work_bytes(count)))
    return E.download(d_out, ct_in.shape), E.download(d_pl, (count, n))


def _refresh(P, ct_in, fin, fout, sym, seed, in_place=False):
    E, count = P["E"], P["count"]
    d_in = E.upload(ct_in)
    d_out = d_in if in_place else E.alloc(ct_in.nbytes)
    if not in_place:
        E.L.crc_memset(E.c, d_out.ptr, 0xff, ct_in.nbytes, E.stream)
    if sym:
        E.slots_refresh_sym_dev(P["d_sk"], d_in, count, P["D"], seed, d_out, E.alloc(E.slots_refresh_sym_dev_work_bytes(count, fin)), in_form=fin, out_form=fout)
    else:
        E.slots_refresh_dev(P["d_sk"], P["d_pk"], d_in, count, P["D"], seed, d_out, E.alloc(E.slots_refresh_dev_work_bytes(count, fin)), in_form=fin, out_form=fout)
    return E.download(d_out, ct_in.shape)


def _in_form(P, ct, form):
    import crcnn_amd as ca
    if form == ca.COEFF:
        return ct
    E = P["E"]
    d = E.upload(ct); E.ntt_fwd(d, P["count"])
    return E.download(d, ct.shape)


@pytest.mark.parametrize("sym", [False, True], ids=["public_key", "secret_key"])
def test_refresh_is_the_three_public_calls(pset, sym):
    import crcnn_amd as ca
    P = pset
    E, n, t, D, count = P["E"], P["n"], P["t"], P["D"], P["count"]
    for fin in (ca.COEFF, ca.NTT):
        ct_in = _in_form(P, P["ct"], fin)
        for fout in (ca.COEFF, ca.NTT):
            want, plain = _composed(P, ct_in, fin, fout, sym, 4242)
            assert np.array_equal(_refresh(P, ct_in, fin, fout, sym, 4242), want), (fin, fout, "out of place")
            assert np.array_equal(_refresh(P, ct_in, fin, fout, sym, 4242, in_place=True), want), (fin, fout, "in place")
            assert not np.array_equal(_refresh(P, ct_in, fin, fout, sym, 4243), want)           # another seed, other ciphertexts
    # what the refreshed ciphertexts decrypt to: the model's integers in every slot
    got_ct = _refresh(P, P["ct"], ca.COEFF, ca.COEFF, sym, 7)
    d_pl = E.alloc(count * n * 8)
    E.decrypt_dev(P["d_sk"], E.upload(got_ct), count, d_pl, E.alloc(E.decrypt_dev_work_bytes(count)))
    d_v = E.alloc(count * n * 8)
    E.slots_decompose_dev(d_pl, count, n, d_v, n, 1)
    got = E.download(d_v, (count, n), dtype=np.int64)
    want_v = [[rm.rescale_value(int(x), D) for x in row] for row in P["v"]]
    assert got.tolist() == want_v
    # refusals of the composed call: a divisor out of range, a form that is no ciphertext form
    d_in = E.upload(P["ct"]); d_w = E.alloc(E.slots_refresh_dev_work_bytes(count, ca.COEFF))
    assert E.L.crc_slots_refresh_sym_dev(E.c, P["d_sk"].ptr, d_in.ptr, count, ca.COEFF, 0, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == -1
    assert E.L.crc_slots_refresh_dev(E.c, P["d_sk"].ptr, P["d_pk"].ptr, d_in.ptr, count, ca.NTTP, 3, 1, ca.COEFF, d_in.ptr, d_w.ptr, None) == -1
    assert E.slots_refresh_dev_work_bytes(count, ca.NTTP) == 0


def test_refresh_restores_the_noise_budget(pset):
    """a tensor that went through multiply_plain_ntt + square_relin: every refreshed ciphertext has more budget than before, and the refreshed tensor is bit for bit
    the composed sequence's"""
    import crcnn_amd as ca
    P = pset
    E, n, t, w, count = P["E"], P["n"], P["t"], P["w"], P["count"]
    d_ct = E.upload(P["ct"]); E.ntt_fwd(d_ct, count)
    d_w = E.alloc(E.k * n * 8); E.plain_to_ntt(E.upload(np.array([[w % t] + [0] * (n - 1)], dtype=np.uint64)), 1, d_w)
    E.multiply_plain_ntt(d_ct, d_w, count, count)
    d_y = E.alloc(P["ct"].nbytes)
    E.square_relin(d_ct, count, E.upload(P["evk"]), d_y, E.alloc(E.square_relin_work_bytes(count)), in_form=ca.NTT, out_form=ca.COEFF)
    y = E.download(d_y, P["ct"].shape)
    before = [E.noise_budget(P["sk"], y[i]) for i in range(count)]
    for sym in (False, True):
        got = _refresh(P, y, ca.COEFF, ca.COEFF, sym, 31)
        want, plain = _composed(P, y, ca.COEFF, ca.COEFF, sym, 31)
        assert np.array_equal(got, want)
        after = [E.noise_budget(P["sk"], got[i]) for i in range(count)]
        print("noise budget before", before, "after", after)
        assert all(a > b for a, b in zip(after, before))
        # what the refreshed tensor holds is checked in both sets: the square must leave something to decrypt (measured: 2 bits of 28 on the one 54-bit modulus
        # with t = 12289 and the scalar 2, 45 of 79 on the two moduli; keys, seeds and values are fixed, so the figures are the same in every run)
        assert min(before) > 0, before
        # the slots: floor(((w v)^2 mod t centred) / D + 1/2)
        H = ca.Engine(n, P["q"], t, device=-1)
        slots = H.slots_decompose(plain, n, n, 1).reshape(count, n)
        H.close()
        half = (t - 1) // 2
        cen = lambda x: (x + half) % t - half
        assert slots.tolist() == [[rm.rescale_value(cen((w * int(x)) ** 2), P["D"]) for x in row] for row in P["v"]]


# (description under tests/golden/slots, its weights, the golden whose ring and moduli the run takes, bits of the slot prime, input_bits, weight_bits).
# PlainModelTiny runs at (4, 5) and the 20-bit prime of the existing whole-network test (divisors 8 and 128).
# approx_poly: a division does not commute with a wrap-around, so t has to carry the values IN FRONT of the rescale, and at a 20-bit modulus the divisors turn
# every slot into 0.  At (4, 5) -- the bits only the rescale line admits -- the exact integer network reaches 48 bits in front of `rescale r 8` behind act1 and
# 50 bits behind pool2, so t needs 50 / 52 bits; the polynomial activation costs about log2 t + 14 bits of noise, and on the approx256 golden's three moduli
# (164 bits) that leaves NO budget in front of the rescale: at a 53-bit prime profile_budget reports 0 bits there and the decrypted slots are not the model's,
# although the refreshed output tensor reports 43 bits.  As the issue provides for that case, weight_bits is lowered, by one, to 4: the values in front of the
# rescale then have 41 bits (behind act1) / 42 bits (behind pool2), the smallest slot prime that carries them has 44 bits, and profile_budget reports 10 / 9 bits
# where the client decrypts (65 / 66 at the output).  Measured beside it: the 46-bit prime leaves 2 / 1 bits there, and weight_bits 3 (35 / 36-bit values) at a
# 40-bit prime 23 / 22 bits.  Seeds are fixed, so these figures do not vary from run to run
NETS = [("tiny_rescale.net", "PlainModelTiny", "tiny256", 20, 4, 5), ("approx_poly_rescale_act1.net", "ApproxPlainModel", "approx256", 44, 4, 4),
        ("approx_poly_rescale_pool2.net", "ApproxPlainModel", "approx256", 44, 4, 4)]


@pytest.mark.parametrize("desc,model,golden,t_bits,in_bits,w_bits", NETS, ids=[n[0] for n in NETS])
def test_networks_with_rescale_layers(desc, model, golden, t_bits, in_bits, w_bits):
    """test_host slots_build: S = 5 images in the slots of ONE encrypted tensor through Network::forward (NTT-resident), unfused and fused, with the client's rescale
    on the device: every image's outputs are the integer model's, the final scale is the ledger's, both output tensors have noise budget left"""
    import subprocess
    import tempfile
    import crcnn_amd as ca
    from crcnn_amd import netrun
    from netcommon import GOLD, load_net_golden, model_weights
    driver = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")
    g = load_net_golden(golden)
    n, S = g["n"], 5
    t = ca.Engine.slots_prime(n, t_bits)
    assert all(t < q for q in g["q"])
    path = os.path.join(SLOTS, desc)
    layers = netrun.load_description(path)
    zd, xd, yd = layers.input_shape
    rng = np.random.RandomState(17)
    images = rng.uniform(-1, 1, size=(S, zd, xd, yd)).astype(np.float32)
    d = tempfile.mkdtemp()
    np.array([n, len(g["q"]), t] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    h5 = os.path.join(GOLD, "models", model + ".h5")
    out = subprocess.run([driver, "slots_build", path, h5, d, str(S), str(in_bits), str(w_bits)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout, out.stderr[-300:])
    assert "describe-ok" in out.stdout and "slots_build ok" in out.stdout
    want, scale = rm.network_forward(list(layers), model_weights(model), images, t, in_bits, w_bits)
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines() if " " in l)
    assert float(lines["slot_scale"]) == float(scale)
    budgets = lines["budget"].split()
    assert int(budgets[1]) > 0 and int(budgets[3]) > 0, lines["budget"]
    for name in ("slots_unfused.i64", "slots_fused.i64"):
        got = np.fromfile(os.path.join(d, name), dtype=np.int64).reshape(S, -1)
        assert got.tolist() == want, name
    assert len({tuple(r) for r in want}) == S
    if model == "ApproxPlainModel":                            # t carries every value: the integers are the quantised network's own, no wrap-around anywhere
        assert want == rm.network_forward(list(layers), model_weights(model), images, 1 << 400, in_bits, w_bits)[0]
    # fuse() still folds on either side of a rescale layer (approx_poly: norm1 into conv2 in front of it, norm2 into fc3 behind it) and nothing across it: the
    # fused network gives the same integers, which a fold that moved a layer over the rounding would not
    import re
    removed = int(re.search(r"fused: (\d+) layers removed", out.stderr).group(1))
    if model == "ApproxPlainModel":
        assert removed >= 2, out.stderr[-300:]


@pytest.mark.parametrize("desc,model,golden,t_bits,in_bits,w_bits", NETS[:2], ids=[n[0] for n in NETS[:2]])
def test_rescale_layers_under_every_forward_plan(desc, model, golden, t_bits, in_bits, w_bits):
    """test_host slots_rescale_plan: the same integers from the NTT-resident forward, a profiled forward timed with events (the layer is timed as a layer, not as
    T_REENC; its producer hands over CRC_NTT; the budget behind it is larger than in front of it), two-level chunking (three tensors as a batch, one image per
    chunk), the layerwise coefficient-form forward and secret-key re-encryption; a packed output form is refused"""
    import subprocess
    import tempfile
    import crcnn_amd as ca
    from crcnn_amd import netrun
    from netcommon import GOLD, load_net_golden
    g = load_net_golden(golden)
    n, S = g["n"], 3
    t = ca.Engine.slots_prime(n, t_bits)
    path = os.path.join(SLOTS, desc)
    zd, xd, yd = netrun.load_description(path).input_shape
    images = np.random.RandomState(23).uniform(-1, 1, size=(S, zd, xd, yd)).astype(np.float32)
    d = tempfile.mkdtemp()
    np.array([n, len(g["q"]), t] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    out = subprocess.run([os.path.join(ROOT, "crcnn_amd", "lib", "test_host"), "slots_rescale_plan", path, os.path.join(GOLD, "models", model + ".h5"), d, str(S),
                          str(in_bits), str(w_bits)], capture_output=True, text=True)
    print(out.stdout, out.stderr[-500:])
    assert out.returncode == 0 and "slots_rescale_plan ok" in out.stdout, out.stderr[-2000:]
    assert out.stdout.count("rescale layer") == (2 if desc.startswith("tiny") else 1)
