"""Slot batching on the GPU: slots_compose_kernel / slots_decompose_kernel (crc_slots_compose_dev / crc_slots_decompose_dev) bit for bit against their host twins
-- which tests/test_slots_cpu.py holds against the integer model --, a batch through encryption, plaintext multiply, square + relinearise and add_plain against
the slot-wise integers, and the evaluator's prime-t paths (every recorded vector of the suite has a power-of-two t) against the CPU oracle's ciphertexts."""
import numpy as np
import pytest

import slots_model as sm

pytestmark = pytest.mark.gpu
Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
BIG = 0x7fffffff380001                            # 55 bits: above 2^53, still the lazy butterflies
FILL = -0x0101010101010102                        # int64 of the bytes 0xfe: marks words a kernel must not write
SETS = [(2048, Q1, 12289, 2), (4096, Q2, 65537, -37)]       # (n, q, t, scalar): the scalar at (2048, one modulus) leaves about 2 bits of budget, any larger none


def values_for(t, count, slots, seed):
    rng = np.random.RandomState(seed)
    half = (t - 1) // 2
    return np.array([[int(rng.randint(0, 1 << 62)) % t - half for _ in range(slots)] for _ in range(count)], dtype=np.int64)


def ring_cases():
    import crcnn_amd as ca
    out = [(n, ca.Engine.slots_prime(n, 30)) for n in (256, 2048, 4096, 8192)]           # one LDS pass; 3 + 2 stages... : every pass structure of the row transform
    return out + [(256, BIG), (256, ca.Engine.slots_prime(256, 60)), (64, 257), (16384, ca.Engine.slots_prime(16384, 50))]


@pytest.mark.parametrize("case", range(8))
def test_device_compose_decompose_equal_the_host_twin(case):
    import crcnn_amd as ca
    n, t = ring_cases()[case]
    E = ca.Engine(n, Q1, t, device=0)
    H = ca.Engine(n, Q1, t, device=-1)
    assert E.slots_supported
    count = 3
    i64 = np.iinfo(np.int64)
    for S in (5, n):
        v = values_for(t, count, S, 31 * n + S)
        v[0, :5] = [i64.min, i64.max, -1, t, -t - 3]                               # any int64 is its residue
        want = H.slots_compose(v, count, S, S, 1)
        for layout, (istr, sstr) in {"item-major": (S, 1), "image-major": (1, count)}.items():
            src = v if istr == S else np.ascontiguousarray(v.T)
            d_v = E.upload(src)
            d_p = E.alloc(want.nbytes); E.L.crc_memset(E.c, d_p.ptr, 0xff, want.nbytes, E.stream)
            E.slots_compose_dev(d_v, count, S, istr, sstr, d_p)
            assert np.array_equal(E.download(d_p, want.shape), want), (n, t, S, layout, "compose")
            # decompose of arbitrary plaintext words (not only composed ones), S slots written and nothing else
            rng = np.random.RandomState(case * 7 + S)
            plain = (rng.randint(0, 1 << 62, size=(count, n)).astype(np.uint64) % np.uint64(t)).astype(np.uint64)
            plain[0] = want[0]
            size = count * S + 8
            back = H.slots_decompose(plain, S, istr, sstr, size=size)
            d_o = E.upload(np.full(size, FILL, dtype=np.int64))
            E.slots_decompose_dev(E.upload(plain), count, S, d_o, istr, sstr)
            got = E.download(d_o, (size,), dtype=np.int64)
            assert np.array_equal(got[:count * S], back[:count * S]) and (got[count * S:] == FILL).all(), (n, t, S, layout, "decompose")
    E.close(); H.close()


def test_device_refusals():
    import crcnn_amd as ca
    n = 2048
    E = ca.Engine(n, Q1, 1 << 20, device=0)
    d = E.alloc(n * 8)
    for call in (lambda s: E.L.crc_slots_compose_dev(E.c, d.ptr, 1, s, n, 1, d.ptr, None), lambda s: E.L.crc_slots_decompose_dev(E.c, d.ptr, 1, s, d.ptr, n, 1, None)):
        assert call(n) == -2 and call(0) == -2
    E.close()
    E = ca.Engine(n, Q1, 12289, device=0)
    d = E.alloc(n * 8); p = E.alloc(n * 8)
    assert E.L.crc_slots_compose_dev(E.c, d.ptr, 1, 0, n, 1, p.ptr, None) == -1 and E.L.crc_slots_compose_dev(E.c, d.ptr, 1, n + 1, n, 1, p.ptr, None) == -1
    assert E.L.crc_slots_compose_dev(E.c, d.ptr, 1, n, 0, 1, p.ptr, None) == -1 and E.L.crc_slots_decompose_dev(E.c, p.ptr, 1, n, d.ptr, n, 0, None) == -1
    assert E.L.crc_slots_compose_dev(E.c, None, 1, n, n, 1, p.ptr, None) == -1 and E.L.crc_slots_decompose_dev(E.c, p.ptr + 8, 1, n, d.ptr, n, 1, None) == -1
    assert E.L.crc_slots_compose_dev(E.c, d.ptr, 0, n, n, 1, p.ptr, None) == 0                # an empty batch is no error
    E.close()


@pytest.fixture(scope="module", params=SETS, ids=lambda s: f"n{s[0]}_t{s[2]}")
def pset(request):
    import crcnn_amd as ca
    from oracle import orc
    n, q, t, w = request.param
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(5)
    evk = O.gen_evk(6, sk)
    yield n, q, t, w, E, O, sk, pk, evk
    E.close()


def test_batch_through_encryption_square_and_add(pset):
    """compose_dev -> crc_encrypt_dev_forms(NTT) -> multiply_plain_ntt by a scalar -> square + relinearise -> add_plain -> decrypt_dev -> decompose_dev: (w v)^2 + c in
    every slot of every ciphertext, image-major input and output"""
    import crcnn_amd as ca
    n, q, t, w, E, O, sk, pk, evk = pset
    count, S, c = 3, n, 1234
    v = values_for(t, S, count, 5)                                                 # [S][count]: image-major, as a client holds a batch
    d_pl = E.alloc(count * n * 8)
    E.slots_compose_dev(E.upload(v), count, S, 1, count, d_pl)
    d_ct = E.alloc(count * 2 * E.k * n * 8)
    E.encrypt_dev_forms(E.upload(pk), d_pl, count, 99, ca.NTT, d_ct, E.alloc(E.encrypt_dev_work_bytes(count)))
    scal = lambda x: np.array([[x % t] + [0] * (n - 1)], dtype=np.uint64)          # the constant polynomial: x in every slot
    d_w = E.alloc(E.k * n * 8); E.plain_to_ntt(E.upload(scal(w)), 1, d_w)
    d_c = E.alloc(E.k * n * 8); E.plain_to_delta(E.upload(scal(c)), 1, ca.COEFF, d_c)
    E.multiply_plain_ntt(d_ct, d_w, count, count)
    d_y = E.alloc(count * 2 * E.k * n * 8)
    E.square_relin(d_ct, count, E.upload(evk), d_y, E.alloc(E.square_relin_work_bytes(count)), in_form=ca.NTT, out_form=ca.COEFF)
    E.add_plain(d_y, d_c, count, count)
    y = E.download(d_y, (count, 2, E.k, n))
    budgets = [E.noise_budget(sk, y[i]) for i in range(count)]
    print("noise budget left:", budgets)
    assert min(budgets) > 0
    E.decrypt_dev(E.upload(sk), d_y, count, d_pl, E.alloc(E.decrypt_dev_work_bytes(count)))
    d_o = E.alloc(v.nbytes)
    E.slots_decompose_dev(d_pl, count, S, d_o, 1, count)
    got = E.download(d_o, v.shape, dtype=np.int64)
    want = np.array([[sm.centre((w * int(x)) ** 2 + c, t) for x in row] for row in v], dtype=np.int64)
    assert np.array_equal(got, want)


def test_prime_t_square_and_multiply_equal_the_oracle(pset):
    """crc_square_relin_forms and crc_multiply at a PRIME plain modulus, on the default kernels and on the reference-order ones (sq_path / relin_path 1): the
    oracle's relinearize(square(x)), the oracle's square for multiply(x, x), the integer model of Evaluator::multiply for multiply(x, y)"""
    import crcnn_amd as ca
    from bfv_multiply_model import MultiplyModel
    n, q, t, w, E, O, sk, pk, evk = pset
    H = ca.Engine(n, q, t, device=-1)
    count = 2
    x = H.encrypt(pk, H.slots_compose(values_for(t, count, n, 8), count, n, n, 1), 400)
    H.close()
    sq3 = np.stack([O.square(x[i]) for i in range(count)])
    relin = np.stack([O.relinearize(sq3[i], evk) for i in range(count)])
    y = np.ascontiguousarray(x[::-1])
    prod = MultiplyModel(O).multiply(x[0], y[0])
    d_x, d_y, d_evk = E.upload(x), E.upload(y), E.upload(evk)
    d_o = E.alloc(x.nbytes); d_o3 = E.alloc(sq3.nbytes)
    d_work = E.alloc(max(E.square_relin_work_bytes(count), E.multiply_relin_work_bytes(count)))
    try:
        for path in (0, 1):
            E.set_tuning("sq_path", path); E.set_tuning("relin_path", path)
            for fin, fout in ((ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT)):
                d_in = E.upload(x)
                if fin == ca.NTT:
                    E.ntt_fwd(d_in, count)
                E.L.crc_memset(E.c, d_o.ptr, 0xff, x.nbytes, E.stream)
                E.square_relin(d_in, count, d_evk, d_o, d_work, in_form=fin, out_form=fout)
                if fout == ca.NTT:
                    E.ntt_inv(d_o, count)
                assert np.array_equal(E.download(d_o, x.shape), relin), (path, fin, fout, "square_relin")
            E.L.crc_memset(E.c, d_o3.ptr, 0xff, sq3.nbytes, E.stream)
            E.multiply(d_x, d_x, count, d_o3, d_work)
            assert np.array_equal(E.download(d_o3, sq3.shape), sq3), (path, "multiply(x, x)")
            E.L.crc_memset(E.c, d_o3.ptr, 0xff, sq3.nbytes, E.stream)
            E.multiply(d_x, d_y, count, d_o3, d_work)
            assert np.array_equal(E.download(d_o3, sq3.shape)[0], prod), (path, "multiply(x, y)")
    finally:
        E.set_tuning("sq_path", 0); E.set_tuning("relin_path", 0)


# (model description, its weights, the golden whose ring and moduli the run takes, input_bits, weight_bits).  The bits are what the scale ledger admits for the
# description (approx_poly at (4, 5) would pass 2^62 at fc4) and leave noise budget at these moduli: weights below 2^weight_bits cost about weight_bits +
# log2(taps) bits per linear layer -- 37 + 4 w of the about 80 bits PlainModelTiny starts with, 67 + 7 w of approx_poly's about 135
# (the same forwards on the CPU oracle, scalar plaintexts and sum pools, left 44 bits for PlainModelTiny at (4, 5) and 69 for ApproxPlainModel -- approx_poly with
# a square in place of its polynomial -- at (3, 4), with the integer model's outputs in every slot: weight_bits did not have to be lowered)
NETS = [("PlainModelTiny", "PlainModelTiny", "tiny256", 4, 5), ("approx_poly.net", "ApproxPlainModel", "approx256", 3, 4)]


@pytest.mark.parametrize("desc,model,golden,in_bits,w_bits", NETS, ids=[n[0] for n in NETS])
def test_whole_network_on_five_images_per_ciphertext(desc, model, golden, in_bits, w_bits):
    """test_host slots_build: S = 5 distinct images in the slots of ONE encrypted tensor through Network::forward, unfused and fused: every image's outputs are the
    integer network's mod t (exact whether or not a value wraps), and the output tensors have noise budget left"""
    import os
    import subprocess
    import tempfile
    import crcnn_amd as ca
    from crcnn_amd import netrun
    from netcommon import GOLD, load_net_golden, model_weights
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "test_host")
    g = load_net_golden(golden)
    n, S = g["n"], 5
    t = ca.Engine.slots_prime(n, 20)
    assert all(t < q for q in g["q"])
    path = desc if not desc.endswith(".net") else os.path.join(GOLD, "activations", desc)
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
    print(out.stdout)
    assert "describe-ok" in out.stdout and "slots_build ok" in out.stdout
    want, scale = sm.network_forward(list(layers), model_weights(model), images, t, in_bits, w_bits)
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines() if " " in l)
    assert float(lines["slot_scale"]) == float(scale)
    budgets = lines["budget"].split()
    assert int(budgets[1]) > 0 and int(budgets[3]) > 0, lines["budget"]
    for name in ("slots_unfused.i64", "slots_fused.i64"):
        got = np.fromfile(os.path.join(d, name), dtype=np.int64).reshape(S, -1)
        assert got.tolist() == want, name
    assert len({tuple(r) for r in want}) == S                                      # five different images, five different rows
