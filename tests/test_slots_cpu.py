"""Slot batching on the host (crc_slots_supported / crc_slots_prime / crc_slots_compose / crc_slots_decompose on a host-only context) against tests/slots_model.py:
slots are evaluations of the plaintext polynomial at psi^(+-3^i) in Python integers, nothing shared with the engine's transforms or index map.  No GPU."""
import numpy as np
import pytest

import slots_model as sm

Q1 = [0x3fffffff000001]                           # 1 mod 2^24: a coefficient modulus for every ring here
Q2 = [0x7fffffff380001, 0x3fffffff000001]
BIG = 0x7fffffff380001                            # a SEAL default modulus of the larger rings as plain modulus: 55 bits, above 2^53
CASES = [(64, 257), (256, 7681), (1024, 12289), (256, BIG)]
PARAMETERS, INVALID = -2, -1


def engine(n, t, q=None):
    import crcnn_amd as ca
    return ca.Engine(n, q or Q1, t, device=-1)


def strict_prime(n=256):
    import crcnn_amd as ca
    return ca.Engine.slots_prime(n, 60)           # above 2^57: the strict butterflies on the device, the same host transform


def values_for(t, count, slots, seed):
    rng = np.random.RandomState(seed)
    half = (t - 1) // 2
    return np.array([[int(rng.randint(0, 1 << 62)) % t - half for _ in range(slots)] for _ in range(count)], dtype=np.int64)


@pytest.mark.parametrize("n,t", CASES + [(256, None)], ids=lambda v: str(v))
def test_compose_decompose_equal_the_model(n, t):
    t = t or strict_prime()
    E = engine(n, t)
    assert E.slots_supported
    assert int(E.table("slots_root")[0]) == sm.minimal_root(n, t)
    idx = E.table("slots_index_map")
    assert sorted(int(i) for i in idx) == list(range(n))
    v = values_for(t, 1, n, n)
    p = E.slots_compose(v, 1, n, n, 1)
    assert p.max() < t
    # the model evaluates the composed polynomial at the slot points: the values come back
    assert sm.decompose([int(c) for c in p[0]], n, t) == [int(x) for x in v[0]]
    # ... and decompose of an arbitrary plaintext is its evaluations
    rng = np.random.RandomState(n + 1)
    r = np.array([int(rng.randint(0, 1 << 62)) % t for _ in range(n)], dtype=np.uint64)
    assert [int(x) for x in E.slots_decompose(r[None], n, n, 1)] == sm.decompose([int(c) for c in r], n, t)
    if n <= 256:                                  # the model's own interpolation gives the same coefficients
        assert [int(c) for c in p[0]] == sm.compose([int(x) for x in v[0]], n, t)
    E.close()


@pytest.mark.parametrize("n,t", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("slots", [1, 5, 0], ids=["S1", "S5", "Sn"])
def test_round_trip_and_strides(n, t, slots):
    """S = 1, 5, n; item-major (S, 1) and image-major (1, count) layouts carry the same numbers; slots past S are zero; decompose writes S slots only"""
    S = slots or n
    E = engine(n, t)
    count = 3
    v = values_for(t, count, S, 7 * n + S)                     # [count][S]: item-major
    p = E.slots_compose(v, count, S, S, 1)
    assert np.array_equal(E.slots_compose(np.ascontiguousarray(v.T), count, S, 1, count), p)
    back = E.slots_decompose(p, S, S, 1)
    assert np.array_equal(back.reshape(count, S), v)
    assert np.array_equal(E.slots_decompose(p, S, 1, count).reshape(S, count), v.T)
    full = E.slots_decompose(p, n, n, 1).reshape(count, n)
    assert np.array_equal(full[:, :S], v) and not full[:, S:].any()
    if S == 5:                                                # first row against the model
        assert sm.decompose([int(c) for c in p[0]], n, t, S) == [int(x) for x in v[0]]
        guard = E.slots_decompose(p, S, n, 1, size=count * n).reshape(count, n)      # slot_stride 1, item_stride n: words past S stay untouched
        assert np.array_equal(guard[:, :S], v) and not guard[:, S:].any()
    E.close()


@pytest.mark.parametrize("t", [7681, BIG], ids=["t7681", "t55bit"])
def test_any_int64_reduces_to_its_residue(t):
    n = 256
    E = engine(n, t)
    i64 = np.iinfo(np.int64)
    raw = [-1, (t - 1) // 2, -((t - 1) // 2), t, -t - 3, i64.min, i64.max, 0, (t + 1) // 2]
    v = np.array([raw], dtype=np.int64)
    got = E.slots_decompose(E.slots_compose(v, 1, len(raw), len(raw), 1), len(raw), len(raw), 1)
    assert [int(x) for x in got] == [sm.centre(x, t) for x in raw]
    E.close()


def test_refusals():
    import crcnn_amd as ca
    n = 256
    one = np.ones(n, dtype=np.int64); pl = np.zeros((1, n), dtype=np.uint64)

    def status(E, slots=n, item_stride=n, slot_stride=1, values=one, plain=pl):
        import ctypes
        vp = values.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if values is not None else None
        pp = plain.ctypes.data_as(ca.binding.PU) if plain is not None else None
        a = E.L.crc_slots_compose(E.c, vp, 1, slots, item_stride, slot_stride, pp)
        b = E.L.crc_slots_decompose(E.c, pp, 1, slots, vp, item_stride, slot_stride)
        assert a == b
        return a
    # t = 2^20; t prime but not 1 mod 2n; t equal to a q_i is refused by the context itself, t equal to an fp64 prime of the key switch by the slot check
    for t in (1 << 20, 7687, 257):
        E = engine(n, t)
        assert not E.slots_supported and status(E) == PARAMETERS and status(E, slots=0) == PARAMETERS
        with pytest.raises(ca.binding.CrcError):
            E.table("slots_root")
        E.close()
    with pytest.raises(ca.binding.CrcError):
        engine(n, Q1[0])
    G = engine(n, 7681)
    f64 = [int(p) for p in G.table("f64_primes")]
    E = engine(n, f64[0])
    assert f64[0] % (2 * n) == 1 and not E.slots_supported and status(E) == PARAMETERS
    E.close()
    assert G.slots_supported and status(G) == 0
    assert status(G, slots=0) == INVALID and status(G, slots=n + 1) == INVALID
    assert status(G, item_stride=0) == INVALID and status(G, slot_stride=0) == INVALID
    assert status(G, values=None) == INVALID and status(G, plain=None) == INVALID
    G.close()


def test_slots_prime_equals_brute_force():
    import crcnn_amd as ca
    for bits in range(14, 25):
        assert ca.Engine.slots_prime(256, bits) == sm.slots_prime(256, bits), bits
    assert ca.Engine.slots_prime(1024, 14) == 12289 and ca.Engine.slots_prime(4096, 17) == sm.slots_prime(4096, 17) == 114689
    with pytest.raises(ca.binding.CrcError):
        ca.Engine.slots_prime(256, 61)
    with pytest.raises(ca.binding.CrcError):
        ca.Engine.slots_prime(256, 9)             # no number below 2^9 is 1 mod 512 and larger than 512


def test_slotwise_homomorphism_on_the_cpu():
    """compose -> crc_encrypt -> the oracle's multiply_plain by a scalar, square, relinearize, add_plain -> crc_decrypt -> decompose == (w v)^2 + c in every slot"""
    from oracle import orc
    n, t = 256, 7681
    E = engine(n, t, Q2)
    O = orc.Oracle(n, Q2, t)
    sk, pk = O.keygen(5); evk = O.gen_evk(6, sk)
    S, w, c = n, -37, 1234
    v = values_for(t, 2, S, 99)
    plains = E.slots_compose(v, 2, S, S, 1)
    cts = E.encrypt(pk, plains, 1000)
    scal = lambda x: np.array([x % t] + [0] * (n - 1), dtype=np.uint64)          # a constant polynomial: the same number in every slot
    out = []
    for ct in cts:
        y = O.multiply_plain(ct, scal(w))
        y = O.relinearize(O.square(y), evk)
        y = O.add_plain(y, scal(c))
        assert O.noise_budget(sk, y) > 0
        out.append(y)
    dec = E.decrypt(sk, np.stack(out))
    got = E.slots_decompose(dec, S, S, 1).reshape(2, S)
    want = [[sm.centre((w * int(x)) ** 2 + c, t) for x in row] for row in v]
    assert got.tolist() == want
    E.close()


def _driver():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "crcnn_amd", "lib", "test_host")


def _descriptions():
    import glob
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activations")
    return ["PlainModelTiny", "ApproxPlainModel", "PlainModelWoPad"] + sorted(glob.glob(os.path.join(gold, "*.net")))


@pytest.mark.parametrize("desc", _descriptions(), ids=lambda p: p.split("/")[-1])
@pytest.mark.parametrize("bits", [(4, 5), (3, 4), (0, 0), (8, 7)], ids=str)
def test_slots_describe_prints_the_models_ledger(desc, bits):
    """`test_host slots_describe` (no GPU): the scale in front of every layer and the final one equal the model's ledger; a ledger that leaves the exact integers
    below 2^62 is refused with the line of the layer that does it"""
    import subprocess
    from crcnn_amd import netrun
    layers = netrun.load_description(desc)
    out = subprocess.run([_driver(), "slots_describe", desc, str(bits[0]), str(bits[1])], capture_output=True, text=True)
    try:
        want = sm.ledger(list(layers), *bits)
    except ValueError:
        assert out.returncode != 0 and "line " in out.stderr and "scale" in out.stderr
        return
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    assert [(r[2], r[3]) for r in rows[:-1]] == [(k, nm) for k, nm, _ in layers]
    assert [float(r[4]) for r in rows[:-1]] + [float(rows[-1][1])] == [float(s) for s in want] and rows[-1][0] == "slot_scale"


def test_slots_describe_refuses_a_refresh(tmp_path):
    import subprocess
    text = "input 1 6 6\nconv c stride 1 1 filter 3 3 filters 2\nsquare act\nrefresh\nfc f 3\n"
    p = tmp_path / "refresh.net"
    p.write_text(text)
    out = subprocess.run([_driver(), "slots_describe", str(p), "4", "5"], capture_output=True, text=True)
    assert out.returncode != 0 and "line 4: refresh" in out.stderr
    p.write_text(text.replace("refresh\n", ""))
    assert subprocess.run([_driver(), "slots_describe", str(p), "4", "5"], capture_output=True, text=True).returncode == 0


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/slots_kernel_check.cpp: the bodies of slots_compose_kernel / slots_decompose_kernel (csrc/slots_device.h) run on the CPU, one thread per workgroup,
    with the address and undefined-behaviour sanitizers, equal the host twins bit for bit -- every pass structure of the row transform (n = 64 .. 16384), a 13-bit,
    a 30-bit, a 55-bit (lazy butterflies) and a 60-bit (strict) plain modulus, S = 5 and n, both layouts, buffers of exactly the size the strides reach"""
    import os
    import subprocess
    import tempfile
    import crcnn_amd as ca
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "slots_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "tests", "cpp", "hipstub"), "-I", os.path.join(root, "crcnn_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "slots_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    p30 = {n: ca.Engine.slots_prime(n, 30) for n in (2048, 4096, 8192)}
    cases = [(64, 257, 5, 0), (64, 257, 64, 1), (256, 7681, 256, 0), (256, BIG, 5, 1), (256, BIG, 256, 0), (256, strict_prime(), 256, 1), (256, strict_prime(), 5, 0),
             (1024, 12289, 1, 1), (2048, 12289, 2048, 1), (2048, p30[2048], 5, 0), (4096, 65537, 4096, 0), (4096, p30[4096], 5, 1), (8192, p30[8192], 8192, 0),
             (8192, p30[8192], 5, 1), (16384, ca.Engine.slots_prime(16384, 50), 16384, 1)]
    for n, t, S, layout in cases:
        out = subprocess.run([exe, str(n), str(t), str(S), str(layout)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, t, S, layout, out.stdout, out.stderr[-1500:])


def test_the_integer_network_model_is_what_the_oracle_computes_slotwise():
    """the reference the GPU network test compares with, held against the CPU oracle on a small network (conv, average pooling as the sum pool, batch norm, square,
    dense; synthetic weights): three images in the slots of one encrypted tensor, scalar plaintexts at the ledger's scales, the oracle's layer loops -- the decrypted
    slots are slots_model.network_forward's integers mod t for every image, and noise budget is left"""
    from oracle import orc
    from crcnn_amd import netrun
    n, t, S, ib, wb = 256, 7681, 3, 3, 4
    text = "input 1 6 6\nconv c stride 1 1 filter 3 3 filters 2\navgpool p stride 2 2 window 2 2\nbn b\nsquare act\nfc f 3\n"
    layers = netrun.parse_description(text)
    rng = np.random.RandomState(4)
    W = {"c.weight": rng.normal(0, 0.5, 18).astype(np.float32), "c.bias": rng.normal(0, 0.2, 2).astype(np.float32),
         "b.running_mean": rng.normal(0, 0.3, 2).astype(np.float32), "b.running_var": rng.uniform(0.5, 2, 2).astype(np.float32),
         "f.weight": rng.normal(0, 0.5, 3 * 8).astype(np.float32), "f.bias": rng.normal(0, 0.2, 3).astype(np.float32)}
    images = rng.uniform(-1, 1, size=(S, 1, 6, 6)).astype(np.float32)
    want, scale = sm.network_forward(list(layers), W, images, t, ib, wb)
    scales = sm.ledger(list(layers), ib, wb)
    assert scale == scales[-1] == (((1 << ib) * 16 * 4 * 16) ** 2) * 16
    E = engine(n, t, Q2)
    O = orc.Oracle(n, Q2, t)
    sk, pk = O.keygen(1); evk = O.gen_evk(2, sk)
    pixels = np.rint(images.astype(np.float64) * (1 << ib)).astype(np.int64).reshape(S, -1)
    x = E.encrypt(pk, E.slots_compose(pixels, 36, S, 1, 36), 500).reshape(1, 6, 6, 2, O.k, n)

    def scal(vals, s):
        v = sm.quantise(np.asarray(vals, dtype=np.float32), s) % t
        out = np.zeros(v.shape + (n,), dtype=np.uint64); out[..., 0] = v.astype(np.uint64)
        return out
    Wq = 1 << wb
    y = O.conv(x, O.plains_to_ntt(scal(W["c.weight"].reshape(2, 1, 3, 3), Wq)), scal(W["c.bias"], scales[0] * Wq), 1, 1)
    y = O.pool(y, 2, 2, 2, 2)
    y = O.bn(y, scal(W["b.running_mean"], scales[2]), scal(np.float32(1.0 / np.sqrt(W["b.running_var"].astype(np.float64) + 0.00001)), Wq))
    y = O.square_layer(np.asarray(y), evk)
    flat = np.ascontiguousarray(y).reshape(8, 1, 1, 2, O.k, n)
    y = np.asarray(O.conv(flat, O.plains_to_ntt(scal(W["f.weight"].reshape(3, 8, 1, 1), Wq)), scal(W["f.bias"], scales[4] * Wq), 1, 1)).reshape(3, 2, O.k, n)
    assert min(O.noise_budget(sk, c) for c in y) > 0
    got = E.slots_decompose(E.decrypt(sk, y), S, 1, 3).reshape(S, 3)
    assert got.tolist() == want
    E.close()
