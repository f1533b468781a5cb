"""The packed convolution over slots on the host: the planner against a direct integer convolution (with and without the pool fold), its valid-position list, its
refusals, the weight packing against the constant row's definition, the C++ planner against the Python one, the integer model through encryption at the small
ring, and the work-space size."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conv_slots_model as cm
import galois_hoisted_model as hm
import galois_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ops_n256_k2_t20.npz")
T = 65537
# (M, dil, pool) for the 8 x 8 plane at pitch 8 with a 3 x 3 window: dilation 2 needs 2 . 63 < M
CASES = [(64, 1, 1), (64, 1, 2), (128, 1, 1), (128, 1, 2), (128, 2, 1), (128, 2, 2)]


def layer(seed, Cout=2, Cin=2, H=8, W=8, fh=3, fw=3):
    rng = np.random.RandomState(seed)
    w = rng.randint(-(T // 2), T // 2 + 1, size=(Cout, Cin, fh, fw)).astype(np.int64)
    w[0, 0, 0, 0] = T - 1
    return rng.randint(0, T, size=(Cin, H, W)).astype(np.int64), w, rng


@pytest.mark.parametrize("M,dil,pool", CASES)
def test_plan_against_the_integer_convolution(M, dil, pool):
    """planes tiled with period M over both slot rows, zeros elsewhere: the plan's taps with the folded weights give, at the valid slots of every period, the
    'valid' convolution followed by the pool x pool sum pool, mod t; the geometry is the one the next layer takes"""
    import crcnn_amd as ca
    n = 4 * M
    img, w, _ = layer(M + 10 * dil + pool)
    plan = ca.binding.conv_slots_plan(n, M, 8, 8, 8, 3, 3, dil, pool)
    e = 3 + pool - 1
    assert plan.steps == [dil * (a * 8 + b) for a in range(e) for b in range(e)] and len(set(plan.steps)) == e * e
    assert plan.elements == [gm.elt_rows(n, s) for s in plan.steps] and plan.elements[0] == 1
    assert (plan.out_h, plan.out_w, plan.out_dil) == (6 // pool, 6 // pool, dil * pool)
    assert plan.valid == [dil * pool * (y * 8 + x) for y in range(6 // pool) for x in range(6 // pool)]
    wf = plan.fold(w, T)
    assert wf.shape == (2, 2, e * e) and wf.dtype == np.int64 and (wf >= 0).all() and (wf < T).all()
    if pool == 1:
        assert np.array_equal(wf, (w % T).reshape(2, 2, 9))
    planes = [cm.plane_slots(img[ci], n, M, 8, dil) for ci in range(2)]
    got = cm.conv_plan_slots(plan, wf, planes, T)
    want = cm.conv_direct(img, w, pool, T)
    for base in range(0, n, M):
        for co in range(2):
            assert [int(got[co][base + s]) for s in plan.valid] == [int(v) for v in want[co].reshape(-1)], (base, co)


@pytest.mark.parametrize("M,dil,pool", CASES)
def test_the_valid_list_is_exactly_where_the_plan_is_the_convolution(M, dil, pool):
    """random junk in every slot that holds no pixel.  The convolution is taken with its anchor at EVERY pixel the output grid could name -- (pool Y, pool X)
    inside the plane, the image zero beyond its edge -- so it has a value at each such slot; the plan agrees with it at the valid slots and nowhere else (beyond
    them a tap reads junk, or the next row's pixels at pitch = W, where the convolution reads zero).  A slot that is no such anchor has no value to agree with"""
    import crcnn_amd as ca
    n = 2 * M
    img, w, rng = layer(3 * M + 7 * dil + pool)
    plan = ca.binding.conv_slots_plan(n, M, 8, 8, 8, 3, 3, dil, pool)
    wf = plan.fold(w, T)
    pad = np.zeros((2, 8 + 3 + pool, 8 + 3 + pool), dtype=np.int64)
    pad[:, :8, :8] = img
    full = cm.conv_direct(pad, w, 1, T)                                  # anchor (y, x) for every y, x < 8 + pool
    agree = None
    for _ in range(2):                                                  # two junk fills: agreement that holds by accident in one does not in the other
        planes = [cm.plane_slots(img[ci], n, M, 8, dil, junk=rng.randint(0, T, size=M)) for ci in range(2)]
        got = cm.conv_plan_slots(plan, wf, planes, T)
        here = set()
        for Y in range((8 + pool - 1) // pool):
            for X in range((8 + pool - 1) // pool):
                s = dil * pool * (Y * 8 + X)
                want = [sum(int(full[co, pool * Y + u, pool * X + v]) for u in range(pool) for v in range(pool)) % T for co in range(2)]
                if s < M and all(int(got[co][s]) == want[co] and int(got[co][s + M]) == want[co] for co in range(2)):
                    here.add(s)
        agree = here if agree is None else agree & here
    assert agree == set(plan.valid)


def test_refusals():
    import crcnn_amd as ca
    f = ca.binding.conv_slots_plan
    f(256, 64, 8, 8, 8, 3, 3)                                           # the call the refusals vary
    for bad in (dict(M=48), dict(M=0), dict(M=256), dict(M=32),         # not a power of two, none, above n/2, the plane does not fit
                dict(dil=2), dict(pitch=7), dict(pitch=9),              # 2 . 63 >= 64; W > pitch; 7 . 9 + 7 >= 64
                dict(fh=9), dict(fw=9), dict(pool=7), dict(H=0), dict(W=0), dict(fh=0), dict(fw=0), dict(dil=0), dict(pool=0), dict(pitch=0), dict(n=100)):
        a = dict(n=256, M=64, pitch=8, H=8, W=8, fh=3, fw=3, dil=1, pool=1)
        a.update(bad)
        with pytest.raises(ValueError):
            f(**a)
    # (a step >= n/2 is refused too, but no call reaches that check alone: a window that leaves an output lies inside the plane, and the plane inside M <= n/2)
    assert f(64, 32, 5, 6, 5, 6, 5, 1, 1).steps[-1] == 29 and f(64, 32, 5, 6, 5, 5, 4, 1, 2).steps[-1] == 29
    plan = f(256, 64, 8, 8, 8, 3, 3)
    with pytest.raises(ValueError):
        plan.fold(np.zeros((2, 2, 3, 2), dtype=np.int64), T)
    E = ca.Engine(256, [0x3fffffff000001], T, device=-1)
    p2 = E.conv_slots_plan(64, 8, 8, 8, 3, 3, pool=2)
    assert p2.steps == f(256, 64, 8, 8, 8, 3, 3, 1, 2).steps and p2.n == 256
    E.close()


@pytest.mark.parametrize("q,t", [([0x7fffffff380001, 0x3fffffff000001], T), ([0x3fffffff000001], 12289), ([0xffffffffffc0001, 1073479681], (1 << 30) + 3)],
                         ids=["t65537_k2", "t12289_k1", "t_above_a_modulus"])
def test_pack_weights_is_the_constant_rows_word(q, t):
    """w = 0, 1, (t - 1) / 2, (t + 1) / 2, t - 1, -1 and the int64 extremes: c = w mod t in [0, t), then c >= (t + 1) / 2 ? c + q_i - t : c (mod q_i) -- what
    crc_plain_to_ntt puts at every position of the row of the constant plaintext c"""
    import crcnn_amd as ca
    n = 256
    E = ca.Engine(n, q, t, device=-1)
    ws = [0, 1, (t - 1) // 2, (t + 1) // 2, t - 1, -1, -t, t, t + 1, -(t // 2), np.iinfo(np.int64).max, np.iinfo(np.int64).min, 123456789012345]
    got = E.conv_slots_pack_weights(np.array(ws, dtype=np.int64).reshape(1, -1))
    assert got.shape == (len(q), 1, len(ws)) and got.dtype == np.uint64
    for i, qi in enumerate(q):
        assert [int(v) for v in got[i, 0]] == [cm.lift(w, t, qi) for w in ws], i
        assert all(int(v) < qi for v in got[i, 0])
    if min(q) > t:                                                      # ... and through the oracle's own transform of the constant plaintext
        from oracle import orc
        O = orc.Oracle(n, q, t)
        plains = np.zeros((len(ws), n), dtype=np.uint64)
        plains[:, 0] = [int(w) % t for w in ws]
        rows = O.plains_to_ntt(plains).reshape(len(ws), len(q), n)
        for j in range(len(ws)):
            for i in range(len(q)):
                assert (rows[j, i] == got[i, 0, j]).all(), (j, i)
    assert E.conv_slots_pack_weights(np.zeros((0,), dtype=np.int64)).shape == (len(q), 0)
    E.close()


def test_cpp_planner_equals_the_python_planner():
    """tests/cpp/conv_slots_plan_check.cpp (address and undefined-behaviour sanitizers) prints crc_conv_slots_plan and crc_conv_slots_fold for the cases of a file;
    inside it checks that a refusal writes nothing"""
    import crcnn_amd as ca
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "conv_slots_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "conv_slots_plan_check.cpp"), "-o", exe])
    rng = np.random.RandomState(5)
    cases = []
    for M, dil, pool in CASES:
        cases.append((4 * M, M, 8, 8, 8, 3, 3, dil, pool, 2, 2, T))
    cases += [(8192, 256, 14, 12, 12, 3, 3, 1, 2, 3, 1, T), (8192, 256, 14, 5, 5, 3, 3, 2, 1, 2, 3, 12289), (64, 32, 5, 6, 5, 6, 5, 1, 1, 1, 1, 2),
              (4096, 1024, 28, 28, 28, 5, 5, 1, 2, 2, 1, (1 << 61) - 1)]
    bad = [(256, 48, 8, 8, 8, 3, 3, 1, 1, 1, 1, T), (256, 64, 8, 8, 8, 3, 3, 2, 1, 1, 1, T), (256, 64, 7, 8, 8, 3, 3, 1, 1, 1, 1, T), (256, 256, 8, 8, 8, 3, 3, 1, 1, 1, 1, T),
           (64, 32, 5, 6, 5, 6, 5, 1, 2, 1, 1, T), (256, 64, 8, 8, 8, 9, 3, 1, 1, 1, 1, T), (256, 64, 8, 8, 8, 3, 3, 1, 7, 1, 1, T), (256, 64, 8, 8, 8, 3, 3, 0, 1, 1, 1, T)]
    ws = []
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for c in cases + bad:
            w = rng.randint(-(1 << 62), 1 << 62, size=(c[9], c[10], c[5], c[6])).astype(np.int64)
            w.reshape(-1)[0] = np.iinfo(np.int64).min; w.reshape(-1)[-1] = np.iinfo(np.int64).max
            ws.append(w)
            f.write(" ".join(str(v) for v in c) + "\n" + " ".join(str(int(v)) for v in w.reshape(-1)) + "\n")
    out = subprocess.check_output([exe, path], text=True).split("\n")
    at = 0
    for c, w in zip(cases, ws):
        plan = ca.binding.conv_slots_plan(*c[:9])
        assert [out[at + i].split()[0] for i in range(5)] == ["steps", "elts", "geom", "valid", "fold"]
        got = [[int(v) for v in out[at + i].split()[1:]] for i in range(5)]
        assert got[0] == plan.steps and got[1] == plan.elements and got[2] == [plan.out_h, plan.out_w, plan.out_dil] and got[3] == plan.valid, c
        assert got[4] == plan.fold(w, c[11]).reshape(-1).tolist(), c
        at += 5
    assert out[at:] == ["bad"] * len(bad) + [""]
    for c in bad:
        with pytest.raises(ValueError):
            ca.binding.conv_slots_plan(*c[:9])


def test_model_decrypts_to_the_plans_slots():
    """the golden set's ring (n = 256, two moduli) with a batching plaintext modulus: a 2 -> 2 channel layer on 4 x 4 planes (pitch 4, M = 16) with a 2 x 2 window,
    three keyed taps and the element 1, through conv_slots_model decrypts, with the oracle's decryptor, to the convolution at the valid slots of every period"""
    import crcnn_amd as ca
    from oracle import orc
    g0 = dict(np.load(GOLD))
    n, q = int(g0["n"]), [int(v) for v in g0["q"]]
    assert (n, len(q)) == (256, 2)
    t = ca.Engine.slots_prime(n, 20)
    M, half = 16, t // 2
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    GM = gm.GaloisModel(O)
    rng = np.random.RandomState(19)
    img = rng.randint(0, 16, size=(2, 4, 4)).astype(np.int64)
    w = rng.randint(-8, 9, size=(2, 2, 2, 2)).astype(np.int64); w[1, 0, 1, 1] = -8
    plan = E.conv_slots_plan(M, 4, 4, 4, 2, 2)
    assert plan.steps == [0, 1, 4, 5] and plan.valid == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    sk, pk = E.keygen(41)
    elts, gk = E.gen_galois_keys(42, sk, elts=plan.elements[1:])
    kc = {int(g): hm.conjugate_key_coeff(GM, GM.key_coeff(gk[e], 16), int(g)) for e, g in enumerate(elts)}
    planes = np.stack([cm.plane_slots(img[ci], n, M, 4, 1).astype(np.int64) for ci in range(2)])
    x = E.encrypt(pk, E.slots_compose(planes, 2, n, n, 1), 43)
    wl = E.conv_slots_pack_weights(plan.fold(w, t))
    assert wl.shape == (2, 2, 2, 4)
    y = cm.conv_slots(GM, x, plan.elements, wl, kc)
    want = cm.conv_direct(img, w, 1)
    for co in range(2):
        assert O.noise_budget(sk, y[co]) >= 1
        got = E.slots_decompose(O.decrypt(sk, y[co]), n, n, 1).reshape(-1)
        for base in range(0, n, M):
            assert [int(got[base + s]) for s in plan.valid] == [int(v) for v in want[co].reshape(-1)], (co, base)
    assert int(np.abs(want).max()) < half
    E.close()


def test_work_bytes():
    import crcnn_amd as ca
    E = ca.Engine(4096, [0x7fffffff380001, 0x3fffffff000001], T, device=-1)
    f = E.conv_slots_work_bytes
    sizes = [f(c, 2, 3, 4) for c in (0, 1, 2, 64, 1024, 4096)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and 0 < sizes[1] < sizes[3] and sizes[-1] == sizes[-2]
    assert f(3, 4, 3, 4) >= f(3, 2, 3, 4) and f(1, 4, 3, 4) > f(1, 2, 3, 4)      # a pass holds ciphertexts of every channel
    assert f(3, 2, 3, 8) > f(3, 2, 3, 4)                                          # a prepared key and kept results per tap
    assert f(3, 2, 8, 4) >= f(3, 2, 3, 4)                                         # (the outputs are the caller's)
    assert f(3, 2, 3, 4) == E.diag_mac_work_bytes(6, 4)                           # hoist_layout over the flat input
    for bad in ((3, 0, 3, 4), (3, 2, 0, 4), (3, 2, 3, 0), (3, -1, 3, 4), (3, 2, -1, 4), (3, 2, 3, -1), (3, 4097, 3, 4), (3, 2, 4097, 4), (3, 2, 3, 1025)):
        assert f(*bad) == 0, bad
    assert f(3, 2, 3, 4, 0) == 0 and f(3, 2, 3, 4, 61) == 0
    assert f(3, 4096, 4096, 1024) > 0
    E.close()
