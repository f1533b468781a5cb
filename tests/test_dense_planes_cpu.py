"""The dense layer over channel planes on the host: the planner and its fold against the direct integer sum (junk in every slot that is no input, exact zeros at
every slot that is no output), the refusals, the C++ planner against the Python one, the integer model through encryption at the small ring, and the
work-space size."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dense_planes_model as dm
import galois_hoisted_model as hm
import galois_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ops_n256_k2_t20.npz")
T = 65537
LATTICE = [4 * (28 * y + x) for y in range(4) for x in range(4)]        # 4 x 4 pixels at dilation 4 and pitch 28: what conv2 + pool2 leave of a 28 x 28 image
IRREGULAR = [3, 7, 8, 20, 41, 63]
# (n, M, in_slots, out_slots, Cin)
CASES = [
    (4096, 1024, LATTICE, list(range(6)), 1),
    (4096, 1024, LATTICE, list(range(6)), 3),
    (2048, 1024, LATTICE, [4 * (28 * a + b) for a in range(2) for b in range(5)], 3),       # outputs on the input lattice continued to 2 x 5
    (256, 64, IRREGULAR, [0, 5, 63, 30], 1),
    (256, 64, IRREGULAR, [62, 1, 20, 21, 22], 3),
    (128, 64, [0, 16, 32, 48], [0, 16, 32, 48], 3),                                         # 16 pairs, 4 steps: the differences coincide mod M
    (512, 64, [1, 33], [32, 0, 5], 1),
]
IDS = ["lattice_contiguous_cin1", "lattice_contiguous_cin3", "lattice_to_lattice_cin3", "irregular_cin1", "irregular_cin3", "steps_coincide_mod_M", "wrap_cin1"]


def weights(seed, O, Cin, P):
    rng = np.random.RandomState(seed)
    W = rng.randint(-(T // 2), T // 2 + 1, size=(O, Cin, P)).astype(np.int64)
    W[0, 0, 0] = T - 1; W[-1, -1, -1] = -(1 << 62)
    return W, rng


@pytest.mark.parametrize("n,M,ins,outs,Cin", CASES, ids=IDS)
def test_plan_and_fold_against_the_direct_sum(n, M, ins, outs, Cin):
    import crcnn_amd as ca
    plan = ca.binding.dense_planes_plan(n, M, ins, outs)
    want_steps = sorted({(p - o) % M for p in ins for o in outs})
    assert plan.steps == want_steps and plan.elements == [gm.elt_rows(n, s) for s in want_steps]
    assert len(plan.steps) <= len(ins) * len(outs)
    if 0 in plan.steps:
        assert plan.steps[0] == 0 and plan.elements[0] == 1
    W, rng = weights(n + M + Cin, len(outs), Cin, len(ins))
    rows = plan.fold(W, T)
    R = len(plan.steps)
    assert rows.shape == (R, Cin, n) and rows.dtype == np.int64 and (rows >= 0).all() and (rows < T).all()
    assert np.array_equal(rows, np.stack([plan.fold(W, T, j) for j in range(R)]))
    not_in = np.ones(n, dtype=bool)
    for base in range(0, n, M):
        not_in[[base + s for s in ins]] = False
    assert not rows[:, :, not_in].any()                                 # the rows read nothing but the inputs
    for fill in range(2):                                               # two junk fills: what holds by accident in one does not in the other
        xs = rng.randint(0, T, size=(Cin, len(ins))).astype(np.int64)
        planes = [dm.vector_slots(xs[c], ins, n, M, junk=rng.randint(0, T, size=M)) for c in range(Cin)]
        got = dm.dense_slots(plan, rows, planes, T)
        want = dm.dense_direct(W, xs, T)
        expect = np.zeros(M, dtype=object)
        for o, s in enumerate(outs):
            expect[s] = want[o]
        assert [int(v) for v in got] == [int(v) for v in np.tile(expect, n // M)], fill      # ... and exactly 0 at every slot that is no output


def test_the_layout_of_the_outputs_decides_the_step_count():
    """PlainModelTiny's fc3 behind conv2 + pool2: 64 planes of 4 x 4 pixels at slots 4 (28 y + x) -> 512 outputs.  Outputs on contiguous slots against outputs on
    the input lattice continued: the counts are the planner's (printed), the bounds are reasoned.  The lattice 4 (28 a + b) continued to 16 x 32 names slots that
    are not distinct (28 a + 28 = 28 (a + 1)) and do not fit M = 1024, which has 256 multiples of 4: the planner refuses it.  Continued row-major over
    the period M = 2048 instead, output m at slot 4 m for m < 512: every difference is a multiple of 4 below M, so at most 512 steps -- below the
    (16 + 3) (32 + 3) = 665 distinct differences a 16 x 32 lattice could have"""
    import crcnn_amd as ca
    f = ca.binding.dense_planes_plan
    with pytest.raises(ValueError):
        f(4096, 1024, LATTICE, [4 * (28 * a + b) for a in range(16) for b in range(32)])
    contiguous, lattice = f(4096, 1024, LATTICE, 512), f(4096, 2048, LATTICE, [4 * m for m in range(512)])
    print("fc3 steps: contiguous outputs", len(contiguous.steps), "lattice outputs", len(lattice.steps))
    assert len(contiguous.steps) <= 1024 and len(lattice.steps) <= 512 < (16 + 3) * (32 + 3)
    assert len(lattice.steps) < len(contiguous.steps)
    fc4 = f(4096, 2048, lattice.out_slots, [4 * m for m in range(10)])                       # fc4 behind it: a vector at strided slots, Cin = 1
    print("fc4 steps:", len(fc4.steps))
    assert len(fc4.steps) <= 512


def test_refusals():
    import crcnn_amd as ca
    f = ca.binding.dense_planes_plan
    f(256, 64, [1, 2], [0])                                             # the call the refusals vary
    for bad in (dict(M=48), dict(M=0), dict(M=256), dict(n=100), dict(in_slots=[]), dict(out_slots=[]), dict(in_slots=[1, 1]), dict(out_slots=[0, 0]),
                dict(in_slots=[64]), dict(out_slots=[64]), dict(in_slots=[-1]), dict(out_slots=[-1]), dict(out_slots=0)):
        a = dict(n=256, M=64, in_slots=[1, 2], out_slots=[0])
        a.update(bad)
        with pytest.raises(ValueError):
            f(**a)
    plan = f(256, 64, [1, 2], 3)
    assert plan.out_slots == [0, 1, 2]
    for shape in ((3, 1, 3), (2, 1, 2), (3, 0, 2), (3, 2)):
        with pytest.raises(ValueError):
            plan.fold(np.zeros(shape, dtype=np.int64), T)
    with pytest.raises(ValueError):
        plan.fold(np.zeros((3, 1, 2), dtype=np.int64), 1)
    E = ca.Engine(256, [0x3fffffff000001], T, device=-1)
    assert E.dense_planes_plan(64, [1, 2], 3).steps == plan.steps
    E.close()


def test_cpp_planner_equals_the_python_planner():
    """tests/cpp/dense_planes_plan_check.cpp (address and undefined-behaviour sanitizers) prints crc_dense_planes_plan and crc_dense_planes_fold for the cases of
    a file; inside it checks that a refusal writes nothing"""
    import crcnn_amd as ca
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "dense_planes_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dense_planes_plan_check.cpp"), "-o", exe])
    rng = np.random.RandomState(6)
    cases = [(n, M, ins, outs, Cin, t) for (n, M, ins, outs, Cin), t in zip(CASES, (T, 2, (1 << 61) - 1, T, 12289, T, T))]
    bad = [(256, 48, [1], [0], 1, T), (256, 256, [1], [0], 1, T), (256, 64, [], [0], 1, T), (256, 64, [1], [], 1, T), (256, 64, [1, 1], [0], 1, T),
           (256, 64, [1], [0, 0], 1, T), (256, 64, [64], [0], 1, T), (256, 64, [1], [-1], 1, T), (100, 32, [1], [0], 1, T)]
    ws = []
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for n, M, ins, outs, Cin, t in cases + bad:
            w = rng.randint(-(1 << 62), 1 << 62, size=(len(outs), Cin, len(ins))).astype(np.int64)
            if w.size:
                w.reshape(-1)[0] = np.iinfo(np.int64).min; w.reshape(-1)[-1] = np.iinfo(np.int64).max
            ws.append(w)
            f.write(f"{n} {M} {len(ins)} {len(outs)} {Cin} {t}\n" + " ".join(str(v) for v in ins) + "\n" + " ".join(str(v) for v in outs) + "\n"
                    + " ".join(str(int(v)) for v in w.reshape(-1)) + "\n")
    out = subprocess.check_output([exe, path], text=True).split("\n")
    at = 0
    for (n, M, ins, outs, Cin, t), w in zip(cases, ws):
        plan = ca.binding.dense_planes_plan(n, M, ins, outs)
        assert [out[at + i].split()[0] for i in range(3)] == ["steps", "elts", "fold"]
        got = [[int(v) for v in out[at + i].split()[1:]] for i in range(3)]
        assert got[0] == plan.steps and got[1] == plan.elements, (n, M)
        assert got[2] == plan.fold(w, t).reshape(-1).tolist(), (n, M, Cin)
        at += 3
    assert out[at:] == ["bad"] * len(bad) + [""]
    for n, M, ins, outs, Cin, t in bad:
        with pytest.raises(ValueError):
            ca.binding.dense_planes_plan(n, M, ins, outs)


def test_model_decrypts_to_the_layer():
    """the golden set's ring (n = 256, two moduli) with a batching plaintext modulus: two planes of 2 x 2 pixels (pitch 4, M = 16) under junk -> 3 outputs at slots
    0, 1, 2 through dense_planes_model (galois_hoisted_model.hoisted per step, integers mod q).  First the parameters: the model's own decryption must leave a
    positive noise budget -- a failure there is a parameter choice, not a fault of the layer.  Then every slot of every period is the integer layer, 0 off the
    outputs"""
    import crcnn_amd as ca
    from oracle import orc
    g0 = dict(np.load(GOLD))
    n, q = int(g0["n"]), [int(v) for v in g0["q"]]
    assert (n, len(q)) == (256, 2)
    t = ca.Engine.slots_prime(n, 20)
    M, half, Cin = 16, t // 2, 2
    ins, outs = [0, 1, 4, 5], [0, 1, 2]
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    GM = gm.GaloisModel(O)
    rng = np.random.RandomState(23)
    xs = rng.randint(0, 16, size=(Cin, len(ins))).astype(np.int64)
    W = rng.randint(-8, 9, size=(len(outs), Cin, len(ins))).astype(np.int64); W[1, 0, 3] = -8
    plan = E.dense_planes_plan(M, ins, outs)
    assert plan.steps == [0, 1, 2, 3, 4, 5, 14, 15]
    sk, pk = E.keygen(51)
    elts, gk = E.gen_galois_keys(52, sk, elts=plan.elements[1:])
    kc = {int(g): hm.conjugate_key_coeff(GM, GM.key_coeff(gk[e], 16), int(g)) for e, g in enumerate(elts)}
    planes = np.stack([dm.vector_slots(xs[c], ins, n, M, junk=rng.randint(-half, half + 1, size=M)).astype(np.int64) for c in range(Cin)])
    x = E.encrypt(pk, E.slots_compose(planes, Cin, n, n, 1), 53)
    rows = plan.fold(W, t)
    centred = (rows + half) % t - half
    p_ntt = O.plains_to_ntt(E.slots_compose(centred.reshape(-1, n), len(plan.steps) * Cin, n, n, 1)).reshape(len(plan.steps), Cin, len(q), n)
    y = dm.dense_planes(GM, x, plan.elements, p_ntt, kc)
    budget = O.noise_budget(sk, y)
    print("noise budget of the layer's result:", budget)
    assert budget > 0, "the parameters leave no noise budget: choose others"
    got = E.slots_decompose(O.decrypt(sk, y), n, n, 1).reshape(-1)
    want = dm.dense_direct(W, xs, t)
    expect = [0] * M
    for o, s in enumerate(outs):
        expect[s] = (want[o] + half) % t - half
    assert [int(v) for v in got] == expect * (n // M)
    E.close()


def test_work_bytes_follow_the_layout_rule():
    """square_chunk = 1024 at (4096, 2): a pass is min(count, 1024 . 8 / (Cin + R)) ciphertexts per channel and keeps (Cin + R) of them; without d_pk the work
    space holds R prepared keys, with it one"""
    import crcnn_amd as ca
    E = ca.Engine(4096, [0x7fffffff380001, 0x3fffffff000001], T, device=-1)
    f = E.dense_planes_work_bytes
    sizes = [f(c, 3, 5) for c in (0, 1, 2, 64, 1024, 4096)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and 0 < sizes[1] < sizes[3] and sizes[-1] == sizes[-2]
    kpw = (E.galois_prepared_key_words() + 31) & ~31
    assert E.galois_prepared_key_words() == 2 * E.L.crc_evk_words(E.c, 16)
    for R in (1, 5, 34):
        assert f(2, 3, R) - f(2, 3, R, prepared=True) == (R - 1) * kpw * 8
    ctb = 2 * 2 * 4096 * 8
    assert f(1, 4, 5, prepared=True) - f(1, 3, 5, prepared=True) == ctb                        # one more transformed input per pass
    assert f(1, 3, 6, prepared=True) > f(1, 3, 5, prepared=True)                               # one more inner sum, and a longer sub-batch
    # 8192 / (64 + 600) = 12 ciphertexts per pass: 13 and 4096 need the same room
    assert f(13, 64, 600, prepared=True) == f(4096, 64, 600, prepared=True) == f(12, 64, 600, prepared=True)
    for bad in ((3, 0, 5), (3, 3, 0), (3, -1, 5), (3, 3, -1), (3, 4097, 5), (3, 3, 65537)):
        assert f(*bad) == 0, bad
    assert f(3, 3, 5, 0) == 0 and f(3, 3, 5, 61) == 0
    assert f(3, 4096, 65536, prepared=True) > 0
    S = ca.Engine(256, [0x3fffffff000001], 12289, device=-1)
    assert S.galois_prepared_key_words(16) > 0 and S.galois_prepared_key_words(0) == 0 and S.galois_prepared_key_words(61) == 0
    E.close(); S.close()
