"""The baby-step / giant-step matrix-vector product on the host: the planner against W x mod t with plain slot rotations, what it drops for sparse matrices, the
flat plan as the split at B = M, the element list, the C++ planner against the Python one, and the integer model through encryption at the small ring."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bsgs_model as bm
import galois_hoisted_model as hm
import galois_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ops_n256_k2_t20.npz")
T = 65537


def powers(M):
    return [1 << e for e in range(M.bit_length())]


def matrix(M, shape, seed):
    rng = np.random.RandomState(seed)
    W = rng.randint(0, T, size=shape).astype(np.int64)
    W[0, 0] = T - 1
    return W, rng.randint(0, T, size=shape[1]).astype(np.int64)


def tiled(x, M, n):
    return np.tile(np.concatenate([np.asarray(x, dtype=np.int64), np.zeros(M - len(x), dtype=np.int64)]), n // M)


def only_diagonals(W, M, keep):
    i = np.arange(M)[:, None]; j = np.arange(M)[None, :]
    return np.where(np.isin((j - i) % M, keep), W, 0)


@pytest.mark.parametrize("M", [4, 16, 64])
def test_plan_against_the_integer_product(M):
    """every power-of-two B <= M, shapes M x M, 5 x M and 3 x 7 (padded; 3 x 4 where M = 4): the plan applied with plain slot rotations is W x mod t in every
    period of both slot rows"""
    import crcnn_amd as ca
    n = 4 * M
    for shape in ((M, M), (min(5, M), M), (3, min(7, M))):
        W, x = matrix(M, shape, 100 * M + shape[0])
        want = hm.matvec(W, x, T)
        want = (want + [0] * (M - len(want))) * (n // M)
        for B in powers(M):
            baby, giant, rows = ca.binding.bsgs_matvec_plan(W, M, n, B)
            assert rows.shape == (len(giant), len(baby), n) and rows.dtype == np.int64
            assert baby == sorted(set(baby)) and all(0 <= b < B for b in baby)
            assert giant == sorted(set(giant)) and all(0 <= g < M and g % B == 0 for g in giant)
            assert np.array_equal(rows, np.tile(rows[..., :M], n // M))                # period M
            assert bm.bsgs_slots(baby, giant, rows, tiled(x, M, n), T) == want, (shape, B)


def test_sparse_matrices_drop_their_steps():
    import crcnn_amd as ca
    M, n, B = 16, 64, 4
    W, x = matrix(M, (M, M), 7)
    # no entry on the diagonals 8..11 (giant group 2) nor on any d = 1 mod 4 (baby step 1)
    keep = [d for d in range(M) if d // B != 2 and d % B != 1]
    Ws = only_diagonals(W, M, keep)
    baby, giant, rows = ca.binding.bsgs_matvec_plan(Ws, M, n, B)
    assert baby == [0, 2, 3] and giant == [0, 4, 12]
    assert bm.bsgs_slots(baby, giant, rows, tiled(x, M, n), T) == hm.matvec(Ws, x, T) * (n // M)
    # a baby step used by one kept group only: a zero row in the others
    Wz = only_diagonals(W, M, [0, 5, 6])
    baby, giant, rows = ca.binding.bsgs_matvec_plan(Wz, M, n, B)
    assert baby == [0, 1, 2] and giant == [0, 4]
    assert not rows[0, 1].any() and not rows[0, 2].any() and not rows[1, 0].any() and rows[0, 0].any() and rows[1, 1].any()
    assert bm.bsgs_slots(baby, giant, rows, tiled(x, M, n), T) == hm.matvec(Wz, x, T) * (n // M)
    # the only non-zero diagonal is d = B + 1: one baby step and one giant step
    W1 = only_diagonals(np.ones((M, M), dtype=np.int64), M, [B + 1])
    baby, giant, rows = ca.binding.bsgs_matvec_plan(W1, M, n, B)
    assert baby == [1] and giant == [B] and rows.shape == (1, 1, n)
    assert bm.bsgs_slots(baby, giant, rows, tiled(x, M, n), T) == hm.matvec(W1, x, T) * (n // M)
    baby, giant, rows = ca.binding.bsgs_matvec_plan(np.zeros((M, M), dtype=np.int64), M, n, B)
    assert baby == [] and giant == [] and rows.shape == (0, 0, n)


def test_the_flat_plan_is_the_split_at_M_and_refusals():
    import crcnn_amd as ca
    M, n = 16, 64
    W, _ = matrix(M, (11, M), 3)
    W = only_diagonals(np.pad(W, ((0, M - 11), (0, 0))), M, [0, 3, 7, 15])
    steps, flat = ca.binding.diag_matvec_plan(W, M, n)
    baby, giant, rows = ca.binding.bsgs_matvec_plan(W, M, n, M)
    assert baby == steps == [0, 3, 7, 15] and giant == [0] and np.array_equal(rows[0], flat)
    E = ca.Engine(n, [0x3fffffff000001], T, device=-1)
    b2, g2, r2 = E.bsgs_matvec_plan(W, M, 4)
    b3, g3, r3 = ca.binding.bsgs_matvec_plan(W, M, n, 4)
    assert (b2, g2) == (b3, g3) and np.array_equal(r2, r3)
    E.close()
    for M_, B_ in ((3, 1), (0, 1), (n, 4), (M, 0), (M, 3), (M, 2 * M), (M, -4)):
        with pytest.raises(ValueError):
            ca.binding.bsgs_matvec_plan(W[:1, :1], M_, n, B_)
        with pytest.raises(ValueError):
            ca.binding.bsgs_elements(M_, B_, n)
    with pytest.raises(ValueError):
        ca.binding.bsgs_matvec_plan(np.zeros((M + 1, M), dtype=np.int64), M, n, 4)


@pytest.mark.parametrize("M", [4, 16, 64])
def test_bsgs_elements_are_the_dense_plans(M):
    import crcnn_amd as ca
    n = 4 * M
    W = np.ones((M, M), dtype=np.int64)
    for B in powers(M):
        baby, giant, _ = ca.binding.bsgs_matvec_plan(W, M, n, B)
        assert baby == list(range(B)) and giant == list(range(0, M, B))
        used = {gm.elt_rows(n, s) for s in baby + giant} - {1}
        elts = ca.binding.bsgs_elements(M, B, n)
        assert len(elts) == len(set(elts)) == B + M // B - 2 and set(elts) == used, B
    assert len(ca.binding.bsgs_elements(16, 4, 4096)) == 6                              # where the flat method needs 15


def test_cpp_planner_equals_the_python_planner():
    """tests/cpp/bsgs_plan_check.cpp (address and undefined-behaviour sanitizers) prints crc_bsgs_plan and crc_bsgs_elements for the cases of a file; inside it
    checks that a refusal writes nothing and that B = M is crc_diag_plan"""
    import crcnn_amd as ca
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "bsgs_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "bsgs_plan_check.cpp"), "-o", exe])
    cases = []
    for M in (4, 16, 64):
        n = 4 * M
        for si, shape in enumerate(((M, M), (min(5, M), M), (3, min(7, M)))):
            W, _ = matrix(M, shape, 10 * M + si)
            W = W - T // 2                                              # (signed entries pass through unchanged)
            if si == 1:
                W = only_diagonals(np.pad(W, ((0, M - shape[0]), (0, 0))), M, [0, M // 2 + 1, M - 1])
            cases += [(M, n, B, W) for B in powers(M)]
    cases += [(16, 64, 4, np.zeros((16, 16), dtype=np.int64)), (1, 2, 1, np.array([[5]]))]
    bad = [(3, 64, 1, W), (16, 64, 3, W[:2, :2]), (16, 64, 32, W[:2, :2]), (16, 16, 4, W[:2, :2]), (16, 64, 0, W[:2, :2]), (4, 64, 2, np.zeros((5, 4), dtype=np.int64))]
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for M, n, B, W in cases + bad:
            f.write(f"{M} {n} {B} {W.shape[0]} {W.shape[1]}\n" + " ".join(str(int(v)) for v in W.reshape(-1)) + "\n")
    out = subprocess.check_output([exe, path], text=True).split("\n")
    at = 0
    for M, n, B, W in cases:
        baby, giant, rows = ca.binding.bsgs_matvec_plan(W, M, n, B)
        got = [[int(v) for v in out[at + i].split()[1:]] for i in range(4)]
        assert [out[at + i].split()[0] for i in range(4)] == ["baby", "giant", "rows", "elts"]
        assert got[0] == baby and got[1] == giant and got[2] == rows.reshape(-1).tolist() and got[3] == ca.binding.bsgs_elements(M, B, n), (M, B, W.shape)
        at += 4
    assert out[at:] == ["bad 0"] * (len(bad) - 1) + ["bad 2", ""]     # (the last: a matrix too tall for M, the split itself valid)


def test_model_decrypts_to_the_plans_slots():
    """the golden set's ring (n = 256, two moduli) with a batching plaintext modulus: a 4 x 4 matrix split at B = 2 (G = 2) through bsgs_model decrypts, with the
    oracle's decryptor, to the plan's slots = W x mod t in every period"""
    import crcnn_amd as ca
    from oracle import orc
    g0 = dict(np.load(GOLD))
    n, q = int(g0["n"]), [int(v) for v in g0["q"]]
    assert (n, len(q)) == (256, 2)
    t = ca.Engine.slots_prime(n, 20)
    M, B = 4, 2
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    GM = gm.GaloisModel(O)
    rng = np.random.RandomState(11)
    W = rng.randint(0, t, size=(M, M)).astype(np.int64); W[1, 2] = t - 1
    x = rng.randint(0, t, size=M).astype(np.int64)
    baby, giant, rows = E.bsgs_matvec_plan(W, M, B)
    assert baby == [0, 1] and giant == [0, 2]
    elts = ca.binding.bsgs_elements(M, B, n)
    assert elts == [gm.elt_rows(n, 1), gm.elt_rows(n, 2)]
    sk, pk = E.keygen(41)
    elts, gk = E.gen_galois_keys(42, sk, elts=elts)
    kc = {int(g): hm.conjugate_key_coeff(GM, GM.key_coeff(gk[e], 16), int(g)) for e, g in enumerate(elts)}
    ct = E.encrypt(pk, E.slots_compose(tiled(x, M, n), 1, n, n, 1), 43)[0]
    p_ntt = O.plains_to_ntt(E.slots_compose(rows.reshape(-1, n), len(giant) * len(baby), n, n, 1)).reshape(len(giant), len(baby), len(q), n)
    y = bm.bsgs(GM, ct, [gm.elt_rows(n, b) for b in baby], [gm.elt_rows(n, s) for s in giant], p_ntt, kc)
    assert O.noise_budget(sk, y) >= 1
    half = t // 2
    got = E.slots_decompose(O.decrypt(sk, y), n, n, 1)
    want = [(w + half) % t - half for w in hm.matvec(W, x, t)] * (n // M)
    assert got.tolist() == want
    assert [(v + half) % t - half for v in bm.bsgs_slots(baby, giant, rows, tiled(x, M, n), t)] == want
    E.close()


def test_work_bytes():
    import crcnn_amd as ca
    E = ca.Engine(4096, [0x7fffffff380001, 0x3fffffff000001], T, device=-1)
    f = E.diag_mac_bsgs_work_bytes
    sizes = [f(c, 4, 4) for c in (0, 1, 2, 64, 1024, 4096)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and 0 < sizes[1] < sizes[3] and sizes[-1] == sizes[-2]
    assert f(3, 0, 4) == 0 and f(3, 4, 0) == 0 and f(3, 4, 4, 0) == 0 and f(3, 4, 4, 61) == 0
    assert f(3, 8, 4) > f(3, 4, 4) and f(3, 4, 8) > f(3, 4, 4)       # a prepared key and kept ciphertexts per element
    assert f(3, 4, 1) > E.diag_mac_work_bytes(3, 4)                     # (the inner sums' room)
    E.close()
