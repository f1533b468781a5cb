"""Hoisted rotations on the host: the NTT-domain index table and the key conjugation against their definitions (the oracle's transforms), the identity the
design rests on (H_g decrypts to what apply_galois decrypts to), and the diagonal planner against W x mod t."""
import os

import numpy as np
import pytest

import galois_hoisted_model as hm
import galois_model as gm

Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_n256_k2_t20.npz")


def host(n, q, t=1 << 20):
    import crcnn_amd as ca
    return ca.Engine(n, q, t, device=-1)


def elements(n):
    return [3, pow(3, -1, 2 * n), 2 * n - 1, 27 * (2 * n - 1) % (2 * n)]        # the last: a composite, 3^3 . (-1)


@pytest.mark.parametrize("n", [64, 256])
def test_ntt_table_is_ntt_sigma_intt(n):
    from oracle import orc
    E = host(n, Q2)
    O = orc.Oracle(n, Q2, 1 << 20)
    rng = np.random.RandomState(n)
    x = np.stack([rng.randint(0, 1 << 62, size=n).astype(np.uint64) % np.uint64(q) for q in Q2])[None]
    for g in elements(n) + [1]:
        tab = E.galois_ntt_table(g)
        assert sorted(tab.tolist()) == list(range(n)), g                # a permutation
        assert np.array_equal(x[..., tab], hm.ntt_sigma_rows(O, x, g)), g
    for bad in (0, 2, 2 * n + 1):
        assert E.L.crc_galois_ntt_table(E.c, bad, E.galois_ntt_table(3).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_uint32))) == -1
    E.close()


@pytest.mark.parametrize("n,q,dbc", [(64, Q2, 16), (256, Q2, 8), (256, Q1, 16)], ids=["n64_k2", "n256_k2_dbc8", "n256_k1"])
def test_host_conjugation_is_sigma_inverse_of_every_polynomial(n, q, dbc):
    import crcnn_amd as ca
    from oracle import orc
    E = host(n, q)
    O = orc.Oracle(n, q, 1 << 20)
    sk, _ = E.keygen(5)
    elts, gk = E.gen_galois_keys(6, sk, dbc=dbc, elts=elements(n))
    cg = E.galois_conjugate_keys(elts, gk, dbc=dbc)
    assert cg.shape == gk.shape
    for e, g in enumerate(int(v) for v in elts):
        assert np.array_equal(cg[e], hm.conjugate_key(O, gk[e], g)), g
        assert not np.array_equal(cg[e], gk[e])
    # refusals: g = 1 has no key, invalid elements, a bad dbc, in place
    one = np.zeros((1, gk.shape[1]), dtype=np.uint64)
    for bad in ([1], [2], [2 * n + 1]):
        with pytest.raises(ca.binding.CrcError):
            E.galois_conjugate_keys(bad, one, dbc=dbc)
    e3 = E._elts([3]); pu = ca.binding._pu
    assert E.L.crc_galois_conjugate_keys(E.c, pu(e3), 1, 0, pu(one), pu(one.copy())) == -1
    assert E.L.crc_galois_conjugate_keys(E.c, pu(e3), 1, dbc, pu(one), pu(one)) == -1
    assert E.L.crc_galois_conjugate_keys(E.c, pu(e3), 0, dbc, None, None) == 0
    E.close()


def test_hoisted_rotation_decrypts_to_apply_galois():
    """n = 256, k = 2 with the golden set's parameters: H_g under the conjugated key and apply_galois under the direct key decrypt to the same plaintext,
    both with noise budget left; their ciphertext bits differ (another digit decomposition); and the model equals the oracle's key switch of (c0, 0, c1)
    under K'_g followed by sigma_g -- an independent route to H_g's bits"""
    import crcnn_amd as ca
    from oracle import orc
    g0 = dict(np.load(GOLD))
    n, q, t = int(g0["n"]), [int(v) for v in g0["q"]], int(g0["t"])
    assert (n, len(q)) == (256, 2)
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    M = gm.GaloisModel(O)
    sk, pk = E.keygen(31)
    rng = np.random.RandomState(7)
    ct = E.encrypt(pk, rng.randint(0, t, size=(1, n)).astype(np.uint64), 78)[0]
    for dbc in (16, 8):
        elts, gk = E.gen_galois_keys(32, sk, dbc=dbc, elts=elements(n))
        cg = E.galois_conjugate_keys(elts, gk, dbc=dbc)
        for e, g in enumerate(int(v) for v in elts):
            direct = M.apply(ct, g, gk[e], dbc)
            hoist = hm.hoisted(M, ct, g, cg[e], dbc)
            assert E.noise_budget(sk, hoist) >= 1 and E.noise_budget(sk, direct) >= 1, (dbc, g)
            assert np.array_equal(E.decrypt(sk, hoist[None]), E.decrypt(sk, direct[None])), (dbc, g)
            assert not np.array_equal(hoist, direct), (dbc, g)
            x3 = np.zeros((3, len(q), n), dtype=np.uint64)
            x3[0] = ct[0]; x3[2] = ct[1]
            z = O.relinearize(x3, np.ascontiguousarray(cg[e]), dbc)
            assert np.array_equal(np.stack([gm.sigma_rows_np(z[p], g, q) for p in range(2)]), hoist), (dbc, g)
            # an UN-conjugated key in H_g's place decrypts to something else: the mistake the interface cannot detect
            wrong = hm.hoisted(M, ct, g, gk[e], dbc)
            assert not np.array_equal(E.decrypt(sk, wrong[None]), E.decrypt(sk, direct[None])), (dbc, g)
    assert np.array_equal(hm.hoisted(M, ct, 1, None), ct)
    E.close()


def tiled(x, M, n):
    return np.tile(np.concatenate([np.asarray(x, dtype=np.int64), np.zeros(M - len(x), dtype=np.int64)]), n // M)


@pytest.mark.parametrize("M,shape,kind", [(4, (4, 4), "dense"), (8, (8, 8), "dense"), (8, (5, 8), "dense"), (8, (8, 3), "dense"), (8, (8, 8), "sparse"),
                                          (8, (8, 8), "zero")])
def test_diag_matvec_plan_against_the_integer_product(M, shape, kind):
    import crcnn_amd as ca
    n, t = 64, 65537
    rng = np.random.RandomState(M * 100 + shape[0] * 10 + shape[1])
    W = rng.randint(0, t, size=shape).astype(np.int64)
    if kind == "sparse":                                              # only the diagonals 0, 3 and 7 are populated
        i = np.arange(M)[:, None]; j = np.arange(M)[None, :]
        W = np.where(np.isin((j - i) % M, [0, 3, 7]), W, 0)
    if kind == "zero":
        W[:] = 0
    x = rng.randint(0, t, size=shape[1]).astype(np.int64)
    steps, rows = ca.binding.diag_matvec_plan(W, M, n)
    assert rows.shape == (len(steps), n) and steps == sorted(set(steps)) and all(0 <= d < M for d in steps)
    if kind == "sparse":
        assert steps == [0, 3, 7]
    if kind == "zero":
        assert steps == []
    for r, d in enumerate(steps):                                     # period M over both rows of n/2 slots
        assert np.array_equal(rows[r], np.tile(rows[r][:M], n // M))
    got = hm.diag_matvec_slots(steps, rows, tiled(x, M, n), t)
    want = hm.matvec(W, x, t)
    want = want + [0] * (M - len(want))
    assert got == want * (n // M)
    for bad_M in (3, 0, n):                                            # not a power of two, none, beyond n/2
        with pytest.raises(ValueError):
            ca.binding.diag_matvec_plan(W, bad_M, n)
    with pytest.raises(ValueError):
        ca.binding.diag_matvec_plan(np.zeros((M + 1, M), dtype=np.int64), M, n)


def test_work_bytes():
    import crcnn_amd as ca
    E = ca.Engine(4096, Q2, 65537, device=-1)
    for f in (E.rotate_hoisted_work_bytes, E.diag_mac_work_bytes):
        sizes = [f(c, 4) for c in (0, 1, 2, 3, 64, 1024, 4096)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0 and sizes[1] < sizes[4]
        assert sizes[-1] == sizes[-2]                                # internal passes: bounded in count
        assert f(3, 4, 0) == 0 and f(3, 4, 61) == 0 and f(3, 0) == 0 and f(3, 4, 8) >= f(3, 4, 16)
        assert f(3, 8) > f(3, 4)                                     # a prepared key per element
    E.close()
