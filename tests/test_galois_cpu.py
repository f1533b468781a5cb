"""Galois elements, the rotation planner and Galois key generation on the host (crc_galois_* / crc_gen_galois_keys), against tests/galois_model.py."""
import numpy as np
import pytest

import galois_model as gm

Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
NOISE_CLIP = 19                                   # client.cpp gauss(): sigma = 3.19 cut at 6 sigma = 19.14, truncated towards zero


def host(n, q, t=1 << 20):
    import crcnn_amd as ca
    return ca.Engine(n, q, t, device=-1)


def plan_or_none(E, g, elts):
    import crcnn_amd as ca
    try:
        return E.galois_plan(g, elts)
    except ca.binding.CrcError as e:
        assert e.status == -1
        return None


@pytest.mark.parametrize("n", [64, 4096])
def test_element_helpers(n):
    E = host(n, Q1)
    assert [int(v) for v in E.galois_default_elts()] == gm.default_elts(n)
    assert len(set(gm.default_elts(n))) == len(gm.default_elts(n)) == 2 * (n.bit_length() - 1) - 2
    assert E.galois_elt_columns() == 2 * n - 1
    steps = range(-n // 2 - 2, n // 2 + 3) if n == 64 else [0, 1, -1, 5, n // 2 - 1, -(n // 2 - 1), n // 2, -n // 2, 1 << 20, -(1 << 20)]
    for s in steps:
        assert E.galois_elt_rows(s) == gm.elt_rows(n, s), s
    assert E.galois_elt_rows(0) == 1 and E.galois_elt_rows(n // 2) == 0 and E.galois_elt_rows(-(n // 2)) == 0
    for g in (0, 1, 2, 3, 2 * n - 2, 2 * n - 1, 2 * n, 2 * n + 1, 1 << 40):
        assert E.galois_elt_valid(g) == gm.elt_valid(n, g), g
    E.close()


def test_plan_every_step_and_element_at_n64():
    n = 64
    E = host(n, Q1)
    elts = gm.default_elts(n)
    for s in range(-(n // 2 - 1), n // 2):
        g = gm.elt_rows(n, s)
        assert E.galois_plan(g, elts) == gm.plan(n, g, elts), s
    for g in range(1, 2 * n, 2):                                   # every valid element, the column swaps among them
        assert E.galois_plan(g, elts) == gm.plan(n, g, elts), g
    assert E.galois_plan(1, elts) == [] and E.galois_plan(1, []) == []
    # applying the planned elements one after the other IS the element: their product mod 2n
    for g in range(1, 2 * n, 2):
        prod = 1
        for i in E.galois_plan(g, elts):
            prod = prod * elts[i] % (2 * n)
        assert prod == g
    E.close()


def test_plan_sample_missing_key_and_hamming_branch():
    n = 4096
    E = host(n, Q1)
    elts = gm.default_elts(n)
    rng = np.random.RandomState(4)
    for g in [int(v) | 1 for v in rng.randint(0, 2 * n, size=200)]:
        want = gm.plan(n, g, elts)
        assert want is not None and E.galois_plan(g, elts) == want, g
        assert len(want) <= n.bit_length() - 1
    # the Hamming-weight branch: rotate_rows(n/2 - 1) has o1 = n/2 - 1 (log2 n - 1 bits set) but n/2 - o1 = 1: ONE step over 3^-1
    g = gm.elt_rows(n, n // 2 - 1)
    inv3 = pow(3, -1, 2 * n)
    assert g == inv3 and E.galois_plan(g, [e for e in elts if e != inv3] + [inv3]) == [len(elts) - 1]
    g = gm.elt_rows(n, n // 2 - 3)                                   # o1 = n/2 - 3 -> 3 over 3^-1: (3^-1)^1 (3^-1)^2
    assert E.galois_plan(g, elts) == [elts.index(inv3), elts.index(inv3 * inv3 % (2 * n))] == gm.plan(n, g, elts)
    # a set with one element removed: every plan through it is refused, every other unchanged
    for drop in (3, 2 * n - 1, pow(3, 4, 2 * n)):
        less = [e for e in elts if e != drop]
        refused = 0
        for g in [gm.elt_rows(n, s) for s in (1, 2, 3, 4, 5, 16, 21, -1, -7)] + [2 * n - 1, 2 * n - 3, n + 1]:
            want = gm.plan(n, g, less)
            assert plan_or_none(E, g, less) == want, (drop, g)
            refused += want is None
        assert refused > 0, drop
    assert plan_or_none(E, 3, []) is None
    assert E.L.crc_galois_plan(E.c, 2, None, 0, None, 0) == -1 and E.L.crc_galois_plan(E.c, 2 * n + 1, None, 0, None, 0) == -1
    out = (__import__("ctypes").c_int * 1)()
    g = gm.elt_rows(n, 5)                                            # two steps do not fit a capacity of one
    assert E.L.crc_galois_plan(E.c, g, E._elts(elts).ctypes.data_as(__import__("crcnn_amd").binding.PU), len(elts), out, 1) == -1
    E.close()


@pytest.mark.parametrize("n,q,dbc", [(256, Q2, 16), (2048, Q1, 16), (256, Q2, 8)], ids=["n256_k2", "n2048_k1", "n256_k2_dbc8"])
def test_galois_keys_hide_sigma_s_under_clipped_noise(n, q, dbc):
    """first + second s - [j == l] w_{l,d} sigma_g(s) = -e: inverse-transformed and centred, every coefficient within the sampler's clip bound"""
    from oracle import orc
    E = host(n, q)
    O = orc.Oracle(n, q, 1 << 20)
    k = len(q)
    sk, _ = E.keygen(21)
    elts, gk = E.gen_galois_keys(22, sk, dbc=dbc)
    assert [int(e) for e in elts] == gm.default_elts(n) and gk.shape == (len(elts), gm.evk_words(n, q, dbc))
    s_coeff = [O.ntt_inv(j, sk[j]) for j in range(k)]
    seconds = set()
    for e, g in enumerate(int(v) for v in elts):
        sig = [O.ntt_fwd(j, np.array(gm.sigma_row(s_coeff[j], g, q[j]), dtype=np.uint64)).astype(object) for j in range(k)]
        off = 0
        for l in range(k):
            factor = 1
            for j in range(k):
                if j != l:
                    factor = factor * q[j] % q[l]
            for d in range(gm.digits(q[l], dbc)):
                first = gk[e, off:off + k * n].reshape(k, n); second = gk[e, off + k * n:off + 2 * k * n].reshape(k, n); off += 2 * k * n
                if l == 0 and d == 0:
                    seconds.add(second.tobytes())
                for j in range(k):
                    v = first[j].astype(object) + second[j].astype(object) * sk[j].astype(object)
                    if j == l:
                        v = v - factor * sig[j]
                    err = O.ntt_inv(j, np.array([int(x) % q[j] for x in v], dtype=np.uint64)).astype(object)
                    cen = np.array([int(x) if int(x) <= q[j] // 2 else int(x) - q[j] for x in err], dtype=np.int64)
                    assert np.abs(cen).max() <= NOISE_CLIP, (g, l, d, j, int(np.abs(cen).max()))
                    assert np.abs(cen).max() > 0                     # a key without noise is no key
                factor = factor * (1 << dbc) % q[l]
        assert off == gk.shape[1]
    assert len(seconds) == len(elts)                                 # no two elements share their uniform rows
    # the same seed gives the same blob, another seed another; a key does not depend on its place in the set
    _, again = E.gen_galois_keys(22, sk, dbc=dbc)
    assert np.array_equal(again, gk)
    _, other = E.gen_galois_keys(23, sk, dbc=dbc)
    assert not np.array_equal(other[0], gk[0])
    sub_e, sub = E.gen_galois_keys(22, sk, dbc=dbc, elts=[int(elts[2]), int(elts[0])])
    assert np.array_equal(sub[0], gk[2]) and np.array_equal(sub[1], gk[0])
    E.close()


def test_key_generation_refusals():
    import crcnn_amd as ca
    n = 256
    E = host(n, Q2)
    sk, _ = E.keygen(1)
    for bad in ([2], [2 * n + 1], [3, 0]):
        with pytest.raises(ca.binding.CrcError):
            E.gen_galois_keys(1, sk, elts=bad)
    for dbc in (0, 61):
        gk = np.zeros(8, dtype=np.uint64); e = E._elts([3])
        assert E.L.crc_gen_galois_keys(E.c, 1, ca.binding._pu(sk), dbc, ca.binding._pu(e), 1, ca.binding._pu(gk)) == -1
    E.close()


def test_model_rotation_decrypts_to_rotated_slots():
    """the model itself on the CPU at n = 256: apply_galois under generated keys decrypts to the slot statement, with noise budget left at dbc 16 and 8 -- the
    chain the GPU tests run at larger rings"""
    import crcnn_amd as ca
    from oracle import orc
    n, q = 256, Q2
    t = ca.Engine.slots_prime(n, 20)
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    M = gm.GaloisModel(O)
    sk, pk = E.keygen(31)
    rng = np.random.RandomState(2)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(1, n)).astype(np.int64)
    ct = E.encrypt(pk, E.slots_compose(v, 1, n, n, 1), 77)[0]
    for dbc in (16, 8):
        elts, gk = E.gen_galois_keys(32, sk, dbc=dbc)
        elts = [int(e) for e in elts]
        for g, want in ((gm.elt_rows(n, 1), gm.rotate_rows_slots(v, 1)), (gm.elt_rows(n, -1), gm.rotate_rows_slots(v, -1)),
                        (gm.elt_rows(n, 5), gm.rotate_rows_slots(v, 5)), (2 * n - 1, gm.rotate_columns_slots(v))):
            y = M.apply_planned(ct, g, elts, gk, dbc)
            assert E.noise_budget(sk, y) >= 1, (dbc, g)
            got = E.slots_decompose(E.decrypt(sk, y[None]), n, n, 1)
            assert np.array_equal(got.reshape(1, n), want), (dbc, g)
    # the model's one step is the oracle's key switch of (sigma(c0), 0, sigma(c1)): an independent route to the same bits
    g = 3
    x3 = np.zeros((3, len(q), n), dtype=np.uint64)
    x3[0] = gm.sigma_rows_np(ct[0], g, q); x3[2] = gm.sigma_rows_np(ct[1], g, q)
    elts, gk = E.gen_galois_keys(32, sk, dbc=16)
    i3 = [int(e) for e in elts].index(3)
    assert np.array_equal(O.relinearize(x3, np.ascontiguousarray(gk[i3]), 16), M.apply(ct, 3, gk[i3], 16))
    E.close()


def test_work_bytes():
    import crcnn_amd as ca
    E = ca.Engine(4096, Q2, 65537, device=-1)
    for f in (E.apply_galois_work_bytes, E.sum_slots_work_bytes):
        sizes = [f(c) for c in (0, 1, 2, 3, 64, 1024, 4096)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0 and sizes[1] < sizes[4]
        assert sizes[-1] == sizes[-2]                                # internal passes: bounded in count
        assert f(3, 0) == 0 and f(3, 61) == 0 and f(3, 8) >= f(3, 16)
    E.close()
