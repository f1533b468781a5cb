"""The host decryptor (crc_decrypt, the twin of crc_decrypt_dev) against tests/decrypt_model.py at rounding and gamma-correction boundaries: twelve parameter
sets from one modulus and t = 2 to eight moduli and t = 2^60 - 1, ciphertexts (c0 = v, c1 = 0) that put a chosen v in front of the scaling step, and dense size-2
and size-3 ciphertexts whose every operand of c0 + c1 s + c2 s^2 is q_i - 1.  The model itself is held to round(t v / q) wherever the two must agree.  No GPU."""
import numpy as np
import pytest

import decrypt_model as dm

W44 = [0xfffffdf8001, 0x3fffffff000001]            # the width classes of tests/test_gpu_ntt_paths.py: generic Barrett reduction ...
W60 = [0xffffffffffe8001, 0x3fffffff000001]        # ... and the 60-bit fold
SETS = [(128, 1, 2), (128, 1, 1 << 18), (128, 2, 3), (128, 2, 65537), (128, 3, 1 << 42), (128, 8, 1 << 44), (128, 8, (1 << 60) - 1), (1024, 2, 1 << 20),
        (1024, 8, (1 << 60) - 1), (128, "w44", 1 << 20), (128, "w60", 1 << 42), (128, "w60", (1 << 60) - 1)]
DENSE = [(128, 2, 65537), (128, 8, 1 << 44)]
SEED = 2024


def set_id(s):
    n, m, t = s
    return f"n{n}_{m if isinstance(m, str) else 'k%d' % m}_t{t if t < 1 << 17 else '2e%d' % (t.bit_length() - 1) if t & (t - 1) == 0 else '2e60m1'}"


def moduli(m):
    """SEAL's default moduli of the ring that has m of them, or a width class"""
    import crcnn_amd as ca
    if isinstance(m, str):
        return list({"w44": W44, "w60": W60}[m])
    q = ca.default_coeff_modulus_128({1: 2048, 2: 4096, 3: 8192, 8: 16384}[m])[:m]
    assert len(q) == m
    return [int(p) for p in q]


def tables(E):
    return [E.table(f"root_powers:{i}") for i in range(E.k)], [E.table(f"inv_root_powers_div_two:{i}") for i in range(E.k)]


def test_the_sets_are_the_twelve():
    assert len(SETS) == 12 and len({set_id(s) for s in SETS}) == 12


@pytest.mark.parametrize("n, m, t", SETS, ids=[set_id(s) for s in SETS])
def test_host_decryptor_is_the_model_at_the_boundaries(n, m, t):
    import crcnn_amd as ca
    q = moduli(m); k = len(q)
    Q = dm.product(q)
    cs = dm.cases(tuple(q), t, SEED)
    has_pair = dm.GAMMA * t < Q
    assert len(cs) == 200 + 5 + 35 + (2 if has_pair else 0) + 1
    assert has_pair == (k > 1 and not (m == "w60" and t == (1 << 60) - 1))
    if has_pair:
        assert [c.r_gamma for c in cs if c.kind == "gamma"] == [dm.GAMMA >> 1, (dm.GAMMA >> 1) + 1]
    acc = cs[-1]
    assert acc.kind == "accumulator" and all(int(r) * y % qi == qi - 1 for r, y, qi in zip(acc.res, dm.constants(tuple(q), t).yc, q))
    # the model is the rounding wherever t v / q is clear of the half-integers ...
    plain = [c for c in cs if c.kind in ("uniform", "extreme")]
    assert len(plain) == 205
    for c in cs:
        if c.v is not None and dm.outside_band(c.v, Q, t, k):
            assert c.m == dm.true_round(c.v, Q, t), c
    # ... which the uniform values and the ends of [0, q) are.  The two middle values q // 2 and q // 2 + 1 are, too, under an even t; under an odd t they
    # give t v mod q = (q -+ t) / 2, which is t / 2 from q / 2: inside the band exactly when gamma t <= 2 (k + 1) q
    for c in plain:
        if t % 2 and c.v in (Q // 2, Q // 2 + 1):
            assert abs(2 * (t * c.v % Q) - Q) == t
            assert dm.outside_band(c.v, Q, t, k) == (dm.GAMMA * t > 2 * (k + 1) * Q), c
        else:
            assert dm.outside_band(c.v, Q, t, k), c
    # ... and it has not silently become the rounding
    if has_pair:
        assert any(c.m != dm.true_round(c.v, Q, t) for c in cs if c.kind == "rounding")
    E = ca.Engine(n, q, t, device=-1)
    try:
        cts, want = dm.place(cs, q, n)
        got = E.decrypt(np.zeros((k, n), dtype=np.uint64), cts)
        wrong = [(j, cs[j].kind, int(got[j, 7 * j % n]), cs[j].m) for j in range(len(cs)) if not np.array_equal(got[j], want[j])]
        assert not wrong, wrong[:10]
    finally:
        E.close()


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("n, m, t", DENSE, ids=[set_id(s) for s in DENSE])
def test_host_decryptor_on_dense_worst_case_operands(n, m, t, size):
    import crcnn_amd as ca
    q = moduli(m)
    E = ca.Engine(n, q, t, device=-1)
    try:
        ct, sk, v = dm.dense_case(q, n, size, *tables(E), seed=SEED + size)
        got = E.decrypt(sk, ct, size=size)
        assert [int(x) for x in got[0]] == dm.scale_rows(v, q, t)
    finally:
        E.close()
