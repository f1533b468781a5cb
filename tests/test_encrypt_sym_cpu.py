"""BFV encryption under the secret key, host twin (crc_encrypt_sym / crc_encrypt_sym_key; no GPU: host-only contexts).

c1 = A uniform (sampled as NTT-form residues), c0 = NTT(e + Delta m) - A . s.  The checker is the ORACLE (pinned to SEAL's Decryptor by
tests/test_oracle_golden.py): every ciphertext decrypts to its plaintext, its budget is at least what t (c0 + c1 s) = -r m_c + t e (mod q), |e| <= 19 allows, the
noise polynomial c0 + c1 s of an encryption of zero IS e and follows the clipped, truncated normal, and c1 is uniform.  tests/test_gpu_encrypt_sym.py pins the
device to these bits."""
import ctypes
import math
import os

import numpy as np
import pytest

import crcnn_amd as ca
from oracle import orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _golden_params(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return int(g["n"]), [int(x) for x in g["q"]], int(g["t"])


def _moduli(n, k):
    return ca.default_coeff_modulus_128(n) if n in (2048, 4096) else ca.default_coeff_modulus_128(8192)[:k]


def param_sets():
    """the four rings of test_device_encryptor / test_device_refresh with SEAL's default moduli, and the goldens with 40-bit moduli (t > q_i) and a 60-bit one"""
    sets = [(n, _moduli(n, k), t) for n, k, t in [(4096, 2, 1 << 29), (2048, 1, 1 << 18), (8192, 3, 1 << 42), (1024, 2, 1 << 16)]]
    return sets + [_golden_params("ops_n256_k2_q40_t41"), _golden_params("ops_n256_k1_q60_t30")]


IDS = ["n4096_k2_t29", "n2048_k1_t18", "n8192_k3_t42", "n1024_k2_t16", "n256_k2_q40_t41", "n256_k1_q60_t30"]


def _prod(q):
    Q = 1
    for v in q:
        Q *= int(v)
    return Q


def _plaintexts(E, n, q, t, cnt, rng):
    """random plaintexts below t with the all-zero and all-(t - 1) rows where r floor(t/2) + 19 t < q/2 (then every plaintext decrypts); else encoder-made
    ones (|m_c| <= 1).  Returns (plaintexts, max |m_c|)"""
    Q = _prod(q); r = Q % t
    if 2 * (r * (t // 2) + 19 * t) < Q:
        pl = rng.integers(0, t, size=(cnt, n), dtype=np.uint64)
        pl[0] = 0; pl[1] = t - 1
        return pl, t // 2
    pl, _ = E.encode((rng.standard_normal(cnt) * 3).astype(np.float32))
    return pl, 1


def _derived_budget(q, t, max_mc):
    Q = _prod(q); r = Q % t
    return max(0, Q.bit_length() - (r * max_mc + 19 * t).bit_length() - 1)


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_decrypts_under_the_oracle_with_the_derived_budget(n, q, t):
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, pk = E.keygen(11)
    rng = np.random.default_rng(5)
    cnt = 12
    pl, max_mc = _plaintexts(E, n, q, t, cnt, rng)
    if max_mc == 1:
        c = pl.astype(object); c = np.where(c > t // 2, t - c, c)
        assert int(c.max()) <= 1
    ct = E.encrypt_sym(sk, pl, 77)
    ctn = E.encrypt_sym(sk, pl, 77, out_form=ca.NTT)
    assert ct.shape == (cnt, 2, len(q), n)
    # the NTT form is the oracle's transform of the coefficient form: one ciphertext, two forms
    assert np.array_equal(ctn, np.stack([O.ct_to_ntt(ct[i]) for i in range(cnt)]))
    assert np.array_equal(np.stack([O.decrypt(sk, ct[i]) for i in range(cnt)]), pl)
    assert np.array_equal(np.stack([O.decrypt(sk, O.ct_from_ntt(ctn[i])) for i in range(cnt)]), pl)
    # t (c0 + c1 s) = -r m_c + t e (mod q), |e| <= 19: the budget follows in integers; and a public-key ciphertext of the same plaintext carries more noise
    bound = _derived_budget(q, t, max_mc)
    b_sym = [O.noise_budget(sk, ct[i]) for i in range(cnt)]
    print("budget", IDS[param_sets().index((n, q, t))], "derived bound", bound, "symmetric", b_sym)
    assert min(b_sym) >= bound, (b_sym, bound)
    ref = O.encrypt_many(pk, pl, 3)
    b_pk = [O.noise_budget(sk, ref[i]) for i in range(cnt)]
    print("public-key budgets", b_pk)
    assert all(b_sym[i] >= b_pk[i] for i in range(cnt)), (b_sym, b_pk)
    # the key-based entry point decrypts as well and equals the seed-based one under the expanded seed's key only by construction: distinct bits here
    key = E.random_key()
    ck = E.encrypt_sym(sk, pl, 0, key=key, stream_base=1000)
    assert np.array_equal(np.stack([O.decrypt(sk, ck[i]) for i in range(cnt)]), pl)
    assert not np.array_equal(ck[:, 1], ct[:, 1])
    E.close()


def _noise_of_zero(E, O, sk, q, cnt, seed):
    """c0 + c1 s of encryptions of zero, formed slot-wise from the NTT form in Python integers, back through the oracle's inverse transform: [cnt][k][n] centred"""
    n, k = E.n, len(q)
    ctn = E.encrypt_sym(sk, np.zeros((cnt, n), dtype=np.uint64), seed, out_form=ca.NTT)
    out = np.zeros((cnt, k, n), dtype=np.int64)
    for i in range(k):
        qi = int(q[i])
        v = (ctn[:, 0, i].astype(object) + ctn[:, 1, i].astype(object) * sk[i].astype(object)) % qi
        v = v.astype(np.uint64)
        for m in range(cnt):
            e = O.ntt_inv(i, v[m]).astype(np.int64)
            out[m, i] = np.where(e > qi // 2, e - qi, e)
    return out


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_noise_polynomial_is_the_small_integer_vector(n, q, t):
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(12)
    e = _noise_of_zero(E, O, sk, q, 4, 21)
    assert all(np.array_equal(e[:, i], e[:, 0]) for i in range(len(q)))        # the same integers under every modulus
    assert e.min() >= -19 and e.max() <= 19 and e.any()
    E.close()


def test_noise_follows_the_clipped_truncated_normal():
    """the chi-square of test_device_encryptor_noise_law (same law, same cell rule, same bound) over 2^19 draws"""
    n, q, t = 4096, _moduli(4096, 2), 1 << 29
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(13)
    e = _noise_of_zero(E, O, sk, q, 128, 4242)
    assert np.array_equal(e[:, 0], e[:, 1])
    e = e[:, 0]
    assert e.size >= 1 << 19 and e.min() >= -19 and e.max() <= 19
    sigma, lim = 3.19, 6 * 3.19
    Phi = lambda x: 0.5 * math.erfc(-x / (sigma * math.sqrt(2)))
    Z = Phi(lim) - Phi(-lim)
    law = {}
    for a in range(-19, 20):
        lo, hi = (-1.0, 1.0) if a == 0 else ((a, min(a + 1, lim)) if a > 0 else (max(a - 1, -lim), a))
        law[a] = (Phi(hi) - Phi(lo)) / Z
    assert abs(sum(law.values()) - 1.0) < 1e-12
    N = e.size
    counts = {a: int((e == a).sum()) for a in range(-19, 20)}
    chi, pooled_obs, pooled_exp, cells = 0.0, 0, 0.0, 0
    for a in range(-19, 20):
        ex = law[a] * N
        if ex >= 20: chi += (counts[a] - ex) ** 2 / ex; cells += 1
        else: pooled_obs += counts[a]; pooled_exp += ex
    if pooled_exp > 0: chi += (pooled_obs - pooled_exp) ** 2 / pooled_exp
    print("noise chi-square", chi, "cells", cells)
    assert chi < 80, (chi, cells, counts)
    assert abs(float(e.mean())) < 5 * sigma / math.sqrt(N) and abs(float(e.std()) - math.sqrt(sum(a * a * p for a, p in law.items()))) < 0.02
    E.close()


def _chi2_cdf(x, dof):
    """regularised lower incomplete gamma P(dof / 2, x / 2) by its power series (converges for every x; 400 terms are plenty at x < 200)"""
    a, z = dof / 2.0, x / 2.0
    term = 1.0 / a; s = term
    for j in range(1, 400):
        term *= z / (a + j); s += term
    return s * math.exp(-z + a * math.log(z) - math.lgamma(a))


def _chi2_quantile(p, dof):
    lo, hi = 0.0, 10.0 * dof
    for _ in range(200):
        mid = (lo + hi) / 2
        if _chi2_cdf(mid, dof) < p: lo = mid
        else: hi = mid
    return hi


def test_c1_is_uniform_and_a_function_of_the_stream_alone():
    n, q, t = 4096, _moduli(4096, 2), 1 << 29
    k = len(q)
    E = ca.Engine(n, q, t, device=-1)
    sk, pk = E.keygen(14)
    rng = np.random.default_rng(6)
    cnt = 256                                                # 2^20 residues per modulus
    pl = rng.integers(0, t, size=(cnt, n), dtype=np.uint64)
    ctn = E.encrypt_sym(sk, pl, 31337, out_form=ca.NTT)
    bound = _chi2_quantile(0.9999, 63)
    assert abs(bound - 113.5) < 0.1, bound
    for i in range(k):
        qi = int(q[i])
        x = ctn[:, 1, i].reshape(-1)
        assert x.size >= 1 << 20 and int(x.max()) < qi
        if qi < 1 << 58:
            bins = (x * np.uint64(64)) // np.uint64(qi)
        else:
            bins = np.array([(int(v) * 64) // qi for v in x], dtype=np.uint64)
        counts = np.bincount(bins.astype(np.int64), minlength=64)
        assert counts.size == 64
        ex = x.size / 64.0
        chi = float(((counts - ex) ** 2 / ex).sum())
        print("c1 chi-square, modulus", i, chi, "bound", bound)
        assert chi < bound, (i, chi)
    # c1 does not depend on the plaintext (nor does it under the other form's entry: the coefficient form is the inverse transform of this one)
    ctz = E.encrypt_sym(sk, np.zeros((cnt, n), dtype=np.uint64), 31337, out_form=ca.NTT)
    assert np.array_equal(ctz[:, 1], ctn[:, 1]) and not np.array_equal(ctz[:, 0], ctn[:, 0])
    # ... differs across ciphertexts, seeds and stream bases; stream m under base b + 1 is stream m + 1 under base b
    assert not np.array_equal(ctn[2, 1], ctn[3, 1])
    assert len({ctn[m, 1].tobytes() for m in range(cnt)}) == cnt
    assert not np.array_equal(E.encrypt_sym(sk, pl[:4], 31338, out_form=ca.NTT)[:, 1], ctn[:4, 1])
    key = bytes(range(32))
    a = E.encrypt_sym(sk, pl[:8], 0, out_form=ca.NTT, key=key, stream_base=500)
    b = E.encrypt_sym(sk, pl[:8], 0, out_form=ca.NTT, key=key, stream_base=501)
    assert not np.array_equal(a[:, 1], b[:, 1])
    assert np.array_equal(b[:7, 1], a[1:, 1])
    assert np.array_equal(E.encrypt_sym(sk, pl[1:8], 0, out_form=ca.NTT, key=key, stream_base=501), a[1:])     # (same plaintext, same stream: same ciphertext)
    # the secret-key streams are not the public-key encryptor's under the same key and base: no residue row of one shows up in the other
    p = E.encrypt_key(pk, pl[:8], key, stream_base=500)
    O = orc.Oracle(n, q, t)
    pn = np.stack([O.ct_to_ntt(p[i]) for i in range(8)])
    ac = E.encrypt_sym(sk, pl[:8], 0, key=key, stream_base=500)
    assert not np.array_equal(pn[:, 1], a[:, 1]) and not np.array_equal(p[:, 1], ac[:, 1])
    assert float((pn[:, 1] == a[:, 1]).mean()) < 1e-3 and float((p[:, 1] == ac[:, 1]).mean()) < 1e-3
    E.close()


def test_invalid_arguments_are_refused():
    n, q, t = 1024, _moduli(1024, 2), 1 << 16
    E = ca.Engine(n, q, t, device=-1)
    sk, _ = E.keygen(3)
    PU, PB = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    pl = np.zeros((1, n), dtype=np.uint64); ct = np.zeros((1, 2, 2, n), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(PU)
    key = (ctypes.c_uint8 * 32)()
    INVALID = -1
    L = E.L
    assert INVALID == L.crc_encrypt_sym(E.c, None, p(pl), 1, 5, ca.COEFF, p(ct)) == L.crc_encrypt_sym(E.c, p(sk), None, 1, 5, ca.COEFF, p(ct))
    assert INVALID == L.crc_encrypt_sym(E.c, p(sk), p(pl), 1, 5, ca.COEFF, None) == L.crc_encrypt_sym(None, p(sk), p(pl), 1, 5, ca.COEFF, p(ct))
    for form in (ca.NTTP, ca.NTTL, -1, 7):
        assert L.crc_encrypt_sym(E.c, p(sk), p(pl), 1, 5, form, p(ct)) == INVALID
        assert L.crc_encrypt_sym_key(E.c, p(sk), p(pl), 1, key, 0, form, p(ct)) == INVALID
    assert L.crc_encrypt_sym_key(E.c, p(sk), p(pl), 1, None, 0, ca.COEFF, p(ct)) == INVALID
    assert L.crc_encrypt_sym_key(E.c, None, p(pl), 1, key, 0, ca.COEFF, p(ct)) == INVALID
    assert not ct.any()                                      # nothing was written
    assert L.crc_encrypt_sym(E.c, p(sk), p(pl), 0, 5, ca.COEFF, p(ct)) == 0 and not ct.any()      # count 0: fine, writes nothing
    # device entry points on a host-only context: the error the neighbours return; the size queries need no device
    one = ctypes.c_void_p(8)
    assert L.crc_encrypt_sym_dev_forms(E.c, one, one, 1, 5, ca.COEFF, one, one, None) == L.crc_encrypt_dev_forms(E.c, one, one, 1, 5, ca.COEFF, one, one, None) == INVALID
    assert L.crc_encrypt_sym_dev_key_forms(E.c, one, one, 1, key, 0, ca.COEFF, one, one, None) == INVALID
    assert L.crc_refresh_sym_dev(E.c, one, one, 1, ca.COEFF, 5, ca.COEFF, one, None, one, None) == L.crc_refresh_dev(E.c, one, one, one, 1, ca.COEFF, 5, ca.COEFF, one, None, one, None) == INVALID
    assert L.crc_refresh_sym_dev_key(E.c, one, one, 1, ca.COEFF, key, 0, ca.COEFF, one, None, one, None) == INVALID
    assert E.encrypt_sym_dev_work_bytes(4) == 8 * 4 * 2 * n + 256 and L.crc_encrypt_sym_dev_work_bytes(None, 4) == 0
    assert E.refresh_sym_dev_work_bytes(4, ca.NTT) > 0 and E.refresh_sym_dev_work_bytes(4, 9) == 0 and L.crc_refresh_sym_dev_work_bytes(None, 4, ca.NTT) == 0
    assert E.refresh_sym_dev_work_bytes(40, ca.NTT) <= E.refresh_dev_work_bytes(40, ca.NTT)
    with pytest.raises(ca.CrcError):
        E.encrypt_sym(sk, pl, 5, out_form=9)
    E.close()
