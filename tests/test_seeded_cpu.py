"""Seeded secret-key ciphertexts on the host (crc_encrypt_sym_seeded[_key], crc_seeded_expand, crc_seeded_ct_*; no GPU: host-only contexts).

A seeded batch is the c0 rows [count][k][n] (NTT form), a PUBLIC 32-byte seed and a stream base; c1 = A(seed, base + m) is regenerated from the seed.  The mask
comes from the public seed (ChaCha20 domain 6), the noise from the private key (domain 7).  The checker is the ORACLE (pinned to SEAL's Decryptor by
tests/test_oracle_golden.py); tests/test_gpu_seeded.py pins the device to the host twin checked here."""
import ctypes
import math

import numpy as np
import pytest

import crcnn_amd as ca
from oracle import orc
from test_encrypt_sym_cpu import IDS, _chi2_quantile, _derived_budget, _moduli, _plaintexts, param_sets

CARRY_BASE = (1 << 32) - 3          # + m carries into the high nonce word from m = 3 on


def _noise(E, O, sk, q, ctn, pl=None):
    """c0 + c1 s (- Delta m) of NTT-form ciphertexts, formed slot-wise in Python integers and taken back through the oracle's inverse transform (as
    test_encrypt_sym_cpu._noise_of_zero): [cnt][k][n] centred"""
    cnt, n, k, t = ctn.shape[0], E.n, len(q), E.t
    out = np.zeros((cnt, k, n), dtype=np.int64)
    delta, uhi = E.table("delta"), E.table("upper_half_increment")
    for i in range(k):
        qi = int(q[i])
        v = ((ctn[:, 0, i].astype(object) + ctn[:, 1, i].astype(object) * sk[i].astype(object)) % qi).astype(np.uint64)
        for m in range(cnt):
            e = O.ntt_inv(i, v[m]).astype(object)
            if pl is not None:
                p = pl[m].astype(object)
                e = (e - (int(delta[i]) * p + np.where(p >= (t + 1) // 2, int(uhi[i]), 0))) % qi
            e = np.where(e > qi // 2, e - qi, e)
            out[m, i] = e.astype(np.int64)
    return out


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_expansion_decrypts_under_the_oracle_with_the_derived_budget(n, q, t):
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(11)
    rng = np.random.default_rng(5)
    cnt = 12
    pl, max_mc = _plaintexts(E, n, q, t, cnt, rng)
    c0, seed, base = E.encrypt_sym_seeded(sk, pl, 77)
    assert c0.shape == (cnt, len(q), n) and len(seed) == 32 and base == 0 and seed == E.seeded_public_seed(77)
    ctn = E.seeded_expand(c0, seed, base, ca.NTT)
    ct = E.seeded_expand(c0, seed, base, ca.COEFF)
    assert ct.shape == (cnt, 2, len(q), n)
    assert np.array_equal(ctn[:, 0], c0)                     # the rows that travelled ARE the NTT-form c0
    assert np.array_equal(ctn, np.stack([O.ct_to_ntt(ct[i]) for i in range(cnt)]))
    assert np.array_equal(np.stack([O.decrypt(sk, ct[i]) for i in range(cnt)]), pl)
    assert np.array_equal(np.stack([O.decrypt(sk, O.ct_from_ntt(ctn[i])) for i in range(cnt)]), pl)
    bound = _derived_budget(q, t, max_mc)
    b = [O.noise_budget(sk, ct[i]) for i in range(cnt)]
    print("budget", IDS[param_sets().index((n, q, t))], "derived bound", bound, "seeded", b)
    assert min(b) >= bound, (b, bound)
    # the key-based entry point, a stream base of its own
    key, pub = E.random_key(), E.random_key()
    c0k, sd, bs = E.encrypt_sym_seeded(sk, pl, 0, key=key, public_seed=pub, stream_base=1000)
    assert sd == pub and bs == 1000
    ck = E.seeded_expand(c0k, pub, 1000, ca.COEFF)
    assert np.array_equal(np.stack([O.decrypt(sk, ck[i]) for i in range(cnt)]), pl)
    assert min(O.noise_budget(sk, ck[i]) for i in range(cnt)) >= bound
    E.close()


def test_who_depends_on_what():
    n, q, t = 1024, _moduli(1024, 2), 1 << 16
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(21); sk2, _ = E.keygen(22)
    rng = np.random.default_rng(8)
    cnt = 6
    pl = rng.integers(0, t, size=(cnt, n), dtype=np.uint64); pl2 = rng.integers(0, t, size=(cnt, n), dtype=np.uint64)
    k1, k2, s1, s2 = bytes(range(32)), bytes(range(1, 33)), bytes(range(100, 132)), bytes(range(101, 133))
    base = 40

    def c1(seed, b):
        return E.seeded_expand(np.zeros((cnt, len(q), n), dtype=np.uint64), seed, b, ca.NTT)[:, 1]

    A = c1(s1, base)
    # c1 is a function of (seed, base) alone: the expansion never sees a key, a plaintext or a secret key, and what the encryptor masked with is that A
    for key, plain, secret in ((k1, pl, sk), (k2, pl, sk), (k1, pl2, sk), (k1, pl, sk2)):
        c0, _, _ = E.encrypt_sym_seeded(secret, plain, 0, key=key, public_seed=s1, stream_base=base)
        ctn = E.seeded_expand(c0, s1, base, ca.NTT)
        assert np.array_equal(ctn[:, 1], A)
        assert np.array_equal(np.stack([O.decrypt(secret, O.ct_from_ntt(ctn[i])) for i in range(cnt)]), plain)
    assert not np.array_equal(c1(s2, base), A) and float((c1(s2, base) == A).mean()) < 1e-3
    B = c1(s1, base + 1)
    assert not np.array_equal(B, A) and np.array_equal(B[:-1], A[1:])          # stream m under base b + 1 is stream m + 1 under base b
    assert len({A[m].tobytes() for m in range(cnt)}) == cnt
    # the noise polynomial c0 + c1 s - Delta m: a function of the private key, not of the public seed; the same small integers under every modulus
    e1 = _noise(E, O, sk, q, E.seeded_expand(E.encrypt_sym_seeded(sk, pl, 0, key=k1, public_seed=s1, stream_base=base)[0], s1, base), pl)
    e2 = _noise(E, O, sk, q, E.seeded_expand(E.encrypt_sym_seeded(sk, pl, 0, key=k1, public_seed=s2, stream_base=base)[0], s2, base), pl)
    e3 = _noise(E, O, sk, q, E.seeded_expand(E.encrypt_sym_seeded(sk, pl, 0, key=k2, public_seed=s1, stream_base=base)[0], s1, base), pl)
    assert np.array_equal(e1, e2) and not np.array_equal(e1, e3)
    assert all(np.array_equal(e1[:, i], e1[:, 0]) for i in range(len(q)))
    assert e1.min() >= -19 and e1.max() <= 19 and e1.any()
    E.close()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_mask_stream_is_what_the_header_says(n, q, t):
    """A[i][s + c] = z mod q_i, z the 128-bit little-endian integer of words 4c .. 4c + 3 of the half (i odd: words 8..15) of block i // 2 of the stream
    nonce = (sid low, sid high, 6 << 24 | s) under the PUBLIC seed, sid = stream_base + m"""
    k = len(q)
    E = ca.Engine(n, q, t, device=-1)
    seed = bytes((7 * j + 3) & 0xff for j in range(32))
    cnt = 8
    A = E.seeded_expand(np.zeros((cnt, k, n), dtype=np.uint64), seed, CARRY_BASE, ca.NTT)[:, 1]
    PB = ctypes.POINTER(ctypes.c_uint8)
    keyb = (ctypes.c_uint8 * 32).from_buffer_copy(seed)

    def expect(m, s, i):
        sid = CARRY_BASE + m
        pair = s & ~1
        nonce = (ctypes.c_uint8 * 12).from_buffer_copy((sid & 0xffffffff).to_bytes(4, "little") + (sid >> 32).to_bytes(4, "little")
                                                       + ((6 << 24) | pair).to_bytes(4, "little"))
        out = (ctypes.c_uint8 * 64)()
        assert E.L.crc_chacha20_block(ctypes.cast(keyb, PB), i // 2, ctypes.cast(nonce, PB), ctypes.cast(out, PB)) == 0
        off = 32 * (i & 1) + 16 * (s & 1)
        return int.from_bytes(bytes(out)[off:off + 16], "little") % int(q[i])

    # (before the carry, slot 0; after it, the last modulus -- odd and even k occur among the sets --, an odd slot of the last pair; the middle of the ring)
    for m, s, i in [(0, 0, 0), (cnt - 1, n - 1, k - 1), (3, n // 2 + 4, (k - 1) // 2), (5, 7, min(1, k - 1))]:
        assert (CARRY_BASE + m) >> 32 == (1 if m >= 3 else 0)
        assert int(A[m, i, s]) == expect(m, s, i), (m, s, i)
    E.close()


def test_domains_are_disjoint():
    n, q, t = 1024, _moduli(1024, 2), 1 << 16
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(31)
    one = bytes((11 * j + 5) & 0xff for j in range(32)); other = bytes(range(32))
    cnt, base = 6, 9
    zeros = np.zeros((cnt, n), dtype=np.uint64)
    sym = E.encrypt_sym(sk, zeros, 0, out_form=ca.NTT, key=one, stream_base=base)                       # `one` as the key of crc_encrypt_sym_key
    as_seed = E.seeded_expand(E.encrypt_sym_seeded(sk, zeros, 0, key=other, public_seed=one, stream_base=base)[0], one, base)     # as the public seed
    as_key = E.seeded_expand(E.encrypt_sym_seeded(sk, zeros, 0, key=one, public_seed=other, stream_base=base)[0], other, base)    # as the private key
    rows = lambda c: {c[m, 1, i].tobytes() for m in range(cnt) for i in range(len(q))}
    assert not rows(sym) & rows(as_seed) and not rows(sym) & rows(as_key) and not rows(as_seed) & rows(as_key)
    assert float((sym[:, 1] == as_seed[:, 1]).mean()) < 1e-3
    # the attack needs equal noise under the two encryptors: the noise of crc_encrypt_sym_key and of the seeded encryptor under the same private key differ
    e_sym, e_seeded = _noise(E, O, sk, q, sym), _noise(E, O, sk, q, as_key)
    assert max(abs(e_sym).max(), abs(e_seeded).max()) <= 19
    assert not np.array_equal(e_sym, e_seeded) and float((e_sym == e_seeded).mean()) < 0.2           # (independent draws agree with probability ~ 0.09)
    # ... and the seeded noise is not the mask stream's block under the same bytes either (domain 6 vs 7): key == seed is refused outright
    c0 = np.zeros((cnt, len(q), n), dtype=np.uint64)
    PU, PB = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    kb = (ctypes.c_uint8 * 32).from_buffer_copy(one); kb2 = (ctypes.c_uint8 * 32).from_buffer_copy(one)
    assert E.L.crc_encrypt_sym_seeded_key(E.c, sk.ctypes.data_as(PU), zeros.ctypes.data_as(PU), cnt, kb, kb2, base, c0.ctypes.data_as(PU)) == -1
    assert not c0.any()
    with pytest.raises(ca.CrcError):
        E.encrypt_sym_seeded(sk, zeros, 0, key=one, public_seed=one, stream_base=base)
    E.close()


def test_mask_is_uniform_and_noise_follows_the_clipped_truncated_normal():
    """the chi-square tests of test_encrypt_sym_cpu.py, same cell rules and bounds: 64 bins per modulus on 2^20 residues against the 0.9999 quantile at 63
    degrees of freedom, the noise law over 2^19 draws against 80"""
    n, q, t = 4096, _moduli(4096, 2), 1 << 29
    k = len(q)
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(14)
    cnt = 256
    zeros = np.zeros((cnt, n), dtype=np.uint64)
    c0, seed, base = E.encrypt_sym_seeded(sk, zeros, 31337)
    ctn = E.seeded_expand(c0, seed, base, ca.NTT)
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
        print("seeded c1 chi-square, modulus", i, chi, "bound", bound)
        assert chi < bound, (i, chi)
    e = _noise(E, O, sk, q, ctn[:128])
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
    print("seeded noise chi-square", chi, "cells", cells)
    assert chi < 80, (chi, cells, counts)
    E.close()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_container_round_trip_and_refusals(n, q, t):
    k = len(q)
    E = ca.Engine(n, q, t, device=-1)
    sk, _ = E.keygen(5)
    rng = np.random.default_rng(2)
    cnt = 8
    pl, _ = _plaintexts(E, n, q, t, cnt, rng)
    c0, seed, _ = E.encrypt_sym_seeded(sk, pl, 9)
    base = CARRY_BASE + 12345
    blob = E.seeded_save(c0, seed, base)
    # a fixed header of at most 128 bytes plus the rows; less than 0.51 of the SEAL form of the same ciphertexts from eight on
    for c in (0, 1, 8, 784):
        assert E.seeded_bytes(c) - c * k * n * 8 == E.seeded_bytes(0) <= 128
    assert len(blob) == E.seeded_bytes(cnt)
    E.L.crc_seal_ct_bytes.restype = ctypes.c_size_t
    for c in (8, 9, 784):
        assert E.seeded_bytes(c) < 0.51 * c * E.L.crc_seal_ct_bytes(E.c, 2), (c, E.seeded_bytes(c))
    r0, rs, rb = E.seeded_load(blob)
    assert np.array_equal(r0, c0) and rs == seed and rb == base
    assert E.seeded_save(r0, rs, rb) == blob
    # refusals write nothing
    PU, PB = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    hash_off = blob.index(np.array(_hash(E), dtype=np.uint64).tobytes())
    bad_hash = bytearray(blob); bad_hash[hash_off + 5] ^= 0x10
    wrong_count = bytearray(blob); cnt_off = hash_off + 32
    assert int.from_bytes(blob[cnt_off:cnt_off + 8], "little") == cnt
    wrong_count[cnt_off:cnt_off + 8] = (cnt - 1).to_bytes(8, "little")
    more = bytearray(blob); more[cnt_off:cnt_off + 8] = (cnt + 1).to_bytes(8, "little")
    huge = bytearray(blob); huge[cnt_off:cnt_off + 8] = (1 << 63).to_bytes(8, "little")
    for bad in (bytes(bad_hash), blob[:-8], blob[:40], blob[:E.seeded_bytes(0)][:-1], bytes(wrong_count), bytes(more), bytes(huge), blob + b"\0" * 8,
                b"X" + blob[1:]):
        rows = np.zeros((cnt + 1, k, n), dtype=np.uint64); sd = (ctypes.c_uint8 * 32)(); got = ctypes.c_size_t(77); b = ctypes.c_uint64(55)
        raw = np.frombuffer(bad, dtype=np.uint8).copy()
        assert E.L.crc_seeded_ct_load(E.c, raw.ctypes.data, raw.nbytes, rows.ctypes.data_as(PU), cnt + 1, ctypes.byref(got), sd, ctypes.byref(b)) == -1
        assert not rows.any() and not any(sd) and got.value == 77 and b.value == 55
        with pytest.raises(ca.CrcError):
            E.seeded_load(bad)
    # too small a destination
    rows = np.zeros((cnt, k, n), dtype=np.uint64); sd = (ctypes.c_uint8 * 32)(); got = ctypes.c_size_t(77); b = ctypes.c_uint64(55)
    raw = np.frombuffer(blob, dtype=np.uint8).copy()
    assert E.L.crc_seeded_ct_load(E.c, raw.ctypes.data, raw.nbytes, rows.ctypes.data_as(PU), cnt - 1, ctypes.byref(got), sd, ctypes.byref(b)) == -1 and not rows.any()
    # another parameter set refuses the blob (the hash)
    F = ca.Engine(n, q, t + 2 if t % 2 == 0 else t + 1, device=-1) if n == 1024 else None
    if F is not None:
        with pytest.raises(ca.CrcError):
            F.seeded_load(blob)
        F.close()
    E.close()


def _hash(E):
    h = (ctypes.c_uint64 * 4)()
    assert E.L.crc_params_hash(E.c, h) == 0
    return list(h)


def test_invalid_arguments_are_refused():
    n, q, t = 1024, _moduli(1024, 2), 1 << 16
    E = ca.Engine(n, q, t, device=-1)
    sk, _ = E.keygen(3)
    PU = ctypes.POINTER(ctypes.c_uint64)
    pl = np.zeros((1, n), dtype=np.uint64); c0 = np.zeros((1, 2, n), dtype=np.uint64); ct = np.zeros((1, 2, 2, n), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(PU)
    key = (ctypes.c_uint8 * 32)(); seed = (ctypes.c_uint8 * 32)(*([1] * 32))
    INVALID = -1
    L = E.L
    assert INVALID == L.crc_encrypt_sym_seeded(E.c, None, p(pl), 1, 5, p(c0)) == L.crc_encrypt_sym_seeded(E.c, p(sk), None, 1, 5, p(c0))
    assert INVALID == L.crc_encrypt_sym_seeded(E.c, p(sk), p(pl), 1, 5, None) == L.crc_encrypt_sym_seeded(None, p(sk), p(pl), 1, 5, p(c0))
    assert L.crc_encrypt_sym_seeded_key(E.c, p(sk), p(pl), 1, None, seed, 0, p(c0)) == INVALID
    assert L.crc_encrypt_sym_seeded_key(E.c, p(sk), p(pl), 1, key, None, 0, p(c0)) == INVALID
    assert L.crc_encrypt_sym_seeded_key(E.c, None, p(pl), 1, key, seed, 0, p(c0)) == INVALID
    assert L.crc_encrypt_sym_seeded_key(None, p(sk), p(pl), 1, key, seed, 0, p(c0)) == INVALID
    assert not c0.any()
    assert L.crc_encrypt_sym_seeded(E.c, p(sk), p(pl), 0, 5, p(c0)) == 0 and not c0.any()              # count 0: fine, writes nothing
    assert L.crc_encrypt_sym_seeded_key(E.c, p(sk), p(pl), 0, key, seed, 0, p(c0)) == 0 and not c0.any()
    assert L.crc_seeded_public_seed(5, None) == INVALID
    c0[:] = 3
    for form in (ca.NTTP, ca.NTTL, -1, 7):
        assert L.crc_seeded_expand(E.c, p(c0), 1, seed, 0, form, p(ct)) == INVALID
    assert INVALID == L.crc_seeded_expand(E.c, None, 1, seed, 0, ca.NTT, p(ct)) == L.crc_seeded_expand(E.c, p(c0), 1, None, 0, ca.NTT, p(ct))
    assert INVALID == L.crc_seeded_expand(E.c, p(c0), 1, seed, 0, ca.NTT, None) == L.crc_seeded_expand(None, p(c0), 1, seed, 0, ca.NTT, p(ct))
    assert L.crc_seeded_expand(E.c, p(c0), 0, seed, 0, ca.NTT, p(ct)) == 0
    assert not ct.any()
    # the device entry point on a host-only context: the error the neighbours return, whatever else is wrong or right
    one = ctypes.c_void_p(16)
    assert L.crc_seeded_expand_dev(E.c, one, 1, seed, 0, ca.NTT, ctypes.c_void_p(1 << 20), None) == INVALID \
        == L.crc_encrypt_sym_dev_forms(E.c, one, one, 1, 5, ca.COEFF, one, one, None)
    assert L.crc_seeded_expand_dev(E.c, one, 0, seed, 0, ca.NTT, ctypes.c_void_p(1 << 20), None) == INVALID
    assert L.crc_seeded_expand_dev(None, one, 1, seed, 0, ca.NTT, ctypes.c_void_p(1 << 20), None) == INVALID
    assert L.crc_seeded_ct_bytes(None, 4) == 0
    buf = np.zeros(E.seeded_bytes(1), dtype=np.uint8); w = ctypes.c_size_t(0)
    assert L.crc_seeded_ct_save(E.c, p(c0), 1, seed, 0, buf.ctypes.data, buf.nbytes - 1, ctypes.byref(w)) == INVALID and not buf.any()      # too small a buffer
    assert w.value == E.seeded_bytes(1)
    assert L.crc_seeded_ct_save(E.c, None, 1, seed, 0, buf.ctypes.data, buf.nbytes, None) == INVALID
    assert L.crc_seeded_ct_save(E.c, p(c0), 1, None, 0, buf.ctypes.data, buf.nbytes, None) == INVALID
    assert L.crc_seeded_ct_save(E.c, p(c0), 1, seed, 0, None, buf.nbytes, None) == INVALID and not buf.any()
    with pytest.raises(ca.CrcError):
        E.seeded_expand(c0, bytes(seed), 0, out_form=9)
    E.close()
