"""The device decryptor (crc_decrypt_dev, kernels_decrypt.hip), its recode variant inside the refresh and the fractional codec around it, on the GPU, bit for
bit: the constructed scalar cases of tests/decrypt_model.py on all twelve parameter sets, dense size-2 and size-3 ciphertexts whose every operand is q_i - 1, more
ciphertexts than one launch of the scaling kernel takes (65535), refreshes of exhausted and of product-like ciphertexts, and the codec at t = 3, 65537 and
2^60 - 1.  The expected values are the model's; where Python integers would be slow, the host twin's, which tests/test_decrypt_cpu.py pins to the model."""
import random

import numpy as np
import pytest

import decrypt_model as dm
from test_decrypt_cpu import DENSE, SEED, SETS, W60, moduli, set_id, tables

pytestmark = pytest.mark.gpu

FORMS = ("COEFF", "NTT")


def decrypt_both_forms(E, sk, cts, size=2):
    """plaintexts [count][n] of crc_decrypt_dev from coefficient form and from NTT form (transformed on the device), into a pre-filled result; the input is
    left as it was"""
    import crcnn_amd as ca
    cts = np.ascontiguousarray(cts)
    count, n = cts.shape[0], E.n
    d_sk = E.upload(sk)
    out = {}
    for name in FORMS:
        form = getattr(ca, name)
        d_ct = E.upload(cts)
        if form == ca.NTT:
            E.ntt_fwd(d_ct, count, size=size)
            before = E.download(d_ct, cts.shape)
        else:
            before = cts
        d_pl = E.alloc(count * n * 8)
        E.L.crc_memset(E.c, E.p(d_pl), 0xff, count * n * 8, E.stream)
        d_w = E.alloc(E.decrypt_dev_work_bytes(count, size, form))
        E.decrypt_dev(d_sk, d_ct, count, d_pl, d_w, size=size, in_form=form)
        out[name] = E.download(d_pl, (count, n))
        assert np.array_equal(E.download(d_ct, cts.shape), before), name            # the input is not modified
        for d in (d_ct, d_pl, d_w):
            d.free()
    return out


@pytest.mark.parametrize("n, m, t", SETS, ids=[set_id(s) for s in SETS])
def test_scalar_cases(n, m, t):
    import crcnn_amd as ca
    q = moduli(m); k = len(q)
    cs = dm.cases(tuple(q), t, SEED)
    assert len(cs) == 241 + (2 if dm.GAMMA * t < dm.product(q) else 0)
    cts, want = dm.place(cs, q, n)
    E = ca.Engine(n, q, t, device=0)
    try:
        got = decrypt_both_forms(E, np.zeros((k, n), dtype=np.uint64), cts)
        for name in FORMS:
            wrong = [(j, cs[j].kind, int(got[name][j, 7 * j % n]), cs[j].m) for j in range(len(cs)) if not np.array_equal(got[name][j], want[j])]
            assert not wrong, (name, wrong[:10])
    finally:
        E.close()


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("n, m, t", DENSE + [(1024, 8, (1 << 60) - 1)], ids=[set_id(s) for s in DENSE + [(1024, 8, (1 << 60) - 1)]])
def test_dense_worst_case_operands(n, m, t, size):
    """at n = 1024 dec_dot_kernel loops and dec_gamma_kernel has several blocks per row; the expected plaintext there is the host twin's"""
    import crcnn_amd as ca
    q = moduli(m)
    E = ca.Engine(n, q, t, device=0)
    try:
        ct, sk, v = dm.dense_case(q, n, size, *tables(E), seed=SEED + size)
        want = E.decrypt(sk, ct, size=size) if n > 128 else np.array([dm.scale_rows(v, q, t)], dtype=np.uint64)
        got = decrypt_both_forms(E, sk, ct, size=size)
        for name in FORMS:
            assert np.array_equal(got[name], want), (name, np.flatnonzero(got[name][0] != want[0])[:10])
    finally:
        E.close()


def test_more_ciphertexts_than_one_launch_takes():
    """65538 ciphertexts: one full chunk of 65535 and a remainder of 3; ciphertext j carries a uniform residue vector at coefficient j mod n"""
    import crcnn_amd as ca
    n, t, count = 64, 1 << 20, 65538
    q = moduli(2); k = len(q)
    rng = np.random.default_rng(SEED)
    cts = np.zeros((count, 2, k, n), dtype=np.uint64)
    j = np.arange(count)
    for i, qi in enumerate(q):
        cts[j, 0, i, j % n] = rng.integers(0, qi, size=count, dtype=np.uint64)
    sk = np.zeros((k, n), dtype=np.uint64)
    E = ca.Engine(n, q, t, device=0)
    try:
        want = E.decrypt(sk, cts)
        for c in (0, 65534, 65535, 65536, 65537):                                   # the host twin, spot-checked against the model where the chunks meet
            assert [int(x) for x in want[c]] == dm.scale_rows(cts[c, 0], q, t)
        assert np.count_nonzero(want[65535:]) >= 3
        got = decrypt_both_forms(E, sk, cts)
        for name in FORMS:
            rows = np.flatnonzero((got[name] != want).any(axis=1))
            assert rows.size == 0, (name, rows[:10], rows[-10:])
    finally:
        E.close()


def negacyclic_product_mod_t(a, b, t):
    """a b mod (x^n + 1, t) for sparse a, b [n]"""
    n = len(a)
    out = [0] * n
    for i in np.flatnonzero(a):
        for j in np.flatnonzero(b):
            s, x = (i + j) % n, int(a[i]) * int(b[j])
            out[s] = (out[s] + (x if i + j < n else -x)) % t
    return out


def refresh_inputs(E, q, t, kind, cnt, seed):
    """c0 rows [cnt][k][n] (coefficient form) and the integers they hold.  "exhausted": uniform at all n coefficients.  "product": floor(q / t) m + e with m the
    product of two encodings (fraction digits at both ends of the polynomial, as mid-network ciphertexts have them) and e uniform in (-q / 4t, q / 4t) --
    returns m as well (else None)"""
    n, Q = E.n, dm.product(q)
    rnd = random.Random(seed)
    if kind == "exhausted":
        vs = [[rnd.randrange(Q) for _ in range(n)] for _ in range(cnt)]
        ms = None
    else:
        vals = (np.random.default_rng(seed).standard_normal(cnt) * 3).astype(np.float32)
        pl, _ = E.encode(vals)
        w, _ = E.encode(np.float32([0.37]))
        ms = [negacyclic_product_mod_t(pl[c], w[0], t) for c in range(cnt)]
        bound = Q // (4 * t)
        vs = [[(Q // t * x + rnd.randrange(-bound + 1, bound)) % Q for x in m] for m in ms]
    c0 = np.array([[[v % qi for v in row] for qi in q] for row in vs], dtype=np.uint64)
    return c0, ms


@pytest.mark.parametrize("kind", ["exhausted", "product"])
@pytest.mark.parametrize("n, m, t", [(128, 2, 65537), (128, 8, 1 << 44), (1024, 2, 1 << 20)], ids=["n128_k2_t65537", "n128_k8_t2e44", "n1024_k2_t2e20"])
def test_recode_inside_the_refresh(n, m, t, kind):
    """crc_refresh_sym_dev on ciphertexts (c0, c1 = 0): the floats are float32(decode(model plaintext)) -- with c0 uniform at all n coefficients a wrong index
    among the 96 that dec_recode_kernel scales cannot cancel -- and every refreshed ciphertext decrypts to encode(float); both forms in, both forms out.  The
    encoder's (long long) round(value) is undefined from 2^63 on: no expected value is that large (checked here, not assumed)"""
    import crcnn_amd as ca
    q = moduli(m); k = len(q)
    cnt = 40
    E = ca.Engine(n, q, t, device=0)
    try:
        sk, _ = E.keygen(31)
        c0, ms = refresh_inputs(E, q, t, kind, cnt, SEED + n + k)
        plain = np.array([dm.scale_rows(c0[c], q, t) for c in range(cnt)], dtype=np.uint64)
        if ms is not None:
            assert np.array_equal(plain, np.array(ms, dtype=np.uint64))            # the construction: noise below q / 4t rounds away
        dec = np.array([E.decode(plain[c]) for c in range(cnt)], dtype=np.float64)
        want_vals = dec.astype(np.float32)
        assert np.all(np.abs(want_vals.astype(np.float64)) < 2.0 ** 63), want_vals
        want_plain, _ = E.encode(want_vals)
        cts = np.zeros((cnt, 2, k, n), dtype=np.uint64)
        cts[:, 0] = c0
        d_sk = E.upload(sk)
        for in_form in (ca.COEFF, ca.NTT):
            d_in = E.upload(cts)
            if in_form == ca.NTT:
                E.ntt_fwd(d_in, cnt)
            for out_form in (ca.COEFF, ca.NTT):
                d_out = E.alloc(cts.nbytes); d_v = E.alloc(cnt * 4)
                E.L.crc_memset(E.c, E.p(d_out), 0xff, cts.nbytes, E.stream); E.L.crc_memset(E.c, E.p(d_v), 0xff, cnt * 4, E.stream)
                d_work = E.alloc(E.refresh_sym_dev_work_bytes(cnt, in_form))
                E.refresh_sym_dev(d_sk, d_in, cnt, 123, d_out, d_work, in_form=in_form, out_form=out_form, d_values=d_v)
                got_vals = E.download(d_v, (cnt,), dtype=np.float32)
                assert np.array_equal(got_vals.view(np.uint32), want_vals.view(np.uint32)), (in_form, out_form)
                if out_form == ca.NTT:
                    E.ntt_inv(d_out, cnt)
                assert np.array_equal(E.decrypt(sk, E.download(d_out, cts.shape)), want_plain), (in_form, out_form)
    finally:
        E.close()


EDGE = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 1 / 3, -1 / 3, 1e-9, -1e-9, 12345.678, -98765.4321, 3.0 ** -32, 0.49999997, 1e6 + 0.5, -1e6 - 0.25]


@pytest.mark.parametrize("t", [3, 65537, (1 << 60) - 1], ids=["t3", "t65537", "t2e60m1"])
def test_codec_at_the_ends_of_t(t):
    """crc_encode_dev_f32 / _f64 and crc_decode_dev against the host encoder where a digit -1 is t - 1 = 2 and where it is 2^60 - 2; and the decoder on
    arbitrary plaintexts"""
    import crcnn_amd as ca
    n = 128
    q = W60 if t >> 59 else moduli(2)
    E = ca.Engine(n, q, t, device=0)
    try:
        rng = np.random.default_rng(17)
        vals64 = np.concatenate([np.array(EDGE, dtype=np.float64), rng.standard_normal(2000) * 10.0 ** rng.integers(-6, 5, 2000)])
        for vals, f64 in ((vals64.astype(np.float32), False), (vals64, True)):
            want, _ = E.encode(vals, dtype=np.float64 if f64 else np.float32)
            d_v = E.upload(vals); d_p = E.alloc(vals.size * n * 8)
            E.L.crc_memset(E.c, E.p(d_p), 0xff, vals.size * n * 8, E.stream)
            E.encode_dev(d_v, vals.size, d_p, f64=f64)
            assert np.array_equal(E.download(d_p, (vals.size, n)), want), f64
            d_o = E.alloc(vals.size * 8)
            E.L.crc_memset(E.c, E.p(d_o), 0xff, vals.size * 8, E.stream)
            E.decode_dev(d_p, vals.size, d_o)
            host = np.array([E.decode(want[i]) for i in range(vals.size)])
            assert np.array_equal(E.download(d_o, (vals.size,), dtype=np.float64).view(np.uint64), host.view(np.uint64)), f64
        junk = rng.integers(0, t, size=(64, n), dtype=np.uint64)
        d_o = E.alloc(64 * 8)
        E.decode_dev(E.upload(junk), 64, d_o)
        assert np.array_equal(E.download(d_o, (64,), dtype=np.float64).view(np.uint64), np.array([E.decode(junk[i]) for i in range(64)]).view(np.uint64))
    finally:
        E.close()
