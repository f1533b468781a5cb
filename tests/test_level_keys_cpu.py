"""Key-switching keys of a lower level derived from the upper level's, on the host (crc_ctx_create_level, crc_keys_restrict, crc_seeded_keys_expand_level; no GPU:
host-only contexts).

A derived level is a prefix context whose key-switching gadget stays the parent's; the parent's blobs restricted to the first P' pairs and k' rows are its keys
(tests/level_keys_model.py).  tests/test_gpu_level_keys.py pins the device to the host twins checked here."""
import os
import subprocess

import numpy as np
import pytest

import crcnn_amd as ca
import galois_model as gm
import level_keys_model as lk
from oracle import orc
from test_seeded_keys_cpu import target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [0xffffe80001, 0xffffc40001, 0xffffffffffc0001]          # the SMALL primes of test_gpu_mod_switch.py
T = 65537
INVALID, PARAMETERS = -1, -2
POISON = np.uint64(0xabababababababab)
CLIP = 19                                                          # both samplers: sigma = 3.19 clipped at 6 sigma


def test_a_derived_level_is_the_prefix_context_with_the_parents_gadget():
    n = 256
    A = ca.Engine(n, SMALL, T, device=-1)
    assert A.key_moduli == 3 and np.array_equal(A.table("key_q"), A.q) and np.array_equal(A.table("ksk_inv_qhat"), A.table("inv_qhat"))
    for kept in (2, 1):
        B, C = A.derived_level(kept), A.level(kept)
        assert B.k == kept and B.n == n and B.t == T and B.kbsk == C.kbsk
        assert B.key_moduli == 3 and C.key_moduli == kept
        names = ["q", "root", "const_ratio", "delta", "upper_half_increment", "bsk", "bsk_root", "f64_primes", "sq64_primes", "inv_qhat"]
        names += [f"root_powers:{i}" for i in range(kept + B.kbsk)] + [f"inv_root_powers_div_two:{i}" for i in range(kept + B.kbsk)]
        for name in names:
            assert np.array_equal(B.table(name), C.table(name)), (kept, name)
        assert np.array_equal(B.table("key_q"), A.q) and np.array_equal(C.table("key_q"), C.q)
        assert [int(v) for v in B.table("ksk_inv_qhat")] == lk.prescale(SMALL, kept)
        assert [int(v) for v in C.table("ksk_inv_qhat")] == lk.prescale(SMALL[:kept], kept) == [int(v) for v in C.table("inv_qhat")]
        assert not np.array_equal(B.table("ksk_inv_qhat"), B.table("inv_qhat"))
        assert A.mod_switch_supported(B) and A.mod_switch_supported(C)
        assert A.keys_restrict_supported(B) and not A.keys_restrict_supported(C) and not B.keys_restrict_supported(A) and not A.keys_restrict_supported(A)
        # encryption, decryption and the switch itself do not see the gadget
        sk, pk = A.keygen(3)
        m = np.random.RandomState(kept).randint(0, T, size=(2, n)).astype(np.uint64)
        ct = A.encrypt(pk, m, 4)
        low = A.mod_switch(B, ct)
        assert np.array_equal(low, A.mod_switch(C, ct)) and np.array_equal(B.decrypt(np.ascontiguousarray(sk[:kept]), low), m)
        B.close(); C.close()
    # a level of a level keeps the top gadget, and is a level of both
    B = A.derived_level(2); D = B.derived_level(1); D2 = A.derived_level(1)
    assert D.key_moduli == 3 and np.array_equal(D.table("key_q"), A.q) and np.array_equal(D.table("ksk_inv_qhat"), D2.table("ksk_inv_qhat"))
    assert A.keys_restrict_supported(D) and B.keys_restrict_supported(D) and B.keys_restrict_supported(D2) and not D.keys_restrict_supported(D2)
    with pytest.raises(ValueError):
        A.derived_level(3)
    with pytest.raises(ValueError):
        A.derived_level(0)
    c = ca.binding.VP()
    assert A.L.crc_ctx_create_level(A.c, 3, -1, c) == PARAMETERS and not c.value and A.L.crc_ctx_create_level(A.c, 0, -1, c) == PARAMETERS
    assert A.L.crc_ctx_create_level(None, 1, -1, c) == INVALID and A.L.crc_ctx_create_level(A.c, 1, -1, None) == INVALID
    # an ordinary context's relinearisation digits are cut with the constant they always were: the oracle's host relinearisation under an unrestricted key
    O = orc.Oracle(n, SMALL, T)
    sk, pk = A.keygen(3)
    ct3 = O.square(A.encrypt(pk, np.arange(n, dtype=np.uint64)[None] % 7, 5)[0])
    evk = A.gen_evk(6, sk)
    assert np.array_equal(lk.relinearize(O, ct3, evk, [int(v) for v in A.table("ksk_inv_qhat")]), O.relinearize(ct3, evk))
    for e in (A, B, D, D2):
        e.close()


RESTRICT = [("n256_3to2_dbc16", 256, SMALL, 2, 16), ("n256_3to2_dbc8", 256, SMALL, 2, 8), ("n256_3to1_dbc16", 256, SMALL, 1, 16), ("n256_3to1_dbc8", 256, SMALL, 1, 8),
            ("n256_2to1_dbc16", 256, SMALL[:2], 1, 16), ("n256_2to1_dbc8", 256, SMALL[:2], 1, 8), ("n16384_4to3", 16384, 4, 3, 16)]


@pytest.mark.parametrize("case", RESTRICT, ids=[c[0] for c in RESTRICT])
def test_restriction_is_slicing(case):
    _, n, q, kept, dbc = case
    q = ca.default_coeff_modulus_128(16384)[:q] if isinstance(q, int) else q
    A = ca.Engine(n, q, T, device=-1); B = A.derived_level(kept)
    n_keys = 3 if n == 256 else 1
    w = A.L.crc_evk_words(A.c, dbc)
    assert w == 2 * lk.pairs(q, len(q), dbc) * len(q) * n and B.L.crc_evk_words(B.c, dbc) == 2 * lk.pairs(q, kept, dbc) * kept * n
    keys = np.random.RandomState(n + kept + dbc).randint(0, 1 << 62, size=(n_keys, w), dtype=np.int64).astype(np.uint64)
    got = A.keys_restrict(B, keys, dbc=dbc)
    assert got.shape == (n_keys, B.L.crc_evk_words(B.c, dbc)) and np.array_equal(got, lk.restrict(keys, n, q, kept, dbc))
    A.close(); B.close()


def minus_e(E, O, sk, factor_at, kid, p, first_p, second_p):
    """(first + second s - [j == l] factor w) of one pair over E's moduli, inverse-transformed by the oracle and centred: [k][n].  factor_at: (l, factor)"""
    l, factor = factor_at
    w = target(E, sk, [int(v) for v in E.q], kid)
    out = np.zeros((E.k, E.n), dtype=np.int64)
    for j in range(E.k):
        qj = int(E.q[j])
        v = first_p[j].astype(object) + second_p[j].astype(object) * sk[j].astype(object)
        if j == l:
            v = v - factor * w[j]
        c = O.ntt_inv(j, (v % qj).astype(np.uint64)).astype(object)
        out[j] = np.where(c > qj // 2, c - qj, c).astype(np.int64)
    return out


@pytest.mark.parametrize("kept,dbc", [(2, 16), (2, 8), (1, 16)])
def test_restricted_keys_are_keys_of_the_level_for_the_parents_gadget(kept, dbc):
    """every pair of a restricted evaluation and Galois key: first + second s - [j == l] (Q / q_l) 2^(dbc d) w = -e with the parent pair's own e"""
    n, q = 256, SMALL
    k = len(q)
    A = ca.Engine(n, q, T, device=-1); B = A.derived_level(kept)
    OA, OB = orc.Oracle(n, q, T), orc.Oracle(n, q[:kept], T)
    sk, _ = A.keygen(3)
    skB = np.ascontiguousarray(sk[:kept])
    elts = [3, 2 * n - 1]
    _, gk = A.gen_galois_keys(8, sk, dbc=dbc, elts=elts)
    keys = np.concatenate([A.gen_evk(7, sk, dbc=dbc)[None], gk])
    ids = [0] + elts
    low = A.keys_restrict(B, keys, dbc=dbc)
    PA, PB = lk.pairs(q, k, dbc), lk.pairs(q, kept, dbc)
    fa, fb = lk.gadget_factors(q, k, dbc), lk.gadget_factors(q, kept, dbc)
    assert [f[:2] for f in fa[:PB]] == [f[:2] for f in fb] and all(x[2] == y[2] for x, y in zip(fa, fb)) and len(fa) == PA and len(fb) == PB
    own = lk.gadget_factors(q[:kept], kept, dbc)                   # the level's own gadget is another one
    assert all(x[2] != y[2] for x, y in zip(own, fb))
    up = keys.reshape(len(ids), PA, 2, k, n); dn = low.reshape(len(ids), PB, 2, kept, n)
    for e, kid in enumerate(ids):
        for p in range(PB):
            l, _, factor = fb[p]
            eB = -minus_e(B, OB, skB, (l, factor), kid, p, dn[e, p, 0], dn[e, p, 1])
            eA = -minus_e(A, OA, sk, (l, factor), kid, p, up[e, p, 0], up[e, p, 1])
            assert all(np.array_equal(eA[j], eA[0]) for j in range(k)), (kid, p)
            assert all(np.array_equal(eB[j], eA[0]) for j in range(kept)), (kid, p)
            assert abs(eB).max() <= CLIP and eB.any(), (kid, p)
    A.close(); B.close()


def test_a_key_switch_at_the_derived_level_decrypts():
    """encrypt under three moduli, switch to two and to one; rotate and (where the level has the room: two moduli) relinearise a square there in the model with
    RESTRICTED keys and the parent's pre-scale constants: the results decrypt, and with the level's own constants (what a plain prefix context cuts digits with)
    they do not.  One 40-bit modulus leaves 40 - 13 - 9 bits after the switch: the rotation there runs at digit width 8"""
    n, q = 256, SMALL
    t = ca.Engine.slots_prime(n, 13)
    A = ca.Engine(n, q, t, device=-1)
    sk, pk = A.keygen(31)
    rng = np.random.RandomState(2)
    v = rng.randint(-40, 41, size=(1, n)).astype(np.int64)
    ct = A.encrypt(pk, A.slots_compose(v, 1, n, n, 1), 77)
    g = gm.elt_rows(n, 1)
    for kept, dbc in ((2, 16), (1, 8)):
        _, gk = A.gen_galois_keys(8, sk, dbc=dbc, elts=[g])
        evk = A.gen_evk(7, sk, dbc=dbc)
        B = A.derived_level(kept); OB = orc.Oracle(n, q[:kept], t)
        skB = np.ascontiguousarray(sk[:kept])
        low = A.mod_switch(B, ct)[0]
        keys = A.keys_restrict(B, np.stack([evk, gk[0]]), dbc=dbc)
        pre = [int(x) for x in B.table("ksk_inv_qhat")]
        assert pre == lk.prescale(q, kept)
        y = lk.apply_galois(OB, low, g, keys[1], pre, dbc)
        assert B.noise_budget(skB, y) > 0, kept
        assert np.array_equal(B.slots_decompose(B.decrypt(skB, y[None]), n, n, 1).reshape(1, n), gm.rotate_rows_slots(v, 1)), kept
        bad = lk.apply_galois(OB, low, g, keys[1], lk.prescale(q[:kept], kept), dbc)
        assert B.noise_budget(skB, bad) == 0, kept
        if kept == 2:
            r = lk.relinearize(OB, OB.square(low), keys[0], pre, dbc)
            assert B.noise_budget(skB, r) > 0
            assert np.array_equal(B.slots_decompose(B.decrypt(skB, r[None]), n, n, 1).reshape(1, n), v * v)
        B.close()
    A.close()


@pytest.mark.parametrize("kept,dbc", [(2, 16), (2, 8), (1, 16)])
def test_the_seeded_route_is_restrict_of_expand(kept, dbc):
    n, q = 256, SMALL
    A = ca.Engine(n, q, T, device=-1); B = A.derived_level(kept)
    sk, _ = A.keygen(3)
    ids = [0, 1, 3, 2 * n - 1, pow(3, -1, 2 * n)]
    first, pub = A.gen_keys_seeded(4, sk, ids, dbc=dbc)
    assert np.array_equal(A.seeded_keys_expand_level(B, first, ids, pub, dbc=dbc), A.keys_restrict(B, A.seeded_keys_expand(first, ids, pub, dbc=dbc), dbc=dbc))
    assert np.array_equal(A.seeded_keys_expand_level(B, first[2:], ids[2:], pub, dbc=dbc, conjugate=True),
                          A.keys_restrict(B, A.seeded_keys_expand(first[2:], ids[2:], pub, dbc=dbc, conjugate=True), dbc=dbc))
    # conjugation commutes with restriction: the level conjugates its own restricted keys to the same blobs
    plain = A.keys_restrict(B, A.seeded_keys_expand(first[2:], ids[2:], pub, dbc=dbc), dbc=dbc)
    assert np.array_equal(B.galois_conjugate_keys(ids[2:], plain, dbc=dbc), A.seeded_keys_expand_level(B, first[2:], ids[2:], pub, dbc=dbc, conjugate=True))
    A.close(); B.close()


def test_refusals_write_nothing():
    n, dbc = 256, 16
    pu = ca.binding._pu
    A = ca.Engine(n, SMALL, T, device=-1); B = A.derived_level(2); C = A.level(2)
    other = ca.Engine(n, SMALL[:2] + [ca.default_coeff_modulus_128(8192)[0]], T, device=-1)       # the same two first primes under another parent
    assert [int(v) for v in other.q[:2]] == SMALL[:2] and int(other.q[2]) != SMALL[2]
    B2 = other.derived_level(2)
    sk, _ = A.keygen(3)
    skB = np.ascontiguousarray(sk[:2])
    ids = np.array([0, 3, 2 * n - 1], dtype=np.uint64)
    first, pub = A.gen_keys_seeded(4, sk, ids, dbc=dbc)
    keys = A.seeded_keys_expand(first, ids, pub, dbc=dbc)
    wA, wB = A.L.crc_evk_words(A.c, dbc), B.L.crc_evk_words(B.c, dbc)
    out = np.full((ids.size, wA), POISON, dtype=np.uint64)         # (room for a parent-sized write, should one happen)
    L = A.L
    seed = A._key(pub)

    def res(f=A.c, t=B.c, kk=pu(keys), m=ids.size, d=dbc, o=pu(out)):
        return L.crc_keys_restrict(f, t, kk, m, d, o)

    def exl(f=A.c, t=B.c, fr=pu(first), i=pu(ids), m=ids.size, d=dbc, sd=seed, conj=0, o=pu(out)):
        return L.crc_seeded_keys_expand_level(f, t, fr, i, m, d, sd, conj, o)

    for call in (res, exl):
        assert call(t=C.c) == INVALID                              # a plain prefix context: its gadget is its own
        assert call(t=B2.c) == INVALID                             # an equal prefix under another parent
        assert call(t=A.c) == INVALID and call(f=B.c, t=A.c) == INVALID and call(f=None) == INVALID and call(t=None) == INVALID
        assert call(d=0) == INVALID and call(d=61) == INVALID and call(m=-1) == INVALID and call(o=None) == INVALID
    assert res(kk=None) == INVALID and exl(fr=None) == INVALID and exl(i=None) == INVALID and exl(sd=None) == INVALID and exl(conj=2) == INVALID
    assert exl(conj=1) == INVALID                                  # id 0 has no conjugated key
    assert not L.crc_keys_restrict_supported(A.c, C.c) and not L.crc_keys_restrict_supported(A.c, B2.c) and not L.crc_keys_restrict_supported(other.c, B.c)
    assert not L.crc_keys_restrict_supported(None, B.c) and not L.crc_keys_restrict_supported(A.c, None)
    assert (out == POISON).all()
    # overlap: the output inside the input, and the input inside the output
    buf = np.full(ids.size * (wA + wB), POISON, dtype=np.uint64)
    buf[:keys.size] = keys.reshape(-1)
    snapshot = buf.copy()
    assert L.crc_keys_restrict(A.c, B.c, pu(buf), ids.size, dbc, pu(buf)) == INVALID
    assert L.crc_keys_restrict(A.c, B.c, pu(buf), ids.size, dbc, pu(buf[keys.size - 2:])) == INVALID
    assert L.crc_keys_restrict(A.c, B.c, pu(buf[2:]), ids.size, dbc, pu(buf)) == INVALID
    assert L.crc_seeded_keys_expand_level(A.c, B.c, pu(buf), pu(ids), ids.size, dbc, seed, 0, pu(buf[first.size - 2:])) == INVALID
    assert np.array_equal(buf, snapshot)
    assert L.crc_keys_restrict(A.c, B.c, pu(buf), ids.size, dbc, pu(buf[keys.size:])) == 0          # adjacent is fine
    assert np.array_equal(buf[keys.size:].reshape(ids.size, wB), lk.restrict(keys, n, SMALL, 2, dbc))
    # n_keys = 0 is a no-op
    assert res(m=0) == 0 and exl(m=0) == 0 and res(m=0, kk=None, o=None) == 0 and (out == POISON).all()
    # generation on a derived context: every entry point, nothing written
    rows = np.full((ids.size, wB // 2), POISON, dtype=np.uint64)
    blob = np.full((2, wB), POISON, dtype=np.uint64)
    key, elts = A._key(bytes(range(1, 33))), np.array([3, 2 * n - 1], dtype=np.uint64)
    assert L.crc_gen_evk(B.c, 7, pu(skB), dbc, pu(blob)) == PARAMETERS and L.crc_gen_evk_key(B.c, key, pu(skB), dbc, pu(blob)) == PARAMETERS
    assert L.crc_gen_galois_keys(B.c, 7, pu(skB), dbc, pu(elts), 2, pu(blob)) == PARAMETERS
    assert L.crc_gen_galois_keys_key(B.c, key, pu(skB), dbc, pu(elts), 2, pu(blob)) == PARAMETERS
    assert L.crc_gen_keys_seeded(B.c, 7, pu(skB), dbc, pu(ids), ids.size, pu(rows)) == PARAMETERS
    assert L.crc_gen_keys_seeded_key(B.c, key, seed, pu(skB), dbc, pu(ids), ids.size, pu(rows)) == PARAMETERS
    assert (rows == POISON).all() and (blob == POISON).all()
    # ... and the plain prefix context generates as it always did
    assert L.crc_gen_evk(C.c, 7, pu(skB), dbc, pu(blob)) == 0 and not (blob[0] == POISON).any()
    flat = out.reshape(-1)
    assert res() == 0 and np.array_equal(flat[:ids.size * wB].reshape(ids.size, wB), lk.restrict(keys, n, SMALL, 2, dbc)) and (flat[ids.size * wB:] == POISON).all()
    for e in (A, B, C, other, B2):
        e.close()


def test_the_level_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/level_keys_kernel_check.cpp: the bodies of ksk_restrict_kernel and both forms of ksk_expand_level_kernel (csrc/seeded_keys_device.h) on the CPU,
    one thread per workgroup over each launch's whole grid, with the address and undefined-behaviour sanitizers, equal the host twins bit for bit on buffers of
    exactly the documented sizes"""
    import tempfile
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "level_keys_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "level_keys_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    K4 = ca.default_coeff_modulus_128(8192)
    cases = [(64, 16, 2, SMALL), (64, 8, 2, SMALL), (64, 16, 1, SMALL), (64, 16, 1, SMALL[:2]), (64, 60, 2, SMALL), (64, 16, 3, K4), (4096, 16, 2, K4[:3]), (4096, 8, 1, K4[:3])]
    for n, dbc, kept, q in cases:
        out = subprocess.run([exe, str(n), str(dbc), str(kept)] + [str(v) for v in q], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, dbc, kept, q, out.stdout, out.stderr[-1500:])
