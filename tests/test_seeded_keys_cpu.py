"""Seeded key-switching keys on the host (crc_gen_keys_seeded[_key], crc_seeded_keys_expand, crc_seeded_keys_*; no GPU: host-only contexts).

A key set is ids (0: the evaluation key, else a Galois element), dbc, a PUBLIC 32-byte seed and the first rows [n_ids][P][k][n]; the second rows are
regenerated from the seed (ChaCha20 domain 9), the noise comes from the private key (domain 10), nonce = (id, p | dbc << 16 | k << 24, domain << 24 | s).  The
keystreams are recomputed here from crc_chacha20_block in Python integers; tests/test_gpu_seeded_keys.py pins the device to the host twin checked here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import crcnn_amd as ca
import galois_model as gm
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
KEY = bytes(range(1, 33))
PUB = bytes(range(101, 133))
DOM_A, DOM_E = 9, 10
PB = ctypes.POINTER(ctypes.c_uint8)
INVALID = -1


def key_ids(n):
    return [0, 1, 3, 2 * n - 1, pow(3, -1, 2 * n)]


def pairs_of(q, dbc):
    """[(l, factor)] in the blob's order: factor = (q / q_l) 2^(dbc d) mod q_l"""
    out = []
    for l, ql in enumerate(q):
        f = 1
        for j, qj in enumerate(q):
            if j != l:
                f = f * qj % ql
        for d in range(-(-int(ql).bit_length() // dbc)):
            out.append((l, f * pow(2, dbc * d, ql) % ql))
    return out


def block(E, key, counter, kid, p, dbc, k, dom, s):
    """the sixteen 32-bit words of one block of the stream (id, pair, even slot s)"""
    kb = (ctypes.c_uint8 * 32).from_buffer_copy(key)
    nonce = (ctypes.c_uint8 * 12).from_buffer_copy(int(kid).to_bytes(4, "little") + (p | dbc << 16 | k << 24).to_bytes(4, "little")
                                                   + (dom << 24 | s).to_bytes(4, "little"))
    out = (ctypes.c_uint8 * 64)()
    assert E.L.crc_chacha20_block(ctypes.cast(kb, PB), counter, ctypes.cast(nonce, PB), ctypes.cast(out, PB)) == 0
    return bytes(out)


def mask_value(E, q, seed, kid, p, dbc, i, s):
    b = block(E, seed, i // 2, kid, p, dbc, len(q), DOM_A, s & ~1)
    off = 32 * (i & 1) + 16 * (s & 1)
    return int.from_bytes(b[off:off + 16], "little") % int(q[i])


def noise_row(E, key, kid, p, dbc, k, n, T):
    e = np.zeros(n, dtype=np.int64)
    for s in range(0, n, 2):
        b = block(E, key, 0, kid, p, dbc, k, DOM_E, s)
        w4 = int.from_bytes(b[16:20], "little")
        for x in range(2):
            m = int.from_bytes(b[8 * x:8 * x + 8], "little")
            mag = sum(1 for thr in T if m >= thr)
            e[s + x] = -mag if (w4 >> x) & 1 else mag
    return e


def target(E, sk, q, kid):
    """w [k][n] as Python integers: s^2 for id 0, s gathered through pi_g for an element"""
    if kid == 0:
        return [(sk[j].astype(object) ** 2) % int(q[j]) for j in range(len(q))]
    tab = E.galois_ntt_table(kid)
    return [sk[j][tab].astype(object) for j in range(len(q))]


def minus_e(E, O, sk, q, dbc, kid, p, first_p, second_p):
    """(first + second s - [j == l] factor w) of one pair, inverse-transformed by the oracle and centred: [k][n]"""
    l, factor = pairs_of(q, dbc)[p]
    w = target(E, sk, q, kid)
    out = np.zeros((len(q), E.n), dtype=np.int64)
    for j, qj in enumerate(q):
        qj = int(qj)
        v = first_p[j].astype(object) + second_p[j].astype(object) * sk[j].astype(object)
        if j == l:
            v = v - factor * w[j]
        c = O.ntt_inv(j, (v % qj).astype(np.uint64)).astype(object)
        out[j] = np.where(c > qj // 2, c - qj, c).astype(np.int64)
    return out


def stream_sets():
    d8, d16 = ca.default_coeff_modulus_128(8192), ca.default_coeff_modulus_128(16384)
    return [(256, Q2, 16, None), (256, Q2, 8, None), (2048, Q1, 16, None), (8192, d8[:3], 16, None), (16384, d16[:5], 16, [3])]


@pytest.mark.parametrize("n,q,dbc,ids", stream_sets(), ids=["n256_k2_dbc16", "n256_k2_dbc8", "n2048_k1", "n8192_k3", "n16384_k5_one_id"])
def test_keystreams_are_what_the_header_says(n, q, dbc, ids):
    k = len(q)
    t = 65537
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    sk, _ = E.keygen(3)
    ids = key_ids(n) if ids is None else ids
    first, pub = E.gen_keys_seeded(0, sk, ids, dbc=dbc, key=KEY, public_seed=PUB)
    pairs = pairs_of(q, dbc)
    P = len(pairs)
    assert pub == PUB and first.shape == (len(ids), P * k * n) and E.seeded_key_words(dbc) == P * k * n == E.L.crc_evk_words(E.c, dbc) // 2
    blobs = E.seeded_keys_expand(first, ids, PUB, dbc=dbc).reshape(len(ids), P, 2, k, n)
    assert np.array_equal(blobs[:, :, 0].reshape(first.shape), first)               # the rows that travelled ARE the first polynomials
    T = E.encrypt_dev_noise_thresholds()
    rng = np.random.RandomState(n + dbc)
    # the mask: every position at n = 256, a seeded sample elsewhere (with the last modulus, whose block serves one modulus where k is odd, and the last pair)
    if n == 256:
        where = [(e, p, i, s) for e in range(len(ids)) for p in range(P) for i in range(k) for s in range(n)]
    else:
        where = [(rng.randint(len(ids)), rng.randint(P), rng.randint(k), rng.randint(n)) for _ in range(300)]
        where += [(len(ids) - 1, P - 1, k - 1, n - 1), (0, 0, 0, 0), (0, P - 1, k - 1, n - 2), (len(ids) - 1, 0, k - 1, 1)]
    if n == 256:
        memo = {}
        for e, p, i, s in where:
            key = (e, p, i // 2, s & ~1)
            if key not in memo:
                memo[key] = block(E, PUB, i // 2, ids[e], p, dbc, k, DOM_A, s & ~1)
            off = 32 * (i & 1) + 16 * (s & 1)
            assert int(blobs[e, p, 1, i, s]) == int.from_bytes(memo[key][off:off + 16], "little") % int(q[i]), (e, p, i, s)
    else:
        for e, p, i, s in where:
            assert int(blobs[e, p, 1, i, s]) == mask_value(E, q, PUB, ids[e], p, dbc, i, s), (e, p, i, s)
    # the noise: exact, the same integer under every modulus.  Every (id, pair) at n = 256, a sample of pairs elsewhere
    if n == 256:
        rows = [(e, p) for e in range(len(ids)) for p in range(P)]
    else:
        rows = sorted({(rng.randint(len(ids)), rng.randint(P)) for _ in range(2)} | {(len(ids) - 1, P - 1)})
    for e, p in rows:
        me = minus_e(E, O, sk, q, dbc, ids[e], p, blobs[e, p, 0], blobs[e, p, 1])
        want = noise_row(E, KEY, ids[e], p, dbc, k, n, T)
        for j in range(k):
            assert np.array_equal(me[j], -want), (e, p, j)
        assert abs(want).max() <= 19 and want.any()
    E.close()


def test_seed_form_is_the_key_form_of_its_two_expansions():
    n = 256
    E = ca.Engine(n, Q2, 65537, device=-1)
    sk, _ = E.keygen(3)
    seed = 77
    a, pub = E.gen_keys_seeded(seed, sk, key_ids(n))
    assert pub == E.seeded_public_seed(seed)
    private = E.seeded_public_seed(~seed & 0xffffffffffffffff)                     # the expansion of ~~seed = seed
    b, _ = E.gen_keys_seeded(0, sk, key_ids(n), key=private, public_seed=pub)
    assert np.array_equal(a, b)
    E.close()


def test_expanded_keys_rotate_and_relinearise():
    """the chain of test_model_rotation_decrypts_to_rotated_slots under an expanded seeded set, and the id-0 blob through the oracle's relinearisation"""
    n, q = 256, Q2
    t = ca.Engine.slots_prime(n, 20)
    E = ca.Engine(n, q, t, device=-1); O = orc.Oracle(n, q, t)
    M = gm.GaloisModel(O)
    sk, pk = E.keygen(31)
    rng = np.random.RandomState(2)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(1, n)).astype(np.int64)
    ct = E.encrypt(pk, E.slots_compose(v, 1, n, n, 1), 77)[0]
    small = rng.randint(-300, 301, size=(1, n)).astype(np.int64)
    cs = E.encrypt(pk, E.slots_compose(small, 1, n, n, 1), 78)[0]
    for dbc in (16, 8):
        elts = [int(e) for e in E.galois_default_elts()]
        first, pub = E.gen_keys_seeded(32, sk, [0] + elts, dbc=dbc)
        blobs = E.seeded_keys_expand(first, [0] + elts, pub, dbc=dbc)
        gk = np.ascontiguousarray(blobs[1:])
        for g, want in ((gm.elt_rows(n, 1), gm.rotate_rows_slots(v, 1)), (gm.elt_rows(n, -1), gm.rotate_rows_slots(v, -1)),
                        (gm.elt_rows(n, 5), gm.rotate_rows_slots(v, 5)), (2 * n - 1, gm.rotate_columns_slots(v))):
            y = M.apply_planned(ct, g, elts, gk, dbc)
            assert E.noise_budget(sk, y) >= 1, (dbc, g)
            got = E.slots_decompose(E.decrypt(sk, y[None]), n, n, 1)
            assert np.array_equal(got.reshape(1, n), want), (dbc, g)
        r = O.relinearize(O.square(cs), np.ascontiguousarray(blobs[0]), dbc)
        assert E.noise_budget(sk, r) >= 1, dbc
        got = E.slots_decompose(E.decrypt(sk, r[None]), n, n, 1).reshape(1, n)
        assert np.array_equal(got, small * small), dbc
    E.close()


def test_who_depends_on_what():
    n, q, dbc = 256, ca.default_coeff_modulus_128(8192)[:3], 16
    k = len(q)
    E = ca.Engine(n, q, 65537, device=-1); O = orc.Oracle(n, q, 65537)
    sk, _ = E.keygen(5)
    ids = key_ids(n)
    first, _ = E.gen_keys_seeded(0, sk, ids, dbc=dbc, key=KEY, public_seed=PUB)
    # a key does not depend on its place or company in the set
    alone, _ = E.gen_keys_seeded(0, sk, [3], dbc=dbc, key=KEY, public_seed=PUB)
    other, _ = E.gen_keys_seeded(0, sk, [2 * n - 1, 0, 3], dbc=dbc, key=KEY, public_seed=PUB)
    assert np.array_equal(alone[0], first[2]) and np.array_equal(other[2], first[2]) and np.array_equal(other[1], first[0]) and np.array_equal(other[0], first[3])
    assert np.array_equal(E.seeded_keys_expand(alone, [3], PUB, dbc=dbc)[0], E.seeded_keys_expand(first, ids, PUB, dbc=dbc)[2])
    assert len({first[e].tobytes() for e in range(len(ids))}) == len(ids)

    def parts(X, sub, fr, seed, d, secret, qq):
        """(second rows, e) of pair 0 of the key `sub`"""
        kk = len(qq)
        b = X.seeded_keys_expand(fr, [sub], seed, dbc=d).reshape(-1, 2, kk, n)
        OO = O if kk == k else orc.Oracle(n, qq, 65537)
        return b[0, 1], -minus_e(X, OO, secret, qq, d, sub, 0, b[0, 0], b[0, 1])

    A, e = parts(E, 3, alone, PUB, dbc, sk, q)
    assert all(np.array_equal(e[j], e[0]) for j in range(k)) and abs(e).max() <= 19 and e.any()
    # another dbc: other second rows and another e (pair 0 has the same factor at every digit width -- the attack the nonce prevents)
    f8, _ = E.gen_keys_seeded(0, sk, [3], dbc=8, key=KEY, public_seed=PUB)
    A8, e8 = parts(E, 3, f8, PUB, 8, sk, q)
    assert pairs_of(q, 8)[0] == pairs_of(q, dbc)[0]
    assert float((A8 == A).mean()) < 1e-2 and not np.array_equal(e8, e) and float((e8 == e).mean()) < 0.3
    # the prefix context of k - 1 primes under the same keys: other rows under the kept primes
    B = E.level(k - 1)
    skB = np.ascontiguousarray(sk[:k - 1])
    fB, _ = B.gen_keys_seeded(0, skB, [3], dbc=dbc, key=KEY, public_seed=PUB)
    AB, eB = parts(B, 3, fB, PUB, dbc, skB, q[:k - 1])
    assert float((AB == A[:k - 1]).mean()) < 1e-2 and not np.array_equal(eB, e[:k - 1]) and float((eB == e[:k - 1]).mean()) < 0.3
    B.close()
    # another public seed changes the mask and not the noise; another private key the noise and not the mask
    pub2, key2 = bytes(range(2, 34)), bytes(range(50, 82))
    fs, _ = E.gen_keys_seeded(0, sk, [3], dbc=dbc, key=KEY, public_seed=pub2)
    As, es = parts(E, 3, fs, pub2, dbc, sk, q)
    assert float((As == A).mean()) < 1e-2 and np.array_equal(es, e)
    fk, _ = E.gen_keys_seeded(0, sk, [3], dbc=dbc, key=key2, public_seed=PUB)
    Ak, ek = parts(E, 3, fk, PUB, dbc, sk, q)
    assert np.array_equal(Ak, A) and not np.array_equal(ek, e) and float((ek == e).mean()) < 0.3
    # another id: both
    A1, e1 = parts(E, 2 * n - 1, first[3:4], PUB, dbc, sk, q)
    assert float((A1 == A).mean()) < 1e-2 and not np.array_equal(e1, e)
    E.close()


def test_conjugation_and_refusals():
    n, q, dbc = 256, Q2, 16
    E = ca.Engine(n, q, 65537, device=-1)
    sk, _ = E.keygen(9)
    ids = np.array(key_ids(n), dtype=np.uint64)
    first, pub = E.gen_keys_seeded(4, sk, ids, dbc=dbc)
    blobs = E.seeded_keys_expand(first, ids, pub, dbc=dbc)
    for d in (16, 8):
        f, p = E.gen_keys_seeded(4, sk, ids[2:], dbc=d)
        assert np.array_equal(E.seeded_keys_expand(f, ids[2:], p, dbc=d, conjugate=True),
                              E.galois_conjugate_keys(ids[2:], E.seeded_keys_expand(f, ids[2:], p, dbc=d), dbc=d))
    pu = ca.binding._pu
    w = E.seeded_key_words(dbc)
    POISON = np.uint64(0xabababababababab)
    out = np.full((ids.size, 2 * w), POISON, dtype=np.uint64)
    rows = np.full((ids.size, w), POISON, dtype=np.uint64)
    key, seed = E._key(KEY), E._key(pub)
    L = E.L

    def gen(c=E.c, ky=key, sd=seed, s=pu(sk), d=dbc, i=pu(ids), m=ids.size, f=pu(rows)):
        return L.crc_gen_keys_seeded_key(c, ky, sd, s, d, i, m, f)

    def gens(c=E.c, s=pu(sk), d=dbc, i=pu(ids), m=ids.size, f=pu(rows)):
        return L.crc_gen_keys_seeded(c, 7, s, d, i, m, f)

    def exp(c=E.c, f=pu(first), i=pu(ids), m=ids.size, d=dbc, sd=seed, conj=0, o=pu(out)):
        return L.crc_seeded_keys_expand(c, f, i, m, d, sd, conj, o)

    for bad in (0, 1):                                                              # no conjugated key
        b = np.array([3, bad], dtype=np.uint64)
        assert exp(i=pu(b), m=2, conj=1) == INVALID
    assert exp(conj=2) == INVALID and exp(conj=-1) == INVALID
    for bad in (2, 4, 2 * n - 2, 2 * n, 2 * n + 1, 1 << 40):                         # even and non-zero, or >= 2n
        b = np.array([3, bad], dtype=np.uint64)
        assert gen(i=pu(b), m=2) == INVALID and gens(i=pu(b), m=2) == INVALID and exp(i=pu(b), m=2) == INVALID, bad
    for d in (0, 61, -3):
        assert gen(d=d) == INVALID and gens(d=d) == INVALID and exp(d=d) == INVALID and E.seeded_key_words(d) == 0 and E.seeded_keys_bytes(2, d) == 0
    assert gen(sd=E._key(KEY)) == INVALID                                           # key == seed
    assert gen(c=None) == INVALID and gen(ky=None) == INVALID and gen(sd=None) == INVALID and gen(s=None) == INVALID and gen(i=None) == INVALID
    assert gen(f=None) == INVALID and gens(c=None) == INVALID and gens(s=None) == INVALID and gens(i=None) == INVALID and gens(f=None) == INVALID
    assert exp(c=None) == INVALID and exp(f=None) == INVALID and exp(i=None) == INVALID and exp(sd=None) == INVALID and exp(o=None) == INVALID
    assert gen(m=-1) == INVALID and exp(m=-1) == INVALID
    assert (out == POISON).all() and (rows == POISON).all()
    assert gen(m=0) == 0 and gens(m=0) == 0 and exp(m=0) == 0 and (out == POISON).all() and (rows == POISON).all()
    assert exp() == 0 and np.array_equal(out, blobs)
    E.close()


def test_container():
    n, q, dbc = 256, Q2, 8
    E = ca.Engine(n, q, 65537, device=-1)
    sk, _ = E.keygen(9)
    ids = np.array(key_ids(n), dtype=np.uint64)
    first, pub = E.gen_keys_seeded(4, sk, ids, dbc=dbc)
    blob = E.seeded_keys_save(first, ids, pub, dbc=dbc)
    P = len(pairs_of(q, dbc))
    HEADER = 88
    assert len(blob) == E.seeded_keys_bytes(ids.size, dbc) == HEADER + 8 * ids.size + 8 * ids.size * P * len(q) * n
    assert len(blob) - HEADER - 8 * ids.size == E.seeded_keys_expand(first, ids, pub, dbc=dbc).nbytes // 2     # half the blobs' bytes
    assert blob[:8] == b"CRCSKEY\0"
    f2, i2, d2, s2 = E.seeded_keys_load(blob)
    assert np.array_equal(f2, first) and np.array_equal(i2, ids) and d2 == dbc and s2 == pub
    assert E.seeded_keys_save(f2, i2, s2, dbc=d2) == blob
    empty = E.seeded_keys_save(np.zeros((0, E.seeded_key_words(dbc)), dtype=np.uint64), [], pub, dbc=dbc)
    assert len(empty) == HEADER and E.seeded_keys_load(empty)[0].shape[0] == 0
    # refusals: a status, never a partial write
    pu = ca.binding._pu
    POISON = np.uint64(0x5a5a5a5a5a5a5a5a)
    rows = np.full(first.shape, POISON, dtype=np.uint64); got_ids = np.full(ids.shape, POISON, dtype=np.uint64)
    sd = (ctypes.c_uint8 * 32)(*([0x5a] * 32)); cnt, dd = ctypes.c_int(-7), ctypes.c_int(-7)

    def load(b, cap=ids.size):
        raw = np.frombuffer(bytes(b), dtype=np.uint8)
        return E.L.crc_seeded_keys_load(E.c, raw.ctypes.data, raw.nbytes, pu(rows), pu(got_ids), cap, ctypes.byref(cnt), ctypes.byref(dd), sd)

    def flip(at):
        b = bytearray(blob); b[at] ^= 1
        return bytes(b)
    bad = {"magic": flip(3), "version": flip(8), "dbc 0": blob[:12] + (0).to_bytes(4, "little") + blob[16:], "dbc 61": blob[:12] + (61).to_bytes(4, "little") + blob[16:],
           "another dbc (length no longer matches)": blob[:12] + (16).to_bytes(4, "little") + blob[16:], "hash": flip(20), "count": flip(48),
           "an even id": blob[:HEADER + 8] + (4).to_bytes(8, "little") + blob[HEADER + 16:],
           "truncated": blob[:-8], "truncated header": blob[:40], "empty": b"", "too long": blob + bytes(8)}
    for what, b in bad.items():
        assert load(b) == INVALID, what
    assert load(blob, cap=ids.size - 1) == INVALID                                  # more keys than the caller has room for
    O = ca.Engine(n, Q2, 1 << 16, device=-1)                                        # another plain modulus: another parameter hash
    raw = np.frombuffer(blob, dtype=np.uint8)
    assert O.L.crc_seeded_keys_load(O.c, raw.ctypes.data, raw.nbytes, pu(rows), pu(got_ids), ids.size, ctypes.byref(cnt), ctypes.byref(dd), sd) == INVALID
    O.close()
    assert (rows == POISON).all() and (got_ids == POISON).all() and bytes(sd) == b"\x5a" * 32 and cnt.value == -7 and dd.value == -7
    buf = np.full(len(blob), 0x5a, dtype=np.uint8); wr = ctypes.c_size_t(0)
    save = lambda cap: E.L.crc_seeded_keys_save(E.c, pu(first), pu(ids), ids.size, dbc, E._key(pub), buf.ctypes.data, cap, ctypes.byref(wr))
    assert save(len(blob) - 1) == INVALID and wr.value == len(blob) and (buf == 0x5a).all()       # a short capacity: the size it needs, nothing written
    assert save(len(blob)) == 0 and buf.tobytes() == blob
    assert load(blob) == 0 and np.array_equal(rows, first) and cnt.value == ids.size and dd.value == dbc
    E.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/seeded_keys_kernel_check.cpp: the bodies of the four kernels (csrc/seeded_keys_device.h) on the CPU, one thread per workgroup over each launch's
    whole grid, with the address and undefined-behaviour sanitizers, equal the host twins bit for bit on buffers of exactly the documented sizes: the ids 0, 1, 3
    and 2n - 1 generated and expanded, 3 and 2n - 1 conjugated, at n = 64 and 4096 with one, two and three moduli"""
    import tempfile
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "seeded_keys_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "seeded_keys_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    K3 = ca.default_coeff_modulus_128(8192)[:3]
    small = [0xffffe80001, 0xffffc40001, 0xffffffffffc0001]                          # two 40-bit primes and a 60-bit one: the generic Barrett path
    cases = [(64, 16, Q1), (64, 8, Q2), (64, 16, K3), (64, 16, small), (64, 60, Q2), (4096, 16, Q1), (4096, 16, Q2), (4096, 8, K3)]
    for n, dbc, q in cases:
        out = subprocess.run([exe, str(n), str(dbc)] + [str(v) for v in q], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, dbc, q, out.stdout, out.stderr[-1500:])
