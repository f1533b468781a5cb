"""Seeded key-switching keys on the GPU: crc_gen_keys_seeded_dev[_key] and crc_seeded_keys_expand_dev against their host twins bit for bit, the expanded keys
through the rotations, the hoisted rotations and a relinearisation on the device, and the refusals."""
import numpy as np
import pytest

import galois_model as gm
from test_encrypt_sym_cpu import IDS, param_sets

pytestmark = pytest.mark.gpu
KEY = bytes(range(1, 33))
PUB = bytes(range(101, 133))
FF = np.uint64(0xffffffffffffffff)


def big_sets():
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(16384)
    return [(16384, q[:k], 1 << 20) for k in (4, 5, 8)]


def key_ids(n):
    return np.array([0, 1, 3, 2 * n - 1, pow(3, -1, 2 * n)], dtype=np.uint64)


def check_set(n, q, t, ids, dbcs, seed_form):
    """device rows == host rows (destination pre-filled with 0xff, a guard behind it, the secret key untouched), then both expansions == the host's"""
    import crcnn_amd as ca
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(n + len(q))
    d_sk = E.upload(sk)
    for dbc in dbcs:
        w = E.seeded_key_words(dbc)
        assert w * 2 == E.L.crc_evk_words(E.c, dbc)
        d_first = E.alloc(ids.size * w * 8 + 64)
        forms = ([dict()] if seed_form else []) + [dict(key=KEY, public_seed=PUB)]                # (the key form last: its rows are expanded below)
        for kw in forms:
            want, pub = H.gen_keys_seeded(77, sk, ids, dbc=dbc, **kw)
            E.L.crc_memset(E.c, d_first.ptr, 0xff, d_first.nbytes, E.stream)
            assert E.gen_keys_seeded_dev(77, d_sk, ids, d_first, dbc=dbc, **kw) == pub
            got = E.download(d_first, (ids.size * w + 8,))
            assert np.array_equal(got[:-8].reshape(want.shape), want), (n, len(q), dbc, kw.keys())
            assert (got[-8:] == FF).all(), "wrote past the rows"
        assert np.array_equal(E.download(d_sk, sk.shape), sk)
        # expansion of the rows just made (key form): every id plain, the elements other than 1 conjugated
        d_out = E.alloc(ids.size * 2 * w * 8 + 64)
        for conj, sel in ((False, np.arange(ids.size)), (True, np.flatnonzero(ids > 1))):
            rows = np.ascontiguousarray(want[sel]); sub = np.ascontiguousarray(ids[sel])
            blobs = H.seeded_keys_expand(rows, sub, PUB, dbc=dbc, conjugate=conj)
            E.L.crc_memset(E.c, d_out.ptr, 0xff, d_out.nbytes, E.stream)
            E.seeded_keys_expand_dev(E.upload(rows), sub, PUB, d_out, dbc=dbc, conjugate=conj)
            got = E.download(d_out, (ids.size * 2 * w + 8,))
            assert np.array_equal(got[:blobs.size].reshape(blobs.shape), blobs), (n, len(q), dbc, conj)
            assert (got[blobs.size:] == FF).all(), "wrote past the blobs"
    E.close(); H.close()


@pytest.mark.parametrize("si", range(6), ids=IDS)
def test_device_rows_and_expansion_equal_the_host_twin(si):
    n, q, t = param_sets()[si]
    check_set(n, q, t, key_ids(n), (16, 8), True)


@pytest.mark.parametrize("bi", range(3), ids=["n16384_k4", "n16384_k5", "n16384_k8"])
def test_device_rows_and_expansion_at_the_largest_ring(bi):
    n, q, t = big_sets()[bi]
    check_set(n, q, t, np.array([3, 2 * n - 1], dtype=np.uint64), (16, 8), False)


def test_the_default_set_fills_more_than_one_launch_of_workgroups():
    """22 elements at (4096, 2): 22 . 8 . 8 workgroups of 256 lanes, more than one per CU; and 40 ids at n = 1024, more than one launch carries by value"""
    import crcnn_amd as ca
    n, q, t = param_sets()[0]
    H = ca.Engine(n, q, t, device=-1)
    elts = H.galois_default_elts()
    assert elts.size == 22
    H.close()
    check_set(n, q, t, elts, (16,), False)
    many = np.array([0] + [2 * i + 1 for i in range(39)], dtype=np.uint64)          # two launches: 32 + 8 ids
    check_set(1024, param_sets()[3][1], 1 << 16, many, (16,), False)


@pytest.mark.parametrize("n,k", [(4096, 2), (8192, 3)], ids=["n4096_k2", "n8192_k3"])
def test_expanded_keys_rotate_and_relinearise_on_the_device(n, k):
    import crcnn_amd as ca
    from test_gpu_galois import moduli
    q = moduli(n, k)
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(7)
    d_sk = E.upload(sk)
    elts = H.galois_default_elts()
    ids = np.concatenate([np.array([0], dtype=np.uint64), elts])
    w = E.seeded_key_words()
    d_first = E.alloc(ids.size * w * 8)
    pub = E.gen_keys_seeded_dev(5, d_sk, ids, d_first, key=KEY, public_seed=PUB)
    d_keys = E.alloc(ids.size * 2 * w * 8)                                          # blob 0: the evaluation key; 1..: the Galois keys
    E.seeded_keys_expand_dev(d_first, ids, pub, d_keys)
    d_gk = d_keys.ptr + 2 * w * 8
    d_cg = E.alloc(elts.size * 2 * w * 8)
    E.seeded_keys_expand_dev(d_first.ptr + w * 8, elts, pub, d_cg, conjugate=True)

    cnt = 2
    rng = np.random.RandomState(n)
    half = (t - 1) // 2
    v = rng.randint(-half, half + 1, size=(cnt, n)).astype(np.int64)
    v[1] = rng.randint(-100, 101, size=n)                                           # (its square stays far below t / 2 at both plain moduli)
    d_pl = E.alloc(cnt * n * 8)
    E.slots_compose_dev(E.upload(v), cnt, n, n, 1, d_pl)
    ctb = cnt * 2 * k * n * 8
    d_x = E.alloc(ctb); d_y = E.alloc(ctb)
    E.encrypt_dev_forms(E.upload(pk), d_pl, cnt, 99, ca.COEFF, d_x, E.alloc(E.encrypt_dev_work_bytes(cnt)))
    gs = [E.galois_elt_rows(s) for s in (1, -1, 5)] + [E.galois_elt_columns()]
    d_work = E.alloc(max(E.apply_galois_work_bytes(cnt), E.rotate_hoisted_work_bytes(cnt, len(gs)), E.square_relin_work_bytes(cnt)))
    d_dw = E.alloc(E.decrypt_dev_work_bytes(cnt)); d_o = E.alloc(v.nbytes)

    def slots_of(ptr):
        E.decrypt_dev(d_sk, ptr, cnt, d_pl, d_dw)
        E.slots_decompose_dev(d_pl, cnt, n, d_o, n, 1)
        return E.download(d_o, v.shape, dtype=np.int64)

    want = [gm.rotate_rows_slots(v, s) for s in (1, -1, 5)] + [gm.rotate_columns_slots(v)]
    for s, wv in zip((1, -1, 5), want):
        E.rotate_rows(d_x, cnt, s, d_gk, elts, d_y, d_work)
        assert np.array_equal(slots_of(d_y), wv), s
    E.rotate_columns(d_x, cnt, d_gk, elts, d_y, d_work)
    assert np.array_equal(slots_of(d_y), want[3])
    assert gs[2] not in [int(e) for e in elts]                                       # (rotate_rows(5) was a plan of two keys)
    hs = [gs[0], gs[1], gs[3]]                                                       # the hoisted form takes elements that have a key
    d_rot = E.alloc(len(hs) * ctb)
    E.rotate_hoisted(d_x, cnt, hs, d_cg, elts, d_rot, d_work)
    for r, wv in enumerate((want[0], want[1], want[3])):
        assert np.array_equal(slots_of(d_rot.ptr + r * ctb), wv), r
    # id 0: the evaluation key
    d_y3 = E.alloc(cnt * 3 * k * n * 8)
    E.square(d_x, cnt, d_y3, d_work)
    E.relinearize(d_y3, cnt, d_keys, d_y, d_work)
    got = slots_of(d_y)
    sq = np.array([[(int(a) * int(a) % t + half) % t - half for a in row] for row in v], dtype=np.int64)
    assert np.array_equal(got, sq)
    y = E.download(d_y, (cnt, 2, k, n))
    assert min(H.noise_budget(sk, y[i]) for i in range(cnt)) >= 1
    E.close(); H.close()


def test_refusals_write_nothing():
    import crcnn_amd as ca
    n, q, t = param_sets()[0]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    L = E.L
    sk, _ = H.keygen(3)
    k = len(q)
    ids = key_ids(n); ni = ids.size
    w = E.seeded_key_words()
    rows, blob = ni * w * 8, ni * 2 * w * 8
    skb = k * n * 8
    # one buffer: [first rows][blobs][secret key]
    total = rows + blob + skb
    d = E.alloc(total)
    L.crc_memset(E.c, d.ptr, 0x5a, total, E.stream)
    E.sync()
    L.crc_memcpy_h2d(E.c, d.ptr + rows + blob, sk.ctypes.data, skb, E.stream)
    before = E.download(d, (total,), dtype=np.uint8)
    fp, op, sp = d.ptr, d.ptr + rows, d.ptr + rows + blob
    key, pub = E._key(KEY), E._key(PUB)
    pu = ca.binding._pu

    def gen(c=E.c, ky=key, sd=pub, s=sp, dbc=16, i=pu(ids), m=ni, f=fp):
        return L.crc_gen_keys_seeded_dev_key(c, ky, sd, s, dbc, i, m, f, E.stream)

    def gens(c=E.c, s=sp, dbc=16, i=pu(ids), m=ni, f=fp):
        return L.crc_gen_keys_seeded_dev(c, 7, s, dbc, i, m, f, E.stream)

    def exp(c=E.c, f=fp, i=pu(ids), m=ni, dbc=16, sd=pub, conj=0, o=op):
        return L.crc_seeded_keys_expand_dev(c, f, i, m, dbc, sd, conj, o, E.stream)

    assert gen(m=0) == 0 and gens(m=0) == 0 and exp(m=0) == 0                         # an empty set is no error
    assert gen(c=H.c) == -1 and gens(c=H.c) == -1 and exp(c=H.c) == -1 and gen(c=None) == -1 and exp(c=None) == -1
    assert gen(sd=E._key(KEY)) == -1                                                  # key == seed
    assert gen(ky=None) == -1 and gen(sd=None) == -1 and gen(s=None) == -1 and gen(i=None) == -1 and gen(f=None) == -1
    assert gens(s=None) == -1 and gens(i=None) == -1 and gens(f=None) == -1
    assert exp(f=None) == -1 and exp(i=None) == -1 and exp(sd=None) == -1 and exp(o=None) == -1
    assert gen(s=sp + 8) == -1 and gen(f=fp + 8) == -1 and exp(f=fp + 8) == -1 and exp(o=op + 8) == -1
    for dbc in (0, 61, -1):
        assert gen(dbc=dbc) == -1 and gens(dbc=dbc) == -1 and exp(dbc=dbc) == -1
    for bad in (2, 2 * n, 2 * n + 1, 1 << 40):
        b = np.array([3, bad], dtype=np.uint64)
        assert gen(i=pu(b), m=2) == -1 and gens(i=pu(b), m=2) == -1 and exp(i=pu(b), m=2) == -1
    for bad in (0, 1):                                                                # no conjugated key
        b = np.array([3, bad], dtype=np.uint64)
        assert exp(i=pu(b), m=2, conj=1) == -1
    assert exp(conj=2) == -1 and gen(m=-1) == -1 and exp(m=-1) == -1
    # overlaps: rows on the secret key, blobs on the rows (equal, by one pair from either side)
    assert gen(f=sp) == -1 and gen(f=sp + skb - 16) == -1 and gen(f=sp - rows + 16) == -1
    assert exp(o=fp) == -1 and exp(o=fp + rows - 16) == -1 and exp(f=op + blob - 16) == -1
    assert np.array_equal(E.download(d, (total,), dtype=np.uint8), before)
    # a grid over 2^31 - 1: the row transform's row count
    assert L.crc_gen_keys_seeded_dev_key(E.c, key, pub, sp, 1, pu(ids), 1 << 30, fp, E.stream) == -1
    assert np.array_equal(E.download(d, (total,), dtype=np.uint8), before)
    E.close(); H.close()


def test_host_classes_make_save_load_and_install_seeded_keys():
    """crcnn_amd/host/seeded_keys_host.cpp: generateGaloisKeysSeeded on the host threads and on the device give equal bytes under the deterministic seed; after
    save -> load -> installGaloisKeys, rotateRows, rotateRowsMany and a densePlanes layer decrypt to what they decrypt to under generateGaloisKeys (the keys
    differ, so the plaintexts are compared) -- and to the integers computed here"""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "seeded_keys_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds seeded_keys_host"
    n, M, t = 4096, 16, 65537
    q = param_sets()[0][1]
    half = (t - 1) // 2
    rng = np.random.RandomState(23)
    vec = np.zeros(M, dtype=np.int64)
    ins, outs = [0, 2, 4, 6, 8, 10], [0, 2, 4]
    vec[ins] = rng.randint(-200, 201, size=6)
    row = np.tile(vec, n // M)
    W = rng.randint(-50, 51, size=(3, 1, 6)).astype(np.int64)
    d = tempfile.mkdtemp()
    np.array([n, len(q), t] + [int(v) for v in q], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    row.tofile(os.path.join(d, "values.i64")); W.tofile(os.path.join(d, "w.i64"))
    out = subprocess.run([driver, d], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "seeded_keys_host ok" in out.stdout and "seeded host_device equal" in out.stdout
    # without the deterministic seed: an element made twice under one master key is one key under one public seed; new parameters give another
    assert "repeat seed equal element equal others differ" in out.stdout and "fresh seed differs element differs" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    same = {l[1]: l[2] for l in lines if l[0] == "plaintexts"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    sizes = [l for l in lines if l[0] == "bytes"][0]
    assert same == {"rows_1": "equal", "many_1": "equal", "many_5": "equal", "dense": "equal"}
    container, blobs = int(sizes[2]), int(sizes[4])
    elements, rest = divmod(blobs, 1 << 20)                                          # one blob at (4096, 2 moduli, dbc 16) is 1 MiB
    assert rest == 0 and elements >= 23 and container == 88 + 8 * elements + blobs // 2
    dense = np.zeros(M, dtype=np.int64)
    dense[outs] = [(int(W[o, 0] @ vec[ins]) + half) % t - half for o in range(3)]
    want = {"rows_1": gm.rotate_rows_slots(row[None], 1)[0], "many_1": gm.rotate_rows_slots(row[None], 1)[0], "many_5": gm.rotate_rows_slots(row[None], 5)[0],
            "dense": np.tile(dense, n // M)}
    for tag in ("ref", "seeded"):
        for name, w in want.items():
            assert budgets[f"{tag}_{name}"] >= 1, (tag, name, budgets)
            got = np.fromfile(os.path.join(d, f"{tag}_{name}.i64"), dtype=np.int64)
            assert np.array_equal(got, w), (tag, name)
    assert np.array_equal(np.fromfile(os.path.join(d, "seeded_after_refusals_rows_1.i64"), dtype=np.int64), want["rows_1"])
    assert throws == {"install_bad_dbc": "invalid_argument", "install_bad_element": "invalid_argument", "install_short_rows": "invalid_argument",
                      "load_truncated": "invalid_argument", "load_huge_count": "invalid_argument", "load_other_parameters": "invalid_argument",
                      "load_not_a_key_file": "invalid_argument", "generate_bad_dbc": "invalid_argument",
                      "generate_bad_element": "invalid_argument"}
