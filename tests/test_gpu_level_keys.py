"""Key-switching keys of a lower level derived from the upper level's, on the GPU: crc_keys_restrict_dev and crc_seeded_keys_expand_level_dev bit for bit against
their host twins (tests/test_level_keys_cpu.py checks those), and a computation that goes on at a derived level with keys generated ONLY at the top and
restricted on the device: square + relinearise, rotate_rows, rotate_hoisted and a dense_planes call with prepared keys, against tests/level_keys_model.py."""
import numpy as np
import pytest

import galois_model as gm
import level_keys_model as lk
from test_gpu_dense_planes import composed, plain_rows
from test_gpu_mod_switch import FILL, GUARD, SMALL, T, default_primes, sparse, sparse_negacyclic

pytestmark = pytest.mark.gpu
KSK_IDS_MAX = 32

CASES = [("n256_3to2", 256, SMALL, 2, (16, 8), (1, 33)), ("n256_3to1", 256, SMALL, 1, (16, 8), (1, 33)), ("n256_2to1", 256, SMALL[:2], 1, (16, 8), (1, 33)),
         ("n4096_3to2", 4096, 3, 2, (16, 8), (1, 33)), ("n16384_4to3", 16384, 4, 3, (16,), (1,))]


def guarded(E, words):
    """a device buffer of GUARD + words + GUARD words, all ones; the output starts behind the front guard (64 bytes in: still 16-byte aligned)"""
    buf = E.alloc((words + 2 * GUARD) * 8)
    E.L.crc_memset(E.c, buf.ptr, 0xff, (words + 2 * GUARD) * 8, E.stream)
    return buf, buf.ptr + GUARD * 8


def check_guarded(E, buf, words, want, what):
    got = E.download(buf, (words + 2 * GUARD,))
    assert np.array_equal(got[GUARD:GUARD + words], np.asarray(want).reshape(-1)), what
    assert (got[:GUARD] == np.uint64(FILL)).all() and (got[GUARD + words:] == np.uint64(FILL)).all(), what + ("guard words",)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_the_host_twins(case):
    """restriction of expanded blobs (plain and conjugated) and the seeded rows expanded straight into the level; 33 ids cross a launch boundary of KSK_IDS_MAX"""
    import crcnn_amd as ca
    _, n, q, kept, dbcs, counts = case
    q = default_primes(n, q) if isinstance(q, int) else q
    A = ca.Engine(n, q, T, device=0); B = A.derived_level(kept)
    assert A.keys_restrict_supported(B) and A.mod_switch_supported(B) and B.key_moduli == len(q)
    sk, _ = A.keygen(3)
    for dbc in dbcs:
        wA, wB = A.L.crc_evk_words(A.c, dbc), B.L.crc_evk_words(B.c, dbc)
        ids_all = [0] + [2 * i + 3 for i in range(max(counts))]                    # the evaluation key, then distinct elements 3, 5, ...
        first_all, pub = A.gen_keys_seeded(4, sk, ids_all, dbc=dbc)
        for cnt in counts:
            assert cnt == 1 or cnt > KSK_IDS_MAX
            for conj in (False, True):
                ids = ids_all[1:cnt + 1] if conj else ids_all[:cnt]
                first = first_all[1:cnt + 1] if conj else first_all[:cnt]
                what = (case[0], dbc, cnt, conj)
                blobs = A.seeded_keys_expand(first, ids, pub, dbc=dbc, conjugate=conj)
                want = A.keys_restrict(B, blobs, dbc=dbc)
                assert np.array_equal(want, lk.restrict(blobs, n, q, kept, dbc)), what
                assert np.array_equal(A.seeded_keys_expand_level(B, first, ids, pub, dbc=dbc, conjugate=conj), want), what
                d_blobs, d_first = A.upload(blobs), A.upload(first)
                buf, out = guarded(A, cnt * wB)
                A.keys_restrict_dev(B, d_blobs, cnt, out, dbc=dbc)
                check_guarded(A, buf, cnt * wB, want, what + ("restrict",))
                assert np.array_equal(A.download(d_blobs, blobs.shape), blobs), what + ("the input was written",)
                buf, out = guarded(A, cnt * wB)
                A.seeded_keys_expand_level_dev(B, d_first, ids, pub, out, dbc=dbc, conjugate=conj)
                check_guarded(A, buf, cnt * wB, want, what + ("level expand",))
                assert np.array_equal(A.download(d_first, first.shape), first), what + ("the rows were written",)
                for b in (d_blobs, d_first, buf):
                    b.free()
    A.close(); B.close()


def test_device_refusals_write_nothing():
    import crcnn_amd as ca
    n, dbc = 256, 16
    A = ca.Engine(n, SMALL, T, device=0); B = A.derived_level(2); C = A.level(2); H = ca.Engine(n, SMALL, T, device=-1)
    sk, _ = A.keygen(3)
    ids = np.array([3, 5], dtype=np.uint64)
    first, pub = A.gen_keys_seeded(4, sk, ids, dbc=dbc)
    blobs = A.seeded_keys_expand(first, ids, pub, dbc=dbc)
    wB = B.L.crc_evk_words(B.c, dbc)
    d_blobs, d_first = A.upload(blobs), A.upload(first)
    buf, out = guarded(A, 2 * wB)
    pu = ca.binding._pu
    seed = A._key(pub)
    res = lambda f, t, kk, m, d, o: A.L.crc_keys_restrict_dev(f, t, kk, m, d, o, None)
    exl = lambda f, t, fr, m, d, cj, o: A.L.crc_seeded_keys_expand_level_dev(f, t, fr, pu(ids), m, d, seed, cj, o, None)
    assert res(A.c, C.c, d_blobs.ptr, 2, dbc, out) == -1 and exl(A.c, C.c, d_first.ptr, 2, dbc, 0, out) == -1                 # a plain prefix context
    assert res(B.c, A.c, d_blobs.ptr, 2, dbc, out) == -1 and res(A.c, A.c, d_blobs.ptr, 2, dbc, out) == -1
    assert res(H.c, B.c, d_blobs.ptr, 2, dbc, out) == -1 and exl(H.c, B.c, d_first.ptr, 2, dbc, 0, out) == -1                 # a host-only context has no device entry points
    assert res(A.c, B.c, None, 2, dbc, out) == -1 and res(A.c, B.c, d_blobs.ptr, 2, dbc, None) == -1 and res(A.c, B.c, d_blobs.ptr, -1, dbc, out) == -1
    assert res(A.c, B.c, d_blobs.ptr, 2, 0, out) == -1 and res(A.c, B.c, d_blobs.ptr, 2, 61, out) == -1 and exl(A.c, B.c, d_first.ptr, 2, dbc, 2, out) == -1
    assert res(A.c, B.c, d_blobs.ptr, 2, dbc, out + 8) == -1 and exl(A.c, B.c, d_first.ptr, 2, dbc, 0, out + 8) == -1         # not 16-byte aligned
    assert res(A.c, B.c, d_blobs.ptr, 2, dbc, d_blobs.ptr) == -1 and res(A.c, B.c, d_blobs.ptr, 2, dbc, d_blobs.ptr + blobs.nbytes - 16) == -1      # overlap
    assert exl(A.c, B.c, d_first.ptr, 2, dbc, 0, d_first.ptr) == -1
    assert exl(A.c, B.c, d_first.ptr, 2, dbc, 1, out) == 0                                                                    # (3 and 5 have conjugated keys ...)
    A.L.crc_memset(A.c, buf.ptr, 0xff, buf.nbytes, A.stream)
    one = np.array([3, 1], dtype=np.uint64)
    assert A.L.crc_seeded_keys_expand_level_dev(A.c, B.c, d_first.ptr, pu(one), 2, dbc, seed, 1, out, None) == -1               # ... 1 has none
    assert res(A.c, B.c, d_blobs.ptr, 0, dbc, out) == 0 and exl(A.c, B.c, d_first.ptr, 0, dbc, 0, out) == 0
    # generation on the device at a derived level
    skB = np.ascontiguousarray(sk[:2]); d_sk = B.upload(skB)
    assert B.L.crc_gen_keys_seeded_dev(B.c, 7, d_sk.ptr, dbc, pu(ids), 2, out, None) == -2
    assert B.L.crc_gen_keys_seeded_dev_key(B.c, A._key(bytes(range(1, 33))), seed, d_sk.ptr, dbc, pu(ids), 2, out, None) == -2
    assert (A.download(buf, (2 * wB + 2 * GUARD,)) == np.uint64(FILL)).all() and np.array_equal(A.download(d_blobs, blobs.shape), blobs)
    # a derived level on the host only is as good a target: only its parameters are read
    HB = H.derived_level(2)
    A.keys_restrict_dev(HB, d_blobs, 2, out, dbc=dbc)
    check_guarded(A, buf, 2 * wB, H.keys_restrict(HB, blobs, dbc=dbc), ("host-only level",))
    for e in (A, B, C, H, HB):
        e.close()


def hoisted_model(OB, ct, g, ckey, pre, dbc):
    """H_g(ct) = sigma_g((c0, 0) + KeySwitch(c1; K'_g)) = sigma_g(apply_galois(sigma_{g^-1}(ct), g, K'_g))   (galois_hoisted_model.hoisted with the level's key switch)"""
    q = [int(v) for v in OB.q]
    h = pow(int(g), -1, 2 * OB.n)
    back = np.stack([gm.sigma_rows_np(ct[p], h, q) for p in range(2)])
    z = lk.apply_galois(OB, back, g, ckey, pre, dbc)
    return np.stack([gm.sigma_rows_np(z[p], g, q) for p in range(2)])


def test_a_computation_continues_at_the_derived_level():
    """test_a_computation_continues_at_the_lower_level (test_gpu_mod_switch.py) without the secret key at the level: evaluation and Galois keys are generated under
    three moduli only and restricted on the device; under two moduli square + relinearise, rotate_rows, rotate_hoisted (restricted CONJUGATED keys) run on both
    key-switch paths.  Every output is the model's key switch bit for bit, decrypts to the expected plaintext and keeps a budget.  The budget under a key generated
    afresh at the level is printed beside it; neither is compared with the other"""
    import crcnn_amd as ca
    from oracle import orc
    n, kept, dbc = 4096, 2, 16
    q = default_primes(n, 3)
    A = ca.Engine(n, q, T, device=0); B = A.derived_level(kept); C = A.level(kept)
    OB = orc.Oracle(n, q[:kept], T)
    sk, pk = A.keygen(5)
    skB = np.ascontiguousarray(sk[:kept])
    rng = np.random.RandomState(8)
    m1, m2, w = sparse(n, 8, rng, 1, T), sparse(n, 8, rng, 1, T), sparse(n, 4, rng, 1, 6)
    cts = A.encrypt(pk, np.stack([m1, m2]).astype(np.uint64), 9)
    d_a, d_b = A.upload(cts[0:1]), A.upload(cts[1:2])
    d_w = A.alloc(A.k * n * 8); A.plain_to_ntt(A.upload(w.astype(np.uint64)[None]), 1, d_w)
    A.multiply_plain(d_a, d_w, 1, 1); A.add(d_a, d_b, 1)
    expect1 = (sparse_negacyclic(m1, w, T) + m2) % T
    d_low = A.alloc(2 * kept * n * 8)
    A.mod_switch_dev(B, d_a, 1, d_low, A.alloc(A.mod_switch_work_bytes(B, 1)))
    A.sync()
    low = B.download(d_low, (1, 2, kept, n))
    assert np.array_equal(B.decrypt(skB, low)[0].astype(np.int64), expect1)
    # keys: made at the top, restricted on the device; nothing below reads sk except decryption and the budget
    g1, g2 = gm.elt_rows(n, 1), gm.elt_rows(n, 2)
    elts, gk = A.gen_galois_keys(14, sk, dbc=dbc, elts=[g1, g2])
    elts = [int(e) for e in elts]
    keys = np.concatenate([A.gen_evk(13, sk, dbc=dbc)[None], gk])
    d_keys = A.upload(keys)
    wA, wB = A.L.crc_evk_words(A.c, dbc), B.L.crc_evk_words(B.c, dbc)
    d_cg = A.alloc(2 * wA * 8); A.galois_conjugate_keys_dev(elts, d_keys.ptr + wA * 8, d_cg, dbc=dbc)
    d_kB, d_cgB = A.alloc(3 * wB * 8), A.alloc(2 * wB * 8)
    A.keys_restrict_dev(B, d_keys, 3, d_kB, dbc=dbc); A.keys_restrict_dev(B, d_cg, 2, d_cgB, dbc=dbc)
    A.sync()
    kB, cgB = B.download(d_kB, (3, wB)), B.download(d_cgB, (2, wB))
    assert np.array_equal(kB, lk.restrict(keys, n, q, kept, dbc)) and np.array_equal(cgB, B.galois_conjugate_keys(elts, kB[1:], dbc=dbc))
    pre = lk.prescale(q, kept)
    assert [int(v) for v in B.table("ksk_inv_qhat")] == pre
    # the model, once
    want_sq = lk.relinearize(OB, OB.square(low[0]), kB[0], pre, dbc)
    want_rot = lk.apply_galois(OB, want_sq, g1, kB[1], pre, dbc)
    want_h = hoisted_model(OB, want_rot, g2, cgB[1], pre, dbc)
    exp_sq = sparse_negacyclic(expect1, expect1, T)
    exp_rot = np.array(gm.sigma_row(exp_sq, g1, T), dtype=np.int64)
    exp_h = np.array(gm.sigma_row(exp_rot, g2, T), dtype=np.int64)
    for want, exp, name in ((want_sq, exp_sq, "square"), (want_rot, exp_rot, "rotate_rows"), (want_h, exp_h, "rotate_hoisted")):
        assert np.array_equal(B.decrypt(skB, want[None])[0].astype(np.int64), exp), name
        bits = B.noise_budget(skB, want)
        print(f"{name}: budget {bits} bits at the derived level")
        assert bits > 0, name
    # the same square under a key generated afresh at the level from the prefix secret-key rows: what the parent commit needs
    d_f = C.alloc(2 * kept * n * 8)
    C.square_relin(d_low, 1, C.upload(C.gen_evk(13, skB, dbc=dbc)), d_f, C.alloc(C.square_relin_work_bytes(1, dbc)), dbc=dbc)
    print(f"square: budget {C.noise_budget(skB, C.download(d_f, (2, kept, n)))} bits under a key generated at the level")
    d_y, d_z, d_h = (B.alloc(2 * kept * n * 8) for _ in range(3))
    d_sw, d_gw, d_hw = B.alloc(B.square_relin_work_bytes(1, dbc)), B.alloc(B.apply_galois_work_bytes(1, dbc)), B.alloc(B.rotate_hoisted_work_bytes(1, 1, dbc))
    d_evkB, d_gkB = d_kB.ptr, d_kB.ptr + wB * 8
    try:
        for path in (0, 1):
            B.set_tuning("relin_path", path)
            for d in (d_y, d_z, d_h):
                B.L.crc_memset(B.c, d.ptr, 0xff, 2 * kept * n * 8, B.stream)
            B.square_relin(d_low, 1, d_evkB, d_y, d_sw, dbc=dbc)
            B.rotate_rows(d_y, 1, 1, d_gkB, elts, d_z, d_gw, dbc=dbc)
            B.rotate_hoisted(d_z, 1, [g2], d_cgB, elts, d_h, d_hw, dbc=dbc)
            assert np.array_equal(B.download(d_y, (2, kept, n)), want_sq), (path, "square + relinearise")
            assert np.array_equal(B.download(d_z, (2, kept, n)), want_rot), (path, "rotate_rows")
            assert np.array_equal(B.download(d_h, (2, kept, n)), want_h), (path, "rotate_hoisted")
    finally:
        B.set_tuning("relin_path", 0)
    assert np.array_equal(B.download(d_low, low.shape), low)
    # a plain prefix context cuts digits with (q_B / q_l)^-1: the restricted keys are not its keys
    C.square_relin(d_low, 1, d_evkB, d_f, C.alloc(C.square_relin_work_bytes(1, dbc)), dbc=dbc)
    assert C.noise_budget(skB, C.download(d_f, (2, kept, n))) == 0
    for e in (A, B, C):
        e.close()


def test_prepared_restricted_keys_feed_dense_planes():
    """galois_prepare_keys on restricted conjugated keys, then one small dense_planes call at the level: the bits of its composition there (products, hoisted
    rotations, sums), and a result that still has a budget"""
    import crcnn_amd as ca
    n, kept, dbc, Cin, count = 4096, 2, 16, 2, 1
    q = default_primes(n, 3)
    A = ca.Engine(n, q, T, device=0); B = A.derived_level(kept)
    sk, pk = A.keygen(61)
    skB = np.ascontiguousarray(sk[:kept])
    gs = [gm.elt_rows(n, 1), 1, gm.elt_rows(n, 2)]
    elts, gk = A.gen_galois_keys(62, sk, dbc=dbc, elts=[gs[0], gs[2]])
    wA, wB = A.L.crc_evk_words(A.c, dbc), B.L.crc_evk_words(B.c, dbc)
    d_cg = A.alloc(2 * wA * 8); A.galois_conjugate_keys_dev(elts, A.upload(gk), d_cg, dbc=dbc)
    d_cgB = A.alloc(2 * wB * 8)
    A.keys_restrict_dev(B, d_cg, 2, d_cgB, dbc=dbc)
    rng = np.random.RandomState(5)
    v = rng.randint(-(T // 2), T // 2 + 1, size=(Cin * count, n)).astype(np.int64)
    d_x = A.upload(A.encrypt(pk, A.slots_compose(v, Cin * count, n, n, 1), 600))
    rowb = kept * n * 8; ctb = 2 * rowb
    d_xc = A.alloc(Cin * count * ctb)
    A.mod_switch_dev(B, d_x, Cin * count, d_xc, A.alloc(A.mod_switch_work_bytes(B, Cin * count)))
    A.sync()
    d_xn = B.alloc(Cin * count * ctb); B.copy_d2d(d_xn, d_xc, Cin * count * ctb); B.ntt_fwd(d_xn, Cin * count)
    R = len(gs)
    d_p = plain_rows(B, B, R, Cin, n, T, 7)
    d_pk = B.galois_prepare_keys(d_cgB, elts, dbc=dbc)
    d_tmp, d_u, d_r, d_ref = (B.alloc(count * ctb) for _ in range(4))
    d_work = B.alloc(max(B.rotate_hoisted_work_bytes(count, 1, dbc), B.dense_planes_work_bytes(count, Cin, R, dbc, prepared=True)))
    composed(B, d_xn, count, Cin, gs, d_p, d_cgB, elts, d_work, d_tmp, d_u, d_r, d_ref)
    B.ntt_inv(d_ref, count)
    want = B.download(d_ref, (count, 2, kept, n))
    buf, out = guarded(B, count * ctb // 8)
    B.dense_planes(d_xc, count, Cin, gs, d_p, d_cgB, elts, out, d_work, d_pk=d_pk, dbc=dbc)
    check_guarded(B, buf, count * ctb // 8, want, ("dense_planes with prepared restricted keys",))
    assert B.noise_budget(skB, want[0]) > 0
    A.close(); B.close()


def test_host_classes_continue_at_a_derived_level():
    """crcnn_amd/host/level_keys_host.cpp: encryptImageSlots -> modSwitch -> squareRelin -> rotateRows -> decryptSlots through makeLevel(kept, true), whose keys
    are the global ones restricted on the device"""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "level_keys_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds level_keys_host"
    n = 4096
    q = default_primes(n, 3)
    row = np.random.RandomState(31).randint(-100, 101, size=n).astype(np.int64)
    d = tempfile.mkdtemp()
    np.array([n, len(q), T] + [int(v) for v in q], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    row.tofile(os.path.join(d, "values.i64"))
    out = subprocess.run([driver, d], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "level_keys_host ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1:] for l in lines if l[0] == "level"] == [["key_moduli", "3", "k", "2", "derived", "1"], ["key_moduli", "2", "k", "2", "derived", "0"]]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    assert set(budgets) == {"switched", "square", "rotated", "rotated_ntt"} and min(budgets.values()) > 0, budgets
    assert throws == {"square_plain_level": "logic_error", "rotate_plain_level": "logic_error", "rotate_too_far": "invalid_argument",
                      "square_bad_form": "invalid_argument", "square_no_level": "invalid_argument", "rotate_key_not_present": "invalid_argument",
                      "stale_level_square": "invalid_argument"}
    got = {name: np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64) for name in budgets}
    want = {"switched": row, "square": row * row, "rotated": gm.rotate_rows_slots((row * row)[None], 1)[0]}
    want["rotated_ntt"] = want["rotated"]
    for name in want:
        assert np.array_equal(got[name], want[name]), name
