"""The baby-step / giant-step diagonal product on the GPU: crc_diag_mac_bsgs_forms against its composed form (crc_diag_mac_forms per giant index, crc_rotate_hoisted_forms
per giant index, crc_add) bit for bit, against crc_diag_mac_forms at G = 1, against the integer model (tests/bsgs_model.py), through encryption and decryption as a
matrix-vector product with the keys of bsgs_elements only, and the refusals."""
import numpy as np
import pytest

import bsgs_model as bm
import galois_hoisted_model as hm
import galois_model as gm
from test_gpu_galois import Q1, gal_sets, moduli

pytestmark = pytest.mark.gpu
FF = 0xffffffffffffffff


def keyed_case(n, k, t, count, gb, gg, seed):
    """host engine, keys for exactly the elements of gb and gg (conjugated), `count` encrypted slot vectors"""
    import crcnn_amd as ca
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(71 + seed)
    need = sorted({int(g) for g in list(gb) + list(gg)} - {1})
    elts, gk = H.gen_galois_keys(72 + seed, sk, elts=need)
    cg = H.galois_conjugate_keys(elts, gk)
    rng = np.random.RandomState(seed)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(count, n)).astype(np.int64)
    x = H.encrypt(pk, H.slots_compose(v, count, n, n, 1), 700 + seed)
    return q, H, sk, pk, elts, gk, cg, v, x


def shape_elements(n, B, G):
    """gb[b] = elt_rows(b) and gg[j] = elt_rows(B j) while that is a row rotation of this ring; beyond it any further valid elements do (the operation takes
    elements, not steps): other row rotations, the column swap and its products.  gb[0] = gg[0] = 1"""
    gb = [gm.elt_rows(n, b) for b in range(B)]
    gg = [gm.elt_rows(n, B * j) for j in range(G) if B * j < n // 2]
    more = [pow(3, s, 2 * n) for s in range(n // 2 - 1, 0, -1)] + [2 * n - 1, 3 * (2 * n - 1) % (2 * n), 9 * (2 * n - 1) % (2 * n)]
    gg += [g for g in more if g not in gg][:G - len(gg)]
    assert len(gb) == B and len(gg) == G and len(set(gg)) == G and all(gm.elt_valid(n, g) for g in gb + gg)
    return gb, gg


@pytest.mark.parametrize("n,k,B,G,count,chunk", [(4096, 2, 4, 5, 2, 0), (256, 2, 34, 5, 3, 8), (64, 1, 2, 34, 2, 0)],
                         ids=["n4096_B4_G5_tile_and_tail", "n256_B34_G5_two_baby_groups", "n64_B2_G34_one_workgroup_two_sum_groups"])
def test_fused_equals_composed(n, k, B, G, count, chunk):
    """the composed form: crc_diag_mac_forms(x, gb, P[j]) into NTT form for every j, crc_rotate_hoisted_forms(u_j, {gg[j]}) into NTT form, crc_add over j, one
    inverse transform for coefficient output -- built once per form pair at the default tuning; the fused call must give its bits on both key-switch paths,
    both settings of hoist_rt and both of bsgs_jt.  n = 4096: the wave-local key-switch kernels, a full tile of 4 inner sums and a tail of 1.  n = 256 with sq_chunk = 8: B = 34 is two
    launches of the multi kernel (32 + 2 baby elements, the second accumulating), and 32 + 5 kept ciphertexts shorten the pass to 8 . 8 / 37 = 1 ciphertext, so
    the keys prepared by pass 0 serve two more passes.  n = 64: both kernels' one-workgroup tail, nine tiles with a tail of 2, two launches of the sum kernel"""
    import crcnn_amd as ca
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 20)
    gb, gg = shape_elements(n, B, G)
    q, H, sk, pk, elts, gk, cg, v, x = keyed_case(n, k, t, count, gb, gg, n + B)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(n + G)
    rows = rng.randint(0, t, size=(G * B, n)).astype(np.int64)
    rows[B + 1] = 0; rows[0, 5] = t - 1                                # one all-zero row, one entry t - 1
    rowb = k * n * 8
    d_p = E.alloc(G * B * rowb)
    E.plain_to_ntt(E.upload(H.slots_compose(rows, G * B, n, n, 1)), G * B, d_p)
    d_cg = E.upload(cg)
    ctb = 2 * rowb
    d_u = E.alloc(G * count * ctb); d_r = E.alloc(G * count * ctb); d_ref = E.alloc(count * ctb); d_y = E.alloc(count * ctb + 64)
    try:
        E.set_tuning("sq_chunk", chunk)
        d_work = E.alloc(max(E.rotate_hoisted_work_bytes(count, 1), E.diag_mac_work_bytes(count, B), E.diag_mac_bsgs_work_bytes(count, B, G)))
        for fin in (ca.COEFF, ca.NTT):
            d_x = E.upload(x)
            if fin == ca.NTT:
                E.ntt_fwd(d_x, count)
            for fout in (ca.COEFF, ca.NTT):
                for j in range(G):
                    uj = d_u.ptr + j * count * ctb; rj = d_r.ptr + j * count * ctb
                    E.diag_mac(d_x, count, gb, d_p.ptr + j * B * rowb, d_cg, elts, uj, d_work, in_form=fin, out_form=ca.NTT)
                    E.rotate_hoisted(uj, count, [gg[j]], d_cg, elts, rj, d_work, in_form=ca.NTT, out_form=ca.NTT)
                    if j == 0:
                        E.copy_d2d(d_ref, rj, count * ctb)
                    else:
                        E.add(d_ref, rj, count)
                if fout == ca.COEFF:
                    E.ntt_inv(d_ref, count)
                want = E.download(d_ref, (count * ctb // 8,))
                for path, rt, jt in ((0, 1, 0), (0, 2, 2), (1, 0, 0), (0, 0, 1)):    # (bsgs_jt = 1: the inner sums by one launch per giant index)
                    E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt); E.set_tuning("bsgs_jt", jt)
                    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                    E.diag_mac_bsgs(d_x, count, gb, gg, d_p, d_cg, elts, d_y, d_work, in_form=fin, out_form=fout)
                    E.set_tuning("relin_path", 0); E.set_tuning("hoist_rt", 0); E.set_tuning("bsgs_jt", 0)
                    got = E.download(d_y, (count * ctb // 8 + 8,))
                    assert np.array_equal(got[:-8], want), (fin, fout, path, rt, jt)
                    assert (got[-8:] == np.uint64(FF)).all(), (fin, fout, path, rt, jt, "wrote past the end")
            if fin == ca.COEFF:
                assert np.array_equal(E.download(d_x, x.shape), x)     # the input is only read
    finally:
        E.set_tuning("sq_chunk", 0); E.set_tuning("relin_path", 0); E.set_tuning("hoist_rt", 0); E.set_tuning("bsgs_jt", 0)
    E.close(); H.close()


def test_one_giant_step_of_1_is_diag_mac():
    import crcnn_amd as ca
    n, k, t, count, B = 4096, 2, 65537, 2, 5
    gb, _ = shape_elements(n, B, 1)
    q, H, sk, pk, elts, gk, cg, v, x = keyed_case(n, k, t, count, gb, [1], 5)
    E = ca.Engine(n, q, t, device=0)
    rows = np.random.RandomState(9).randint(0, t, size=(B, n)).astype(np.int64)
    d_p = E.alloc(B * k * n * 8)
    E.plain_to_ntt(E.upload(H.slots_compose(rows, B, n, n, 1)), B, d_p)
    d_cg = E.upload(cg); d_x = E.upload(x)
    ctb = 2 * k * n * 8
    d_ref = E.alloc(count * ctb); d_y = E.alloc(count * ctb + 64)
    d_work = E.alloc(max(E.diag_mac_work_bytes(count, B), E.diag_mac_bsgs_work_bytes(count, B, 1)))
    for fout in (ca.COEFF, ca.NTT):
        E.diag_mac(d_x, count, gb, d_p, d_cg, elts, d_ref, d_work, out_form=fout)
        E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
        E.diag_mac_bsgs(d_x, count, gb, [1], d_p, d_cg, elts, d_y, d_work, out_form=fout)
        got = E.download(d_y, (count * ctb // 8 + 8,))
        assert np.array_equal(got[:-8], E.download(d_ref, (count * ctb // 8,))), fout
        assert (got[-8:] == np.uint64(FF)).all()
    E.close(); H.close()


COUNT = 5
_MODEL = {}


def model_case(si, dbc):
    """keys, inputs, plaintext rows and the model's result for one (parameter set, dbc): computed once"""
    if (si, dbc) in _MODEL:
        return _MODEL[(si, dbc)]
    import crcnn_amd as ca
    from oracle import orc
    n, q, t = gal_sets()[si]
    H = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    M = gm.GaloisModel(O)
    sk, pk = H.keygen(81 + si)
    gb, gg = [3, 1], [2 * n - 1, 1, 3]
    elts, gk = H.gen_galois_keys(82 + si, sk, dbc=dbc, elts=[2 * n - 1, 3])
    cg = H.galois_conjugate_keys(elts, gk, dbc=dbc)
    elts = [int(e) for e in elts]
    kc = {g: hm.conjugate_key_coeff(M, M.key_coeff(gk[elts.index(g)], dbc), g) for g in elts}
    rng = np.random.RandomState(20 + si)
    x = H.encrypt(pk, (rng.randint(0, 1 << 30, size=(COUNT, n)).astype(np.uint64) % np.uint64(t)), 800)
    plains = rng.randint(0, 1 << 30, size=(len(gg) * len(gb), n)).astype(np.uint64) % np.uint64(t)
    plains[3] = 0; plains[0, 7] = t - 1
    p_ntt = O.plains_to_ntt(plains).reshape(len(gg), len(gb), len(q), n)
    want = np.stack([bm.bsgs(M, x[i], gb, gg, p_ntt, kc, dbc) for i in range(COUNT)])
    H.close()
    _MODEL[(si, dbc)] = (n, q, t, elts, cg, x, gb, gg, plains, p_ntt, want)
    return _MODEL[(si, dbc)]


@pytest.mark.parametrize("dbc", [16, 8])
@pytest.mark.parametrize("si", [0, 1], ids=["n256_k2", "n2048_k1"])
def test_bsgs_equals_the_model(si, dbc):
    """B = 2, G = 3 with g = 1 in both lists, count = 5 in passes of 2 (sq_chunk = 2: 2 . 8 / (2 + 3) = 3, capped at the chunk), both key-switch paths"""
    import crcnn_amd as ca
    n, q, t, elts, cg, x, gb, gg, plains, p_ntt, want = model_case(si, dbc)
    E = ca.Engine(n, q, t, device=0)
    d_cg = E.upload(cg)
    d_p = E.alloc(p_ntt.nbytes)
    E.plain_to_ntt(E.upload(plains), plains.shape[0], d_p)
    assert np.array_equal(E.download(d_p, p_ntt.shape), p_ntt)
    d_y = E.alloc(want.nbytes)
    try:
        E.set_tuning("sq_chunk", 2)
        d_work = E.alloc(E.diag_mac_bsgs_work_bytes(COUNT, len(gb), len(gg), dbc))
        for path, rt in ((0, 1), (0, 2), (1, 0)):
            E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt)
            for fin, fout in ((ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT)):
                d_in = E.upload(x)
                if fin == ca.NTT:
                    E.ntt_fwd(d_in, COUNT)
                E.L.crc_memset(E.c, d_y.ptr, 0xff, want.nbytes, E.stream)
                E.diag_mac_bsgs(d_in, COUNT, gb, gg, d_p, d_cg, elts, d_y, d_work, dbc=dbc, in_form=fin, out_form=fout)
                if fout == ca.NTT:
                    E.ntt_inv(d_y, COUNT)
                assert np.array_equal(E.download(d_y, want.shape), want), (path, rt, fin, fout)
    finally:
        E.set_tuning("relin_path", 0); E.set_tuning("sq_chunk", 0); E.set_tuning("hoist_rt", 0)
    E.close()


def test_matvec_through_encryption():
    """(4096, 2 moduli, t = 65537), M = 16 split at B = 4: 16 x 16 and 11 x 16 matrices with the 6 keys of bsgs_elements(16, 4) where the flat method needs 15;
    every slot is W x mod t, the noise budget of every output is printed and at least 1 bit, and crc_diag_mac_forms with the full key set decrypts to the same
    slots.  The floor is a condition, not a measurement: the flat 8 x 8 product leaves 48 of a fresh ciphertext's 79 bits; this one sums 16 products, adds one
    additive key-switch term per giant step and sums 4 of them -- a few bits more"""
    import crcnn_amd as ca
    n, k, t, count, M, B = 4096, 2, 65537, 2, 16, 4
    half = t // 2
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    E = ca.Engine(n, q, t, device=0)
    sk, pk = H.keygen(91)
    few = ca.binding.bsgs_elements(M, B, n)
    assert len(few) == 6
    full = [gm.elt_rows(n, s) for s in range(1, M)]
    e_few, gk_few = H.gen_galois_keys(92, sk, elts=few)
    e_full, gk_full = H.gen_galois_keys(93, sk, elts=full)
    d_cf = E.upload(H.galois_conjugate_keys(e_few, gk_few)); d_cu = E.upload(H.galois_conjugate_keys(e_full, gk_full))
    d_sk = E.upload(sk)
    rng = np.random.RandomState(16)
    xs = rng.randint(0, t, size=(count, M)).astype(np.int64)
    d_x = E.upload(H.encrypt(pk, H.slots_compose(np.tile(xs, (1, n // M)), count, n, n, 1), 901))
    ctb = 2 * k * n * 8
    d_y = E.alloc(count * ctb); d_pl = E.alloc(count * n * 8); d_o = E.alloc(count * n * 8); d_dw = E.alloc(E.decrypt_dev_work_bytes(count))
    d_work = E.alloc(max(E.diag_mac_bsgs_work_bytes(count, B, M // B), E.diag_mac_work_bytes(count, M)))

    def slots_of(what):
        y = E.download(d_y, (count, 2, k, n))
        budgets = [H.noise_budget(sk, y[i]) for i in range(count)]
        print(what, "noise budget:", budgets)
        assert min(budgets) >= 1, (what, budgets)
        E.decrypt_dev(d_sk, d_y, count, d_pl, d_dw)
        E.slots_decompose_dev(d_pl, count, n, d_o, n, 1)
        return E.download(d_o, (count, n), dtype=np.int64)

    for shape in ((16, 16), (11, 16)):
        W = rng.randint(0, t, size=shape).astype(np.int64)
        W[0, 0] = t - 1
        baby, giant, rows = E.bsgs_matvec_plan(W, M, B)
        assert baby == list(range(B)) and giant == list(range(0, M, B))
        d_p = E.alloc(M * k * n * 8)
        E.plain_to_ntt(E.upload(H.slots_compose(rows.reshape(M, n), M, n, n, 1)), M, d_p)
        E.diag_mac_bsgs(d_x, count, [gm.elt_rows(n, b) for b in baby], [gm.elt_rows(n, s) for s in giant], d_p, d_cf, e_few, d_y, d_work)
        got = slots_of(f"bsgs matvec {shape}")
        steps, frows = E.diag_matvec_plan(W, M)
        E.plain_to_ntt(E.upload(H.slots_compose(frows, len(steps), n, n, 1)), len(steps), d_p)
        E.diag_mac(d_x, count, [gm.elt_rows(n, s) for s in steps], d_p, d_cu, e_full, d_y, d_work)
        flat = slots_of(f"flat matvec {shape}")
        for c in range(count):
            want = hm.matvec(W, xs[c], t)
            want = [(w + half) % t - half for w in want + [0] * (M - len(want))] * (n // M)
            assert got[c].tolist() == want, (shape, c)
            assert flat[c].tolist() == want, (shape, c)
    E.close(); H.close()


def test_refusals_leave_the_output_untouched():
    import crcnn_amd as ca
    n, q, t = 2048, Q1, 12289
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(1)
    elts, gk = H.gen_galois_keys(2, sk, elts=[3, 9, 2 * n - 1])
    cg = H.galois_conjugate_keys(elts, gk)
    pu = ca.binding._pu
    ctb = 2 * n * 8
    B = G = 2
    d_x = E.alloc(2 * ctb); d_y = E.alloc(ctb + 64); d_cg = E.upload(cg); d_p = E.alloc(G * B * n * 8 + 16)
    d_work = E.alloc(E.diag_mac_bsgs_work_bytes(1, B, G))
    E.L.crc_memset(E.c, d_x.ptr, 0, 2 * ctb, E.stream); E.L.crc_memset(E.c, d_p.ptr, 0, d_p.nbytes, E.stream)
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    pe = pu(elts); ne = len(elts)
    no9 = np.ascontiguousarray(elts[elts != 9]); no3 = np.ascontiguousarray(elts[elts != 3])
    A = lambda *g: pu(E._elts(list(g)))

    def f(gb=A(1, 3), b=B, gg=A(1, 9), g=G, x=d_x.ptr, y=d_y.ptr, p=d_p.ptr, ck=d_cg.ptr, e=pe, m=ne, dbc=16, fi=0, fo=0, w=d_work.ptr, c=None, cnt=1):
        return E.L.crc_diag_mac_bsgs_forms(c or E.c, x, fi, cnt, gb, b, gg, g, p, ck, e, m, dbc, y, fo, w, None)
    assert f(e=pu(no9), m=len(no9)) == -1 and f(gg=A(1, 27)) == -1                  # a missing giant key
    assert f(e=pu(no3), m=len(no3)) == -1 and f(gb=A(1, 27)) == -1                  # a missing baby key
    assert f(b=0) == -1 and f(g=0) == -1 and f(b=-1) == -1 and f(g=-1) == -1 and f(gb=None) == -1 and f(gg=None) == -1
    assert f(gb=A(1, 2)) == -1 and f(gg=A(2 * n + 1, 9)) == -1 and f(gg=A(0, 9)) == -1
    assert f(p=d_p.ptr + 8) == -1 and f(p=None) == -1                               # a misaligned or absent d_p_ntt
    assert f(w=d_y.ptr) == -1 and f(y=d_work.ptr + 4096) == -1                      # d_y overlapping d_work
    assert f(y=d_x.ptr) == -1 and f(w=d_x.ptr) == -1 and f(p=d_y.ptr) == -1 and f(p=d_work.ptr + 256) == -1
    assert f(x=d_x.ptr + 8) == -1 and f(y=d_y.ptr + 8) == -1 and f(ck=d_cg.ptr + 8) == -1 and f(x=None) == -1 and f(y=None) == -1 and f(w=None) == -1
    assert f(ck=None) == -1 and f(fi=ca.NTTP) == -1 and f(fo=ca.NTTL) == -1 and f(dbc=0) == -1 and f(dbc=61) == -1
    assert f(c=H.c) == -1                                                           # a host-only context
    assert f(cnt=0) == 0                                                            # an empty batch is no error
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    assert f() == 0                                                                 # ... and the call they all vary is a valid one
    assert (E.download(d_y, (ctb // 8,)) == 0).all()                                # (of a zero ciphertext)
    assert (E.download(d_y, (d_y.nbytes // 8,))[-8:] == np.uint64(FF)).all()
    E.close(); H.close()
