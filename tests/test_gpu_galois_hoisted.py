"""Hoisted rotations on the GPU: galois_permute_ntt_kernel against NTT . sigma_g . INTT, the device key conjugation against the host's,
crc_rotate_hoisted_forms against the integer model of H_g (tests/galois_hoisted_model.py) bit for bit on both key-switch paths, crc_diag_mac_forms against its
composed form, rotations and the diagonal matrix-vector product through encryption and decryption, and the refusals."""
import numpy as np
import pytest

import galois_hoisted_model as hm
import galois_model as gm
from test_gpu_galois import Q1, Q2, gal_sets, moduli, residues

pytestmark = pytest.mark.gpu
COUNT = 5
FF = 0xffffffffffffffff


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [64, 256, 4096, 16384])
def test_permute_ntt_kernel_equals_the_definition(n, k):
    """the reference is the definition run with the engine's own transforms: inverse transform, sigma_g on coefficients (numpy), forward transform"""
    import crcnn_amd as ca
    q = moduli(n, k)
    E = ca.Engine(n, q, 1 << 20, device=0)
    rows = 3
    x = residues(q, rows, n, 5 * n + k)[:, 0]                        # [rows][k][n]
    d_x = E.upload(x)
    d_c = E.upload(x); E.ntt_inv(d_c, rows, size=1)
    coeff = E.download(d_c, x.shape)
    d_o = E.alloc(x.nbytes + 64)
    for g in (3, pow(3, -1, 2 * n), 2 * n - 1, n + 1, 27 * (2 * n - 1) % (2 * n), 1):
        d_w = E.upload(gm.sigma_rows_np(coeff, g, q)); E.ntt_fwd(d_w, rows, size=1)
        want = E.download(d_w, x.shape)
        E.L.crc_memset(E.c, d_o.ptr, 0xff, d_o.nbytes, E.stream)
        E.galois_permute_ntt_dev(d_x, rows, g, d_o)
        got = E.download(d_o, (x.size + 8,))
        assert np.array_equal(got[:-8].reshape(x.shape), want), (n, k, g)
        assert (got[-8:] == np.uint64(FF)).all(), (n, k, g, "wrote past the end")
        assert np.array_equal(want, x[..., E.galois_ntt_table(g)]), (n, k, g)          # the host table is the same gather
    assert np.array_equal(E.download(d_x, x.shape), x)
    E.close()


def test_device_conjugation_equals_the_host():
    import crcnn_amd as ca
    n, q = 256, Q2
    E = ca.Engine(n, q, 1 << 20, device=0)
    sk, _ = E.keygen(3)
    for dbc in (16, 8):
        elts, gk = E.gen_galois_keys(4, sk, dbc=dbc)
        d_gk = E.upload(gk); d_cg = E.alloc(gk.nbytes)
        E.galois_conjugate_keys_dev(elts, d_gk, d_cg, dbc=dbc)
        assert np.array_equal(E.download(d_cg, gk.shape), E.galois_conjugate_keys(elts, gk, dbc=dbc)), dbc
    E.close()


_MODEL = {}


def model_case(si, dbc):
    """engine-side conjugated keys, inputs and the model's H_g for one (parameter set, dbc): computed once, shared"""
    if (si, dbc) in _MODEL:
        return _MODEL[(si, dbc)]
    import crcnn_amd as ca
    from oracle import orc
    n, q, t = gal_sets()[si]
    H = ca.Engine(n, q, t, device=-1)
    M = gm.GaloisModel(orc.Oracle(n, q, t))
    sk, pk = H.keygen(51 + si)
    lists = [[3, 1, 2 * n - 1], [1, 3, 1, 2 * n - 1, 3]]              # the second: copies first and between, three keyed results, one key in two slots
    elts, gk = H.gen_galois_keys(52 + si, sk, dbc=dbc, elts=[2 * n - 1, 3])
    cg = H.galois_conjugate_keys(elts, gk, dbc=dbc)
    elts = [int(e) for e in elts]
    rng = np.random.RandomState(10 + si)
    x = H.encrypt(pk, (rng.randint(0, 1 << 30, size=(COUNT, n)).astype(np.uint64) % np.uint64(t)), 600)
    of = {}
    for g in lists[0]:
        kc = hm.conjugate_key_coeff(M, M.key_coeff(gk[elts.index(g)], dbc), g) if g != 1 else None       # (the model conjugates by the definition)
        of[g] = np.stack([hm.hoisted(M, x[i], g, None, dbc, key_coeff=kc) for i in range(COUNT)])
    H.close()
    _MODEL[(si, dbc)] = (n, q, t, elts, cg, x, [(gs, np.stack([of[g] for g in gs])) for gs in lists])
    return _MODEL[(si, dbc)]


@pytest.mark.parametrize("dbc", [16, 8])
@pytest.mark.parametrize("si", [0, 1], ids=["n256_k2", "n2048_k1"])
def test_rotate_hoisted_equals_the_model(si, dbc):
    """R = 3 with g = 1 and 2n - 1 among them, and R = 5 with an odd number of keyed elements (a pair and a single one at hoist_rt = 2), copies in front of and
    between them and one key in two slots; count = 5 in passes of 2 (a tail pass; the keys prepared by pass 0 serve the others), every form pair, both
    key-switch paths and both settings of the tuning key hoist_rt; then the same call in one pass"""
    import crcnn_amd as ca
    n, q, t, elts, cg, x, cases = model_case(si, dbc)
    E = ca.Engine(n, q, t, device=0)
    d_cg = E.upload(cg)
    for gs, want in cases:
        rotate_hoisted_case(E, dbc, elts, d_cg, x, gs, want)
    E.close()


def rotate_hoisted_case(E, dbc, elts, d_cg, x, gs, want):
    import crcnn_amd as ca
    d_y = E.alloc(want.nbytes)
    d_work = E.alloc(E.rotate_hoisted_work_bytes(COUNT, len(gs), dbc))
    try:
        for chunk in (2, 0):
            E.set_tuning("sq_chunk", chunk)
            assert E.rotate_hoisted_work_bytes(COUNT, len(gs), dbc) <= d_work.nbytes
            for path, rt in ((0, 1), (0, 2), (1, 0)):                    # the fp64 key switch with one and with two keys per digit load; the other path
                E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt)
                for fin in (ca.COEFF, ca.NTT):
                    d_in = E.upload(x)
                    if fin == ca.NTT:
                        E.ntt_fwd(d_in, COUNT)
                    for fout in (ca.COEFF, ca.NTT) if chunk else (ca.COEFF,):
                        E.L.crc_memset(E.c, d_y.ptr, 0xff, want.nbytes, E.stream)
                        E.rotate_hoisted(d_in, COUNT, gs, d_cg, elts, d_y, d_work, dbc=dbc, in_form=fin, out_form=fout)
                        if fout == ca.NTT:
                            E.ntt_inv(d_y, len(gs) * COUNT)
                        got = E.download(d_y, want.shape)
                        for r, g in enumerate(gs):
                            assert np.array_equal(got[r], want[r]), (chunk, path, rt, fin, fout, g)
                    if fin == ca.COEFF:
                        assert np.array_equal(E.download(d_in, x.shape), x)             # the input is only read
    finally:
        E.set_tuning("relin_path", 0); E.set_tuning("sq_chunk", 0); E.set_tuning("hoist_rt", 0)


def big_case(R, n=4096, k=2, count=2, t=65537, seed=0, steps=None):
    import crcnn_amd as ca
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(61 + seed)
    steps = list(range(R)) if steps is None else list(steps)          # step 0 is g = 1
    gs = [gm.elt_rows(n, s) for s in steps]
    elts, gk = H.gen_galois_keys(62 + seed, sk, elts=list(dict.fromkeys(g for g in gs if g != 1)))        # (one key per distinct element)
    cg = H.galois_conjugate_keys(elts, gk)
    rng = np.random.RandomState(R + seed)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(count, n)).astype(np.int64)
    x = H.encrypt(pk, H.slots_compose(v, count, n, n, 1), 700)
    return q, H, sk, pk, steps, gs, elts, gk, cg, v, x


def test_wave_kernels_equal_the_reference_path_at_n4096():
    """n = 4096, k = 2: the fp64 key switch runs its wave-local kernels here, with one key per digit load and with two (relin_mac_multi_f64_kernel); H_g is an
    exact function on Z_q, so its bits are the coefficient-modulus path's"""
    import crcnn_amd as ca
    n, k, count = 4096, 2, 3
    q, H, sk, pk, steps, gs, elts, gk, cg, v, x = big_case(4, count=count)                  # three keyed elements: a pair and a single one at hoist_rt = 2
    E = ca.Engine(n, q, 65537, device=0)
    d_cg = E.upload(cg); d_x = E.upload(x)
    d_y = E.alloc(len(gs) * x.nbytes); d_work = E.alloc(E.rotate_hoisted_work_bytes(count, len(gs)))
    out = {}
    try:
        for path, rt in ((1, 0), (0, 1), (0, 2)):
            E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt)
            E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
            E.rotate_hoisted(d_x, count, gs, d_cg, elts, d_y, d_work)
            out[(path, rt)] = E.download(d_y, (len(gs),) + x.shape)
    finally:
        E.set_tuning("relin_path", 0); E.set_tuning("hoist_rt", 0)
    assert np.array_equal(out[(0, 1)], out[(1, 0)]) and np.array_equal(out[(0, 2)], out[(1, 0)])
    assert np.array_equal(out[(1, 0)][0], x) and not np.array_equal(out[(1, 0)][1], x)
    E.close(); H.close()


@pytest.mark.parametrize("n,R,count,chunk,steps", [(4096, 5, 2, 0, None), (256, 34, 3, 8, None), (256, 4, 3, 2, [0, 1, 0, 2])],
                         ids=["n4096_R5", "n256_R34_two_groups_tail_pass", "n256_identity_twice_in_a_group_tail_pass"])
def test_diag_mac_equals_rotate_multiply_add(n, R, count, chunk, steps):
    """the fused product = crc_rotate_hoisted_forms, crc_multiply_plain_ntt per element, crc_add, bit for bit.  R = 34 needs two launches of the diagonal kernel
    (32 elements each at most, the second accumulating) and, with the pass shortened to 8 . 8 / 32 = 2 ciphertexts, a tail pass.  Steps [0, 1, 0, 2] hold the
    identity twice in one group (one transformed copy of a coefficient-form pass serves both), in passes of 2 with a tail"""
    import crcnn_amd as ca
    k = 2
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 20)
    q, H, sk, pk, steps, gs, elts, gk, cg, v, x = big_case(R, n=n, k=k, count=count, t=t, steps=steps)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(n + R)
    rows = rng.randint(0, t, size=(R, n)).astype(np.int64)
    rows[-1, : n // 2] = 0; rows[0, 5] = t - 1
    d_p = E.alloc(R * k * n * 8)
    E.plain_to_ntt(E.upload(H.slots_compose(rows, R, n, n, 1)), R, d_p)
    d_cg = E.upload(cg)
    ctb = 2 * k * n * 8
    d_rot = E.alloc(R * count * ctb); d_y = E.alloc(count * ctb + 64); d_ref = E.alloc(count * ctb)
    try:
        E.set_tuning("sq_chunk", chunk)
        d_work = E.alloc(max(E.rotate_hoisted_work_bytes(count, R), E.diag_mac_work_bytes(count, R)))
        for rt, fin, fout in ((1, ca.COEFF, ca.COEFF), (2, ca.NTT, ca.NTT), (2, ca.COEFF, ca.NTT), (1, ca.NTT, ca.COEFF)):
            d_x = E.upload(x)
            if fin == ca.NTT:
                E.ntt_fwd(d_x, count)
            E.rotate_hoisted(d_x, count, gs, d_cg, elts, d_rot, d_work, in_form=fin, out_form=ca.NTT)
            for r in range(R):
                E.multiply_plain_ntt(d_rot.ptr + r * count * ctb, d_p.ptr + r * k * n * 8, count, count)
                if r == 0:
                    E.copy_d2d(d_ref, d_rot, count * ctb)
                else:
                    E.add(d_ref, d_rot.ptr + r * count * ctb, count)
            if fout == ca.COEFF:
                E.ntt_inv(d_ref, count)
            E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
            E.set_tuning("hoist_rt", rt)                                 # (the composed form above ran at the default)
            E.diag_mac(d_x, count, gs, d_p, d_cg, elts, d_y, d_work, in_form=fin, out_form=fout)
            E.set_tuning("hoist_rt", 0)
            got = E.download(d_y, (count * ctb // 8 + 8,))
            assert np.array_equal(got[:-8], E.download(d_ref, (count * ctb // 8,))), (rt, fin, fout)
            assert (got[-8:] == np.uint64(FF)).all()
    finally:
        E.set_tuning("sq_chunk", 0); E.set_tuning("hoist_rt", 0)
    E.close(); H.close()


def test_hoisted_rotations_and_matvec_through_encryption():
    """(4096, 2 moduli, t = 65537): the slots of H_g are rotate_rows' slots, with a noise budget within one bit of crc_rotate_rows_forms' (the same noise law; a
    bit is the measure's granularity); the diagonal product of an 8 x 8 and a 5 x 8 matrix with a vector tiled with period 8 is W x mod t in every slot"""
    import crcnn_amd as ca
    n, k, t, count, M = 4096, 2, 65537, 2, 8
    q, H, sk, pk, steps, gs, elts, gk, cg, v, x = big_case(M, count=count, seed=1)
    half = t // 2
    E = ca.Engine(n, q, t, device=0)
    d_sk = E.upload(sk); d_cg = E.upload(cg); d_gk = E.upload(gk)
    ctb = 2 * k * n * 8
    d_pl = E.alloc(count * n * 8); d_o = E.alloc(count * n * 8); d_dw = E.alloc(E.decrypt_dev_work_bytes(count))

    def slots_of(d_ct, what, floor=1):
        y = E.download(d_ct, (count, 2, k, n))
        budgets = [H.noise_budget(sk, y[i]) for i in range(count)]
        print(what, "noise budget:", budgets)
        assert min(budgets) >= floor, (what, budgets)
        E.decrypt_dev(d_sk, d_ct, count, d_pl, d_dw)
        E.slots_decompose_dev(d_pl, count, n, d_o, n, 1)
        return E.download(d_o, (count, n), dtype=np.int64), budgets

    d_x = E.upload(x)
    d_rot = E.alloc(M * count * ctb); d_dir = E.alloc(count * ctb)
    d_work = E.alloc(max(E.rotate_hoisted_work_bytes(count, M), E.diag_mac_work_bytes(count, M), E.apply_galois_work_bytes(count)))
    E.rotate_hoisted(d_x, count, gs, d_cg, elts, d_rot, d_work)
    for r, s in enumerate(steps):
        got, hb = slots_of(d_rot.ptr + r * count * ctb, f"hoisted rotate_rows({s})")
        assert np.array_equal(got, gm.rotate_rows_slots(v, s)), s
        if s:
            E.rotate_rows(d_x, count, s, d_gk, elts, d_dir, d_work)
            got, db = slots_of(d_dir, f"direct rotate_rows({s})")
            assert np.array_equal(got, gm.rotate_rows_slots(v, s)), s
            assert all(h >= d - 1 for h, d in zip(hb, db)), (s, hb, db)
    # the matrix-vector product: the input tiled with period M, so a row rotation is a rotation mod M
    rng = np.random.RandomState(8)
    xs = rng.randint(0, t, size=(count, M)).astype(np.int64)
    d_xt = E.upload(H.encrypt(pk, H.slots_compose(np.tile(xs, (1, n // M)), count, n, n, 1), 701))
    d_y = E.alloc(count * ctb)
    for shape in ((8, 8), (5, 8)):
        W = rng.randint(0, t, size=shape).astype(np.int64)
        W[0, 0] = t - 1
        msteps, rows = E.diag_matvec_plan(W, M)
        assert msteps == list(range(M))
        d_p = E.alloc(len(msteps) * k * n * 8)
        E.plain_to_ntt(E.upload(H.slots_compose(rows, len(msteps), n, n, 1)), len(msteps), d_p)
        E.diag_mac(d_xt, count, [gm.elt_rows(n, s) for s in msteps], d_p, d_cg, elts, d_y, d_work)
        got, _ = slots_of(d_y, f"matvec {shape}")
        for c in range(count):
            want = hm.matvec(W, xs[c], t)
            want = [(w + half) % t - half for w in want + [0] * (M - len(want))] * (n // M)
            assert got[c].tolist() == want, (shape, c)
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
    R = 2
    d_x = E.alloc(2 * ctb); d_y = E.alloc(R * ctb + 64); d_cg = E.upload(cg); d_p = E.alloc(R * n * 8); d_o = E.alloc(3 * n * 8)
    d_work = E.alloc(max(E.rotate_hoisted_work_bytes(1, R), E.diag_mac_work_bytes(1, R)))
    E.L.crc_memset(E.c, d_x.ptr, 0, 2 * ctb, E.stream); E.L.crc_memset(E.c, d_p.ptr, 0, R * n * 8, E.stream)
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream); E.L.crc_memset(E.c, d_o.ptr, 0xff, 3 * n * 8, E.stream)
    pe = pu(elts); ne = len(elts)
    less = np.ascontiguousarray(elts[elts != 9]); pl = pu(less)
    G = lambda *g: pu(E._elts(list(g)))

    def rh(gs=G(3, 9), r=R, x=d_x.ptr, y=d_y.ptr, ck=d_cg.ptr, e=pe, m=ne, dbc=16, fi=0, fo=0, w=d_work.ptr, c=None):
        return E.L.crc_rotate_hoisted_forms(c or E.c, x, fi, 1, gs, r, ck, e, m, dbc, y, fo, w, None)

    def dm(gs=G(3, 9), r=R, x=d_x.ptr, y=d_y.ptr, p=d_p.ptr, ck=d_cg.ptr, e=pe, m=ne, dbc=16, fi=0, fo=0, w=d_work.ptr, c=None):
        return E.L.crc_diag_mac_forms(c or E.c, x, fi, 1, gs, r, p, ck, e, m, dbc, y, fo, w, None)
    for f in (rh, dm):
        assert f(e=pl, m=len(less)) == -1 and f(gs=G(3, 27)) == -1                  # a missing conjugated key: no chain of steps is planned
        assert f(r=0) == -1 and f(r=-1) == -1 and f(gs=None) == -1
        assert f(gs=G(3, 2)) == -1 and f(gs=G(2 * n + 1, 3)) == -1 and f(gs=G(0, 3)) == -1
        assert f(y=d_x.ptr) == -1 and f(y=d_x.ptr + ctb - 16) == -1                 # the output overlaps the input
        assert f(fi=ca.NTTP) == -1 and f(fo=ca.NTTL) == -1 and f(fi=ca.NTTLS) == -1
        assert f(dbc=0) == -1 and f(dbc=61) == -1
        assert f(x=d_x.ptr + 8) == -1 and f(y=d_y.ptr + 8) == -1 and f(ck=d_cg.ptr + 8) == -1 and f(x=None) == -1 and f(y=None) == -1 and f(w=None) == -1
        assert f(ck=None) == -1 and f(w=d_x.ptr) == -1 and f(w=d_y.ptr) == -1       # a work space inside an operand
        assert f(c=H.c) == -1                                                       # a host-only context
    assert rh(x=d_y.ptr + ctb) == -1                                                # the input inside the SECOND element's output
    assert dm(p=None) == -1 and dm(p=d_p.ptr + 8) == -1
    assert dm(p=d_y.ptr) == -1 and dm(p=d_y.ptr + ctb - 16) == -1 and dm(p=d_work.ptr) == -1     # the plaintext rows inside the output or the work space
    pn = lambda g, x=d_x.ptr, o=d_o.ptr, c=None: E.L.crc_galois_permute_ntt_dev(c or E.c, x, 3, g, o, None)
    assert pn(2) == -1 and pn(2 * n + 1) == -1 and pn(3, o=d_o.ptr + 8) == -1 and pn(3, o=None) == -1 and pn(3, x=d_o.ptr) == -1 and pn(3, c=H.c) == -1
    one = E._elts([1]); e3 = E._elts([3])
    cj = lambda e=pu(e3), m=1, dbc=16, i=d_cg.ptr, o=d_y.ptr, c=None: E.L.crc_galois_conjugate_keys_dev(c or E.c, e, m, dbc, i, o, None)
    assert cj(e=pu(one)) == -1 and cj(e=G(2)) == -1 and cj(dbc=0) == -1 and cj(o=d_cg.ptr) == -1 and cj(i=None) == -1 and cj(o=d_y.ptr + 8) == -1 and cj(c=H.c) == -1
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    assert (E.download(d_o, (3 * n,)) == np.uint64(FF)).all()
    # an empty batch is no error, and a call of only g = 1 needs no key set
    assert E.L.crc_rotate_hoisted_forms(E.c, d_x.ptr, 0, 0, G(3, 9), R, d_cg.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == 0
    assert E.L.crc_diag_mac_forms(E.c, d_x.ptr, 0, 0, G(3, 9), R, d_p.ptr, d_cg.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == 0
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    assert E.L.crc_rotate_hoisted_forms(E.c, d_x.ptr, 0, 1, G(1), 1, None, None, 0, 16, d_y.ptr, 0, d_work.ptr, None) == 0
    assert (E.download(d_y, (ctb // 8,)) == 0).all()
    E.close(); H.close()
