"""Galois automorphisms on the GPU: galois_permute_kernel against the definition, crc_apply_galois_forms against the integer model of Evaluator::apply_galois
(tests/galois_model.py) bit for bit, rotations and the slot sum against the slot statement through encryption and decryption, the fused accumulate against
crc_add, and the refusals."""
import os

import numpy as np
import pytest

import galois_model as gm

pytestmark = pytest.mark.gpu
Q1 = [0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
COUNT = 3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_n256_k2_t20.npz")


def moduli(n, k):
    import crcnn_amd as ca
    if k == 1:
        return Q1
    if k == 2:
        return Q2
    return ca.binding.default_coeff_modulus_128(8192)[:3]             # 1 mod 16384: transform primes of every smaller ring too


def residues(q, count, n, seed):
    """[count][2][k][n] canonical residues with 0 and q - 1 among them"""
    rng = np.random.RandomState(seed)
    x = np.zeros((count, 2, len(q), n), dtype=np.uint64)
    for i, qi in enumerate(q):
        x[:, :, i, :] = (rng.randint(0, 1 << 62, size=(count, 2, n)).astype(np.uint64) % np.uint64(qi))
        x[0, :, i, 0] = 0; x[0, :, i, 1] = qi - 1; x[-1, :, i, n - 1] = qi - 1; x[-1, :, i, n - 2] = 0; x[1, 0, i, :] = 0; x[1, 1, i, 5] = qi - 1
    return x


@pytest.mark.parametrize("n,k", [(64, 1), (256, 2), (2048, 3), (4096, 2), (8192, 3), (16384, 1)])
def test_permute_kernel_equals_the_definition(n, k):
    import crcnn_amd as ca
    q = moduli(n, k)
    E = ca.Engine(n, q, 1 << 20, device=0)
    x = residues(q, COUNT, n, 3 * n + k)
    qq = np.array(q, dtype=np.uint64).reshape(1, k, 1)
    inv = []                                                         # (q/q_i)^-1 mod q_i
    for i in range(k):
        h = 1
        for j in range(k):
            if j != i:
                h = h * q[j] % q[i]
        inv.append(pow(h, -1, q[i]) if k > 1 else 1)
    d_x = E.upload(x)
    d_o = E.alloc(COUNT * 3 * k * n * 8 + 64)
    for g in (3, pow(3, -1, 2 * n), 2 * n - 1, n + 1, 2 * n - 3):
        s0 = gm.sigma_rows_np(x[:, 0], g, q); s1 = gm.sigma_rows_np(x[:, 1], g, q)
        p2 = np.stack([np.array([int(v) * inv[i] % q[i] for v in s1[:, i].reshape(-1)], dtype=np.uint64).reshape(COUNT, n) for i in range(k)], axis=1)
        for acc in (False, True):
            want = np.zeros((COUNT, 3, k, n), dtype=np.uint64)
            if acc:
                s = s0 + x[:, 0]                                     # (below 2^56: no wrap)
                want[:, 0] = np.where(s >= qq, s - qq, s); want[:, 1] = x[:, 1]
            else:
                want[:, 0] = s0
            want[:, 2] = p2
            E.L.crc_memset(E.c, d_o.ptr, 0xff, d_o.nbytes, E.stream)
            E.galois_permute_dev(d_x, COUNT, g, d_o, accumulate=acc)
            got = E.download(d_o, (COUNT * 3 * k * n + 8,))
            assert np.array_equal(got[:-8].reshape(want.shape), want), (n, k, g, acc)
            assert (got[-8:] == np.uint64(0xffffffffffffffff)).all(), (n, k, g, acc, "wrote past the end")
    assert np.array_equal(E.download(d_x, x.shape), x)
    E.close()


def gal_sets():
    g = dict(np.load(GOLD))
    return [(int(g["n"]), [int(v) for v in g["q"]], int(g["t"])), (2048, Q1, 12289)]


_MODEL = {}


def model_case(si, dbc):
    """engine-side keys, inputs and the model's results for one (parameter set, dbc): computed once, shared"""
    if (si, dbc) in _MODEL:
        return _MODEL[(si, dbc)]
    import crcnn_amd as ca
    from oracle import orc
    n, q, t = gal_sets()[si]
    H = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    M = gm.GaloisModel(O)
    sk, pk = H.keygen(41 + si)
    elts, gk = H.gen_galois_keys(42 + si, sk, dbc=dbc)
    elts = [int(e) for e in elts]
    rng = np.random.RandomState(si)
    x = H.encrypt(pk, (rng.randint(0, 1 << 30, size=(COUNT, n)).astype(np.uint64) % np.uint64(t)), 500)
    two_step = gm.elt_rows(n, 3)                                     # 27 = 3 . 9: not in the default set
    assert len(gm.plan(n, two_step, elts)) == 2
    gs = [3, 2 * n - 1, two_step]
    kc = {}
    want = {}
    for g in gs:
        out = []
        for i in range(COUNT):
            ct = x[i]
            for s in gm.plan(n, g, elts):
                if s not in kc:
                    kc[s] = M.key_coeff(gk[s], dbc)
                ct = M.apply(ct, elts[s], None, dbc, key_coeff=kc[s])
            out.append(ct)
        want[g] = np.stack(out)
    H.close()
    _MODEL[(si, dbc)] = (n, q, t, sk, elts, gk, x, gs, want, M)
    return _MODEL[(si, dbc)]


@pytest.mark.parametrize("dbc", [16, 8])
@pytest.mark.parametrize("si", [0, 1], ids=["n256_k2", "n2048_k1"])
def test_apply_galois_equals_the_model(si, dbc):
    import crcnn_amd as ca
    n, q, t, sk, elts, gk, x, gs, want, M = model_case(si, dbc)
    E = ca.Engine(n, q, t, device=0)
    d_gk = E.upload(gk)
    d_y = E.alloc(x.nbytes)
    d_work = E.alloc(E.apply_galois_work_bytes(COUNT, dbc))
    try:
        for path in (0, 1):
            E.set_tuning("relin_path", path)
            for fin in (ca.COEFF, ca.NTT):
                d_in = E.upload(x)
                if fin == ca.NTT:
                    E.ntt_fwd(d_in, COUNT)
                for fout in (ca.COEFF, ca.NTT):
                    for g in gs:
                        E.L.crc_memset(E.c, d_y.ptr, 0xff, x.nbytes, E.stream)
                        E.apply_galois(d_in, COUNT, g, d_gk, elts, d_y, d_work, dbc=dbc, in_form=fin, out_form=fout)
                        if fout == ca.NTT:
                            E.ntt_inv(d_y, COUNT)
                        assert np.array_equal(E.download(d_y, x.shape), want[g]), (path, fin, fout, g)
    finally:
        E.set_tuning("relin_path", 0)
    # g = 1: the same ciphertext in the requested form, no key needed
    d_in = E.upload(x)
    E.apply_galois(d_in, COUNT, 1, None, [], d_y, d_work, dbc=dbc, out_form=ca.NTT)
    E.ntt_inv(d_y, COUNT)
    assert np.array_equal(E.download(d_y, x.shape), x)
    E.close()


def test_fused_accumulate_equals_add():
    """sum_slots' step y + rotate(y), formed inside the key switch, is crc_add(y, apply_galois(y)) bit for bit -- and so is the whole slot sum"""
    import crcnn_amd as ca
    n, q, t, sk, elts, gk, x, gs, want, M = model_case(0, 16)
    t = ca.Engine.slots_prime(n, 20)
    E = ca.Engine(n, q, t, device=0)
    assert E.slots_supported
    d_gk = E.upload(gk); d_x = E.upload(x)
    d_y = E.alloc(x.nbytes); d_r = E.alloc(x.nbytes); d_s = E.alloc(x.nbytes)
    d_work = E.alloc(max(E.apply_galois_work_bytes(COUNT), E.sum_slots_work_bytes(COUNT)))
    for fin, fout in ((ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT), (ca.COEFF, ca.NTT)):
        d_in = E.upload(x)
        if fin == ca.NTT:
            E.ntt_fwd(d_in, COUNT)
        E.L.crc_memset(E.c, d_s.ptr, 0xff, x.nbytes, E.stream)
        E.sum_slots(d_in, COUNT, d_gk, elts, d_s, d_work, in_form=fin, out_form=fout)
        if fout == ca.NTT:
            E.ntt_inv(d_s, COUNT)
        # the definition with separate rotations and adds
        E.copy_d2d(d_y, d_x, x.nbytes)
        logn = n.bit_length() - 1
        for j in range(logn):
            if j < logn - 1:
                E.rotate_rows(d_y, COUNT, 1 << j, d_gk, elts, d_r, d_work)
            else:
                E.rotate_columns(d_y, COUNT, d_gk, elts, d_r, d_work)
            E.add(d_y, d_r, COUNT)
        assert np.array_equal(E.download(d_s, x.shape), E.download(d_y, x.shape)), (fin, fout)
    E.close()


SLOT_SETS = [(4096, 2, 65537), (8192, 3, None)]


@pytest.mark.parametrize("n,k,t", SLOT_SETS, ids=["n4096_k2", "n8192_k3"])
def test_rotations_and_slot_sum_move_the_slots(n, k, t):
    """compose -> encrypt on the device -> rotate_rows -> rotate_columns -> decrypt -> decompose = the rolled and swapped integers; sum_slots = the sum mod t"""
    import crcnn_amd as ca
    q = moduli(n, k)
    t = t or ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(7)
    elts, gk = H.gen_galois_keys(8, sk)
    rng = np.random.RandomState(n)
    half = (t - 1) // 2
    v = rng.randint(-half, half + 1, size=(COUNT, n)).astype(np.int64)
    d_pl = E.alloc(COUNT * n * 8)
    E.slots_compose_dev(E.upload(v), COUNT, n, n, 1, d_pl)
    d_x = E.alloc(COUNT * 2 * k * n * 8); d_r = E.alloc(COUNT * 2 * k * n * 8); d_y = E.alloc(COUNT * 2 * k * n * 8)
    E.encrypt_dev_forms(E.upload(pk), d_pl, COUNT, 99, ca.COEFF, d_x, E.alloc(E.encrypt_dev_work_bytes(COUNT)))
    d_gk = E.upload(gk); d_sk = E.upload(sk)
    d_work = E.alloc(max(E.apply_galois_work_bytes(COUNT), E.sum_slots_work_bytes(COUNT)))
    d_dw = E.alloc(E.decrypt_dev_work_bytes(COUNT)); d_o = E.alloc(v.nbytes)

    def slots_of(d_ct, what):
        y = E.download(d_ct, (COUNT, 2, k, n))
        budgets = [H.noise_budget(sk, y[i]) for i in range(COUNT)]
        print(what, "noise budget:", budgets)
        assert min(budgets) >= 1, (what, budgets)
        E.decrypt_dev(d_sk, d_ct, COUNT, d_pl, d_dw)
        E.slots_decompose_dev(d_pl, COUNT, n, d_o, n, 1)
        return E.download(d_o, v.shape, dtype=np.int64)

    assert np.array_equal(slots_of(d_x, "fresh"), v)
    for s in (1, -1, 5, n // 2 - 1):
        E.rotate_rows(d_x, COUNT, s, d_gk, elts, d_r, d_work)
        assert np.array_equal(slots_of(d_r, f"rotate_rows({s})"), gm.rotate_rows_slots(v, s)), s
        E.rotate_columns(d_r, COUNT, d_gk, elts, d_y, d_work)
        assert np.array_equal(slots_of(d_y, f"rotate_rows({s}) + rotate_columns"), gm.rotate_columns_slots(gm.rotate_rows_slots(v, s))), s
    E.sum_slots(d_x, COUNT, d_gk, elts, d_y, d_work)
    tot = [(int(sum(int(a) for a in row)) % t + half) % t - half for row in v]
    want = np.array([[c] * n for c in tot], dtype=np.int64)
    assert np.array_equal(slots_of(d_y, "sum_slots"), want)
    E.close(); H.close()


def test_refusals_leave_the_output_untouched():
    import crcnn_amd as ca
    n, q, t = 2048, Q1, 12289
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(1)
    elts, gk = H.gen_galois_keys(2, sk)
    ctb = 2 * n * 8
    d_x = E.alloc(2 * ctb); d_y = E.alloc(2 * ctb + 64); d_gk = E.upload(gk); d_x3 = E.alloc(3 * n * 8)
    d_work = E.alloc(E.apply_galois_work_bytes(1))
    E.L.crc_memset(E.c, d_x.ptr, 0, 2 * ctb, E.stream); E.L.crc_memset(E.c, d_y.ptr, 0xff, 2 * ctb, E.stream); E.L.crc_memset(E.c, d_x3.ptr, 0xff, 3 * n * 8, E.stream)
    pe = ca.binding._pu(elts); ne = len(elts)
    less = np.ascontiguousarray(elts[elts != 3]); pl = ca.binding._pu(less)

    def ag(g=3, x=d_x.ptr, y=d_y.ptr, gkp=d_gk.ptr, e=pe, m=ne, dbc=16, fi=0, fo=0, w=d_work.ptr):
        return E.L.crc_apply_galois_forms(E.c, x, fi, 1, g, gkp, e, m, dbc, y, fo, w, None)

    def rr(steps, y=d_y.ptr):
        return E.L.crc_rotate_rows_forms(E.c, d_x.ptr, 0, 1, steps, d_gk.ptr, pe, ne, 16, y, 0, d_work.ptr, None)
    assert ag(g=2) == -1 and ag(g=2 * n) == -1 and ag(g=2 * n + 1) == -1 and ag(g=0) == -1
    assert rr(n // 2) == -1 and rr(-(n // 2)) == -1 and rr(1 << 30) == -1
    assert ag(y=d_x.ptr) == -1 and ag(y=d_x.ptr + ctb - 16) == -1                # overlapping output
    assert ag(e=pl, m=len(less)) == -1 and ag(g=27, e=pl, m=len(less)) == -1      # a missing key: directly, and as a step of a plan
    assert E.L.crc_sum_slots_forms(E.c, d_x.ptr, 0, 1, d_gk.ptr, pl, len(less), 16, d_y.ptr, 0, d_work.ptr, None) == -1
    assert ag(fi=ca.NTTP) == -1 and ag(fo=ca.NTTL) == -1 and ag(fi=ca.NTTLS) == -1
    assert ag(dbc=0) == -1 and ag(dbc=61) == -1
    assert ag(x=d_x.ptr + 8) == -1 and ag(y=d_y.ptr + 8) == -1 and ag(gkp=d_gk.ptr + 8) == -1 and ag(x=None) == -1 and ag(y=None) == -1 and ag(w=None) == -1
    assert ag(gkp=None) == -1 and ag(w=d_x.ptr) == -1 and ag(w=d_y.ptr) == -1             # a work space inside an operand
    pd = lambda g, x=d_x.ptr, o=d_x3.ptr: E.L.crc_galois_permute_dev(E.c, x, 1, g, 0, o, None)
    assert pd(2) == -1 and pd(2 * n + 1) == -1 and pd(3, o=d_x3.ptr + 8) == -1 and pd(3, o=None) == -1 and pd(3, x=d_x3.ptr) == -1
    assert (E.download(d_y, (2 * ctb // 8,)) == np.uint64(0xffffffffffffffff)).all()
    assert (E.download(d_x3, (3 * n,)) == np.uint64(0xffffffffffffffff)).all()
    # an empty batch is no error; a host-only context has no device entry points; rotations need slots
    assert E.L.crc_apply_galois_forms(E.c, d_x.ptr, 0, 0, 3, d_gk.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == 0
    assert E.L.crc_apply_galois_forms(H.c, d_x.ptr, 0, 1, 3, d_gk.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == -1
    assert E.L.crc_galois_permute_dev(H.c, d_x.ptr, 1, 3, 0, d_x3.ptr, None) == -1
    assert (E.download(d_y, (2 * ctb // 8,)) == np.uint64(0xffffffffffffffff)).all()
    P = ca.Engine(n, q, 1 << 20, device=0)                            # no prime t: apply_galois works, the slot operations do not
    assert P.L.crc_rotate_rows_forms(P.c, d_x.ptr, 0, 1, 1, d_gk.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == -2
    assert P.L.crc_rotate_columns_forms(P.c, d_x.ptr, 0, 1, d_gk.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == -2
    assert P.L.crc_sum_slots_forms(P.c, d_x.ptr, 0, 1, d_gk.ptr, pe, ne, 16, d_y.ptr, 0, d_work.ptr, None) == -2
    P.close(); E.close(); H.close()
