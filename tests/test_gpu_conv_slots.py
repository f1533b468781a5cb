"""The packed convolution over slots on the GPU: crc_conv_slots_forms against its composed definition (crc_diag_mac_forms per (output channel, input channel) with
constant plaintext rows, crc_add over input channels, one inverse transform) bit for bit at every tuning setting, worst-case operands at a 60-bit modulus against
Python integers, the identity, two planned layers through encryption against the integer convolution, and the refusals."""
import os

import numpy as np
import pytest

import conv_slots_model as cm
import galois_model as gm
from test_gpu_bsgs import keyed_case
from test_gpu_galois import Q1, moduli

pytestmark = pytest.mark.gpu
FF = 0xffffffffffffffff
JT = 8                                                                  # the largest instantiation of galois_conv_mac_kernel
JTS = (0, 2, 4, 8)                                                      # every setting of the tuning key conv_jt
GOLD60 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_n256_k1_q60_t30.npz")


def reset(E):
    for key in ("sq_chunk", "relin_path", "hoist_rt", "conv_jt"):
        E.set_tuning(key, 0)


@pytest.mark.parametrize("n,k,Cin,Cout,T,count,chunk,forms,tunings", [
    (4096, 2, 2, JT + 1, 3, 2, 0, 4, [(p, rt, jt) for p in (0, 1) for rt in (1, 2) for jt in JTS]),
    (256, 2, 3, 2, 34, 3, 8, 2, [(0, 1, 0), (0, 2, 8), (1, 0, 2), (0, 0, 4)]),
    (64, 1, 2, 2 * JT + 1, 3, 2, 0, 2, [(0, 0, jt) for jt in JTS])],
    ids=["n4096_tile_and_tail_every_setting", "n256_T34_two_tap_groups_passes_across_channels", "n64_one_workgroup_three_tiles"])
def test_fused_equals_composed(n, k, Cin, Cout, T, count, chunk, forms, tunings):
    """The composed definition: for every (co, ci) crc_diag_mac_forms(x[ci], gs, P[co][ci]) into NTT form with P[co][ci][tau] = crc_plain_to_ntt of the constant
    plaintext w mod t, crc_add over ci, one inverse transform for coefficient output -- built once per input form at the default tuning.  The fused call must give
    its bits.  n = 4096: the wave-local key-switch kernels, gs[1] = 1 between two keyed taps (a pair at hoist_rt = 2), a full tile and a tail of one at every
    conv_jt, both key-switch paths, all four form pairs.  n = 256 with sq_chunk = 8: T = 34 is two tap groups (32 + 2, the second accumulating) and 32 kept
    results shorten the pass to 8 . 8 / 32 = 2 of the 9 flat ciphertexts -- passes [0,2) [2,4) .. [8,9) end inside channels (count = 3) and span two of them;
    the keys prepared by pass 0 serve the four that follow.  n = 64: the one-workgroup tail of a row, 17 output channels"""
    import crcnn_amd as ca
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 20)
    gs = [gm.elt_rows(n, s) for s in range(T)]
    gs[0], gs[1] = gs[1], gs[0]                                         # the element 1 in the middle of the first pair
    assert gs[1] == 1 and len(set(gs)) == T
    q, H, sk, pk, elts, gk, cg, v, x = keyed_case(n, k, t, Cin * count, gs, [1], n + T)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(n + Cout)
    w = rng.randint(-(t // 2), t // 2 + 1, size=(Cout, Cin, T)).astype(np.int64)
    w[0, 0, 0] = t - 1; w[-1, -1, -1] = 0; w[0, 0, 1] = (t + 1) // 2
    wl = H.conv_slots_pack_weights(w)
    consts = np.zeros((Cout * Cin * T, n), dtype=np.uint64)
    consts[:, 0] = (w.reshape(-1) % t).astype(np.uint64)
    rowb = k * n * 8; ctb = 2 * rowb
    d_p = E.alloc(Cout * Cin * T * rowb)
    E.plain_to_ntt(E.upload(consts), Cout * Cin * T, d_p)
    rows = E.download(d_p, (Cout, Cin, T, k, n))
    assert (rows == wl.transpose(1, 2, 3, 0)[..., None]).all()          # d_w holds the word at every position of the constant's row
    d_w = E.upload(wl); d_cg = E.upload(cg)
    outw = Cout * count * ctb // 8
    d_tmp = E.alloc(count * ctb); d_ref = E.alloc(Cout * count * ctb); d_y = E.alloc(Cout * count * ctb + 64)
    try:
        E.set_tuning("sq_chunk", chunk)
        d_work = E.alloc(max(E.diag_mac_work_bytes(count, T), E.conv_slots_work_bytes(count, Cin, Cout, T)))
        for fin in (ca.COEFF, ca.NTT):
            d_x = E.upload(x)
            if fin == ca.NTT:
                E.ntt_fwd(d_x, Cin * count)
            for co in range(Cout):
                for ci in range(Cin):
                    dst = d_ref.ptr + co * count * ctb if ci == 0 else d_tmp.ptr
                    E.diag_mac(d_x.ptr + ci * count * ctb, count, gs, d_p.ptr + (co * Cin + ci) * T * rowb, d_cg, elts, dst, d_work, in_form=fin, out_form=ca.NTT)
                    if ci:
                        E.add(d_ref.ptr + co * count * ctb, d_tmp, count)
            want = {ca.NTT: E.download(d_ref, (outw,))}
            E.ntt_inv(d_ref, Cout * count)
            want[ca.COEFF] = E.download(d_ref, (outw,))
            for fout in ((ca.COEFF, ca.NTT) if forms == 4 else (fin,)):
                for path, rt, jt in tunings:
                    E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt); E.set_tuning("conv_jt", jt)
                    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                    E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_y, d_work, in_form=fin, out_form=fout)
                    E.set_tuning("relin_path", 0); E.set_tuning("hoist_rt", 0); E.set_tuning("conv_jt", 0)
                    got = E.download(d_y, (outw + 8,))
                    assert np.array_equal(got[:-8], want[fout]), (fin, fout, path, rt, jt)
                    assert (got[-8:] == np.uint64(FF)).all(), (fin, fout, path, rt, jt, "wrote past the end")
            if fin == ca.COEFF:
                assert np.array_equal(E.download(d_x, x.shape), x)     # the input is only read
    finally:
        reset(E)
    E.close(); H.close()


@pytest.mark.parametrize("fill", ["q_minus_1", "random"])
def test_worst_case_operands_no_keys(fill):
    """n = 256, one 60-bit modulus (the width class of tests/golden/ops_n256_k1_q60_t30.npz): 127 - 2 . 60 = 7, so a reduction may sum 2^7 = 128 terms.  Every
    element is 1 (no key, no key switch), T = 34, Cin = 4: 136 terms -- a launch of 32 taps x 4 channels = 128 terms at the bound, then 2 taps x 4 channels
    accumulated onto the reduced sum.  NTT-form input and weights all q - 1: every output residue is 136 (q - 1)^2 = 136 mod q; then random residues (q - 1 and
    0 among them) against Python integers.  count = 2, Cout = 3 (a tail tile at every conv_jt), coefficient-form input through the one shared transform as well"""
    import crcnn_amd as ca
    g = dict(np.load(GOLD60))
    n, q, t = int(g["n"]), [int(v) for v in g["q"]], int(g["t"])
    assert n == 256 and len(q) == 1 and q[0].bit_length() == 60
    Q = q[0]
    Cin, Cout, T, count = 4, 3, 34, 2
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(60)
    if fill == "q_minus_1":
        x = np.full((Cin, count, 2, 1, n), Q - 1, dtype=np.uint64)
        w = np.full((1, Cout, Cin, T), Q - 1, dtype=np.uint64)
    else:
        x = (rng.randint(0, 1 << 62, size=(Cin, count, 2, 1, n)).astype(np.uint64) % np.uint64(Q))
        w = (rng.randint(0, 1 << 62, size=(1, Cout, Cin, T)).astype(np.uint64) % np.uint64(Q))
        x[0, 0, 0, 0, :4] = [Q - 1, 0, 1, Q - 1]; w[0, 0, 0, :3] = [Q - 1, 0, 1]
    ws = w[0].astype(object).sum(axis=2)                                # every element is 1: y[co] = Sum_ci (Sum_tau w) x[ci]
    want = np.zeros((Cout, count, 2, 1, n), dtype=object)
    for co in range(Cout):
        for ci in range(Cin):
            want[co] = (want[co] + int(ws[co, ci]) * x[ci].astype(object)) % Q
    if fill == "q_minus_1":
        assert (want == 136 % Q).all()
    want = want.astype(np.uint64)
    gs = [1] * T
    d_x = E.upload(x); d_w = E.upload(w)
    d_y = E.alloc(want.nbytes + 64)
    d_work = E.alloc(E.conv_slots_work_bytes(count, Cin, Cout, T))
    d_xc = E.upload(x); E.ntt_inv(d_xc, Cin * count)                   # the same ciphertexts in coefficient form
    try:
        for jt in JTS:
            for src, fin in ((d_x, ca.NTT), (d_xc, ca.COEFF)):
                E.set_tuning("conv_jt", jt)
                E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                E.conv_slots(src, count, Cin, gs, d_w, Cout, None, [], d_y, d_work, in_form=fin, out_form=ca.NTT)
                got = E.download(d_y, (want.size + 8,))
                assert np.array_equal(got[:-8], want.reshape(-1)), (jt, fin)
                assert (got[-8:] == np.uint64(FF)).all()
    finally:
        reset(E)
    assert np.array_equal(E.download(d_x, x.shape), x)
    E.close()


def test_one_tap_of_element_1_and_weight_1_is_the_input():
    import crcnn_amd as ca
    n, k, t, count = 4096, 2, 65537, 3
    q = moduli(n, k)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(1)
    x = np.stack([rng.randint(0, 1 << 62, size=(count, 2, n)).astype(np.uint64) % np.uint64(qi) for qi in q], axis=2)      # [count][2][k][n]
    d_w = E.upload(E.conv_slots_pack_weights([1]))
    d_y = E.alloc(x.nbytes + 64)
    d_work = E.alloc(E.conv_slots_work_bytes(count, 1, 1, 1))
    d_c = E.upload(x); d_n = E.upload(x); E.ntt_fwd(d_n, count)
    forms = {ca.COEFF: (d_c, x), ca.NTT: (d_n, E.download(d_n, x.shape))}
    for fin in forms:
        for fout in forms:
            E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
            E.conv_slots(forms[fin][0], count, 1, [1], d_w, 1, None, [], d_y, d_work, in_form=fin, out_form=fout)
            got = E.download(d_y, (x.size + 8,))
            assert np.array_equal(got[:-8], forms[fout][1].reshape(-1)), (fin, fout)
            assert (got[-8:] == np.uint64(FF)).all()
    E.close()


def test_two_layers_through_encryption():
    """(4096, 2 moduli, t = 65537), one 12 x 12 image at pitch 12, M = 256.  conv 1 -> 2 of 3 x 3 with pool = 2 (a 4 x 4 window, 16 taps; 5 x 5 outputs at
    dilation 2), then conv 2 -> 3 of 3 x 3 at that dilation (3 x 3 outputs).  Pixels in [0, 3], weights in [-2, 2]: the integers stay below 16 . 8 . 3 = 384
    after the first layer and 2 . 9 . 2 . 384 = 13 824 < t / 2 after the second.  First the composed reference path (crc_diag_mac_forms per channel pair, crc_add)
    alone must leave a positive noise budget after both layers; then every valid slot of every period of the fused path's result is the integer convolution, and
    its budget is positive too"""
    import crcnn_amd as ca
    n, k, t, M, pitch = 4096, 2, 65537, 256, 12
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(12)
    img = rng.randint(0, 4, size=(1, 12, 12)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64)
    w2 = rng.randint(-2, 3, size=(3, 2, 3, 3)).astype(np.int64)
    p1 = E.conv_slots_plan(M, pitch, 12, 12, 3, 3, 1, 2)
    assert len(p1.steps) == 16 and (p1.out_h, p1.out_w, p1.out_dil) == (5, 5, 2)
    p2 = E.conv_slots_plan(M, pitch, p1.out_h, p1.out_w, 3, 3, p1.out_dil, 1)
    assert len(p2.steps) == 9 and (p2.out_h, p2.out_w, p2.out_dil) == (3, 3, 2)
    mid = cm.conv_direct(img, w1, 2)
    want = cm.conv_direct(mid, w2, 1)
    assert int(np.abs(mid).max()) <= 384 and int(np.abs(want).max()) <= 13824 < t // 2
    sk, pk = H.keygen(31)
    need = sorted(set(p1.elements + p2.elements) - {1})
    elts, gk = H.gen_galois_keys(32, sk, elts=need)
    d_cg = E.upload(H.galois_conjugate_keys(elts, gk)); d_sk = E.upload(sk)
    plane = cm.plane_slots(img[0], n, M, pitch, 1).astype(np.int64)
    d_x = E.upload(H.encrypt(pk, H.slots_compose(plane, 1, n, n, 1), 33))
    rowb = k * n * 8; ctb = 2 * rowb
    f1, f2 = p1.fold(w1, t), p2.fold(w2, t)
    d_w1 = E.upload(H.conv_slots_pack_weights(f1)); d_w2 = E.upload(H.conv_slots_pack_weights(f2))
    d_m = E.alloc(2 * ctb); d_y = E.alloc(3 * ctb); d_tmp = E.alloc(ctb)
    d_work = E.alloc(max(E.conv_slots_work_bytes(1, 1, 2, 16), E.conv_slots_work_bytes(1, 2, 3, 9), E.diag_mac_work_bytes(1, 16)))
    d_bits = E.alloc(3 * 4); d_bw = E.alloc(E.noise_budget_dev_work_bytes(3))
    d_pl = E.alloc(3 * n * 8); d_o = E.alloc(3 * n * 8); d_dw = E.alloc(E.decrypt_dev_work_bytes(3))

    def budgets(what):
        E.noise_budget_dev(d_sk, d_y, 3, d_bits, d_bw)
        b = E.download(d_bits, (3,), dtype=np.int32).tolist()
        print(what, "noise budget:", b)
        return min(b)

    def composed(d_in, Cin, plan, fold, Cout, d_out):
        consts = np.zeros((Cout * Cin * len(plan.steps), n), dtype=np.uint64)
        consts[:, 0] = fold.reshape(-1).astype(np.uint64)
        d_p = E.alloc(consts.shape[0] * rowb)
        E.plain_to_ntt(E.upload(consts), consts.shape[0], d_p)
        for co in range(Cout):
            for ci in range(Cin):
                dst = d_out.ptr + co * ctb if ci == 0 else d_tmp.ptr
                E.diag_mac(d_in.ptr + ci * ctb, 1, plan.elements, d_p.ptr + (co * Cin + ci) * len(plan.steps) * rowb, d_cg, elts, dst, d_work)
                if ci:
                    E.add(d_out.ptr + co * ctb, d_tmp, 1)

    composed(d_x, 1, p1, f1, 2, d_m)
    composed(d_m, 2, p2, f2, 3, d_y)
    assert budgets("composed reference, two layers") >= 1
    ref = E.download(d_y, (3 * ctb // 8,))
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    E.conv_slots(d_x, 1, 1, p1.elements, d_w1, 2, d_cg, elts, d_m, d_work)
    E.conv_slots(d_m, 1, 2, p2.elements, d_w2, 3, d_cg, elts, d_y, d_work)
    assert np.array_equal(E.download(d_y, (3 * ctb // 8,)), ref)       # (and the two paths agree bit for bit)
    assert budgets("fused, two layers") >= 1
    E.decrypt_dev(d_sk, d_y, 3, d_pl, d_dw)
    E.slots_decompose_dev(d_pl, 3, n, d_o, n, 1)
    got = E.download(d_o, (3, n), dtype=np.int64)
    for co in range(3):
        for base in range(0, n, M):
            assert [int(got[co, base + s]) for s in p2.valid] == [int(v) for v in want[co].reshape(-1)], (co, base)
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
    Cin, Cout, T = 2, 2, 3
    d_x = E.alloc(Cin * ctb + 64); d_y = E.alloc(Cout * ctb + 64); d_cg = E.upload(cg); d_w = E.alloc(Cout * Cin * T * 8 + 64)
    d_work = E.alloc(E.conv_slots_work_bytes(1, Cin, Cout, T))
    E.L.crc_memset(E.c, d_x.ptr, 0, d_x.nbytes, E.stream); E.L.crc_memset(E.c, d_w.ptr, 0, d_w.nbytes, E.stream)
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    pe = pu(elts); ne = len(elts)
    no9 = np.ascontiguousarray(elts[elts != 9])
    A = lambda *g: pu(E._elts(list(g)))

    def f(gs=A(1, 3, 9), T=T, ci=Cin, co=Cout, x=d_x.ptr, y=d_y.ptr, w=d_w.ptr, ck=d_cg.ptr, e=pe, m=ne, dbc=16, fi=0, fo=0, wk=d_work.ptr, c=None, cnt=1):
        return E.L.crc_conv_slots_forms(c or E.c, x, fi, cnt, ci, gs, T, w, co, ck, e, m, dbc, y, fo, wk, None)
    assert f(e=pu(no9), m=len(no9)) == -1 and f(gs=A(1, 3, 27)) == -1 and f(m=0) == -1          # a missing conjugated key
    assert f(gs=A(1, 2, 9)) == -1 and f(gs=A(2 * n + 1, 3, 9)) == -1 and f(gs=A(0, 3, 9)) == -1 and f(gs=None) == -1   # an invalid element
    assert f(T=0) == -1 and f(T=-1) == -1 and f(ci=0) == -1 and f(ci=-1) == -1 and f(co=0) == -1 and f(co=-1) == -1
    assert f(T=1025) == -1 and f(ci=4097) == -1 and f(co=4097) == -1                             # above the caps
    assert f(w=d_w.ptr + 8) == -1 and f(w=None) == -1                                            # a misaligned or absent d_w
    assert f(w=d_y.ptr) == -1 and f(w=d_y.ptr + Cout * ctb - 16) == -1 and f(w=d_work.ptr + 256) == -1      # d_w inside d_y or d_work
    assert f(wk=d_y.ptr) == -1 and f(y=d_work.ptr + 4096) == -1 and f(y=d_x.ptr) == -1 and f(wk=d_x.ptr) == -1
    assert f(y=d_x.ptr + ctb) == -1                                                              # d_y over the second input channel
    assert f(x=d_x.ptr + 8) == -1 and f(y=d_y.ptr + 8) == -1 and f(ck=d_cg.ptr + 8) == -1 and f(x=None) == -1 and f(y=None) == -1 and f(wk=None) == -1
    assert f(ck=None) == -1 and f(fi=ca.NTTP) == -1 and f(fo=ca.NTTL) == -1 and f(dbc=0) == -1 and f(dbc=61) == -1
    assert f(c=H.c) == -1                                                                        # a host-only context
    assert f(cnt=0) == 0                                                                         # an empty batch is no error
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    assert f() == 0                                                                              # ... and the call they all vary is a valid one
    assert (E.download(d_y, (Cout * ctb // 8,)) == 0).all()                                      # (of zero ciphertexts)
    assert (E.download(d_y, (d_y.nbytes // 8,))[-8:] == np.uint64(FF)).all()
    E.close(); H.close()
