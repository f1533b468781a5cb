"""The packed convolution with a bias and a mask on the GPU: crc_conv_slots_bias_mask_forms against the composition it is defined as (crc_conv_slots_forms into
NTT form, crc_add_plain per output channel, crc_multiply_plain_ntt by the mask row, one inverse transform) bit for bit at every tuning setting, worst-case operands
at a 60-bit modulus against Python integers, NULL / NULL against crc_conv_slots_forms, padded and strided layers through encryption against the integer
convolution, and the refusals."""
import os

import numpy as np
import pytest

import conv_slots_pad_model as pm
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


def residue_rows(rng, q, n):
    """[k][n] arbitrary canonical residues, 0, 1 and q - 1 among them: the mask operand need not be a mask"""
    m = np.stack([rng.randint(0, 1 << 62, size=n).astype(np.uint64) % np.uint64(qi) for qi in q])
    for i, qi in enumerate(q):
        m[i, :3] = [0, 1, qi - 1]
        m[i, -1] = qi - 1
    return m


@pytest.mark.parametrize("n,k,Cin,Cout,T,count,chunk,forms,tunings", [
    (4096, 2, 2, JT + 1, 3, 2, 0, 4, [(p, rt, jt) for p in (0, 1) for rt in (1, 2) for jt in JTS]),
    (256, 2, 3, 2, 34, 3, 8, 2, [(0, 1, 0), (0, 2, 8), (1, 0, 2), (0, 0, 4)]),
    (64, 1, 2, 2 * JT + 1, 3, 2, 0, 2, [(0, 0, jt) for jt in JTS])],
    ids=["n4096_tile_and_tail_every_setting", "n256_T34_two_tap_groups_passes_across_channels", "n64_one_workgroup_three_tiles"])
def test_fused_equals_composition(n, k, Cin, Cout, T, count, chunk, forms, tunings):
    """The composition, built once per input form at the default tuning from the existing entry points: crc_conv_slots_forms into NTT form; per output channel
    crc_add_plain (sign +1, group = count) of the NTT-form delta row of the constant b[co]; crc_multiply_plain_ntt of all Cout count ciphertexts by the one mask
    row; one inverse transform for coefficient output.  The fused call must give its bits -- with the bias alone, the mask alone and both at the default tuning,
    and with both at every listed setting.  The shapes are test_gpu_conv_slots.py's: at n = 256 with sq_chunk = 8 a row is written by one launch and accumulated
    into by further tap groups and by later passes that begin inside a channel, which is where a mask applied to the accumulated value, or a bias added per
    launch, would show.  The mask row holds arbitrary residues.  Guard words behind d_y stay 0xff; the input is only read"""
    import crcnn_amd as ca
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 20)
    gs = [gm.elt_rows(n, s) for s in range(T)]
    gs[0], gs[1] = gs[1], gs[0]                                         # the element 1 in the middle of the first pair
    assert gs[1] == 1 and len(set(gs)) == T
    q, H, sk, pk, elts, gk, cg, v, x = keyed_case(n, k, t, Cin * count, gs, [1], n + T + 1)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(n + Cout + 1)
    w = rng.randint(-(t // 2), t // 2 + 1, size=(Cout, Cin, T)).astype(np.int64)
    w[0, 0, 0] = t - 1; w[-1, -1, -1] = 0; w[0, 0, 1] = (t + 1) // 2
    b = rng.randint(-(t // 2), t // 2 + 1, size=Cout).astype(np.int64)
    b[0] = t - 1; b[1] = (t + 1) // 2; b[-1] = 0
    bl = H.conv_slots_pack_bias(b)
    consts = np.zeros((Cout, n), dtype=np.uint64)
    consts[:, 0] = (b % t).astype(np.uint64)
    rowb = k * n * 8; ctb = 2 * rowb
    d_delta = E.alloc(Cout * rowb)
    E.plain_to_delta(E.upload(consts), Cout, ca.NTT, d_delta)
    assert (E.download(d_delta, (Cout, k, n)) == bl.T[..., None]).all()  # d_bias holds the word at every position of the constant's delta row
    mask = residue_rows(rng, q, n)
    d_w = E.upload(H.conv_slots_pack_weights(w)); d_cg = E.upload(cg); d_b = E.upload(bl); d_m = E.upload(mask)
    outw = Cout * count * ctb // 8
    d_ref = E.alloc(Cout * count * ctb); d_y = E.alloc(Cout * count * ctb + 64)
    try:
        E.set_tuning("sq_chunk", chunk)
        d_work = E.alloc(E.conv_slots_work_bytes(count, Cin, Cout, T))
        for fin in (ca.COEFF, ca.NTT):
            d_x = E.upload(x)
            if fin == ca.NTT:
                E.ntt_fwd(d_x, Cin * count)
            xin = E.download(d_x, x.shape)
            want = {}
            for what, use_b, use_m in (("bias", True, False), ("mask", False, True), ("both", True, True)):
                E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_ref, d_work, in_form=fin, out_form=ca.NTT)
                if use_b:
                    for co in range(Cout):
                        E.add_plain(d_ref.ptr + co * count * ctb, d_delta.ptr + co * rowb, count, count, 1)
                if use_m:
                    E.multiply_plain_ntt(d_ref, d_m, Cout * count, Cout * count)
                want[what, ca.NTT] = E.download(d_ref, (outw,))
                E.ntt_inv(d_ref, Cout * count)
                want[what, ca.COEFF] = E.download(d_ref, (outw,))
            assert not np.array_equal(want["bias", ca.NTT], want["both", ca.NTT]) and not np.array_equal(want["mask", ca.NTT], want["both", ca.NTT])
            for fout in ((ca.COEFF, ca.NTT) if forms == 4 else (fin,)):
                for what, path, rt, jt in [("bias", 0, 0, 0), ("mask", 0, 0, 0)] + [("both",) + s for s in tunings]:
                    E.set_tuning("relin_path", path); E.set_tuning("hoist_rt", rt); E.set_tuning("conv_jt", jt)
                    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                    E.conv_slots_bias_mask(d_x, count, Cin, gs, d_w, Cout, d_b if what != "mask" else None, d_m if what != "bias" else None, d_cg, elts, d_y, d_work,
                                           in_form=fin, out_form=fout)
                    E.set_tuning("relin_path", 0); E.set_tuning("hoist_rt", 0); E.set_tuning("conv_jt", 0)
                    got = E.download(d_y, (outw + 8,))
                    assert np.array_equal(got[:-8], want[what, fout]), (fin, fout, what, path, rt, jt)
                    assert (got[-8:] == np.uint64(FF)).all(), (fin, fout, what, path, rt, jt, "wrote past the end")
            assert np.array_equal(E.download(d_x, x.shape), xin)       # the input is only read
        assert np.array_equal(E.download(d_b, bl.shape), bl) and np.array_equal(E.download(d_m, mask.shape), mask)
    finally:
        reset(E)
    E.close(); H.close()


@pytest.mark.parametrize("fill", ["q_minus_1", "random"])
def test_worst_case_operands_no_keys(fill):
    """n = 256, one 60-bit modulus: a reduction may sum 2^7 = 128 terms.  Every element is 1 (no key), T = 34, Cin = 4: 136 terms in launches of 128 + 8, the
    second accumulating.  Inputs, weights, bias and mask all q - 1 = -1: the sum is 136, so polynomial 0 holds (136 - 1) (-1) = q - 135 and polynomial 1
    136 (-1) = q - 136 -- a bias added by both launches would give q - 134, a mask applied to the accumulated value -(-127 + 8) = 119.  Then random residues
    (q - 1 and 0 among them) against Python integers, at every conv_jt.  count = 2, Cout = 3 (a tail tile at every conv_jt)"""
    import crcnn_amd as ca
    g = dict(np.load(GOLD60))
    n, q, t = int(g["n"]), [int(v) for v in g["q"]], int(g["t"])
    assert n == 256 and len(q) == 1 and q[0].bit_length() == 60
    Q = q[0]
    Cin, Cout, T, count = 4, 3, 34, 2
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(61)
    if fill == "q_minus_1":
        x = np.full((Cin, count, 2, 1, n), Q - 1, dtype=np.uint64)
        w = np.full((1, Cout, Cin, T), Q - 1, dtype=np.uint64)
        b = np.full((1, Cout), Q - 1, dtype=np.uint64)
        m = np.full((1, n), Q - 1, dtype=np.uint64)
    else:
        x = (rng.randint(0, 1 << 62, size=(Cin, count, 2, 1, n)).astype(np.uint64) % np.uint64(Q))
        w = (rng.randint(0, 1 << 62, size=(1, Cout, Cin, T)).astype(np.uint64) % np.uint64(Q))
        b = (rng.randint(0, 1 << 62, size=(1, Cout)).astype(np.uint64) % np.uint64(Q))
        m = residue_rows(rng, q, n)
        x[0, 0, 0, 0, :4] = [Q - 1, 0, 1, Q - 1]; w[0, 0, 0, :3] = [Q - 1, 0, 1]; b[0, 0] = Q - 1
    ws = w[0].astype(object).sum(axis=2)                                # every element is 1: y[co] = m ( Sum_ci (Sum_tau w) x[ci] + b[co] on polynomial 0 )
    want = np.zeros((Cout, count, 2, 1, n), dtype=object)
    for co in range(Cout):
        for ci in range(Cin):
            want[co] = (want[co] + int(ws[co, ci]) * x[ci].astype(object)) % Q
        want[co][:, 0] = (want[co][:, 0] + int(b[0, co])) % Q
        want[co] = (want[co] * m[0].astype(object)) % Q
    if fill == "q_minus_1":
        assert (want[:, :, 0] == Q - 135).all() and (want[:, :, 1] == Q - 136).all()
    want = want.astype(np.uint64)
    gs = [1] * T
    d_x = E.upload(x); d_w = E.upload(w); d_b = E.upload(b); d_m = E.upload(m)
    d_y = E.alloc(want.nbytes + 64)
    d_work = E.alloc(E.conv_slots_work_bytes(count, Cin, Cout, T))
    d_xc = E.upload(x); E.ntt_inv(d_xc, Cin * count)                   # the same ciphertexts in coefficient form
    try:
        for jt in JTS:
            for src, fin in ((d_x, ca.NTT), (d_xc, ca.COEFF)):
                E.set_tuning("conv_jt", jt)
                E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                E.conv_slots_bias_mask(src, count, Cin, gs, d_w, Cout, d_b, d_m, None, [], d_y, d_work, in_form=fin, out_form=ca.NTT)
                got = E.download(d_y, (want.size + 8,))
                assert np.array_equal(got[:-8], want.reshape(-1)), (jt, fin)
                assert (got[-8:] == np.uint64(FF)).all()
    finally:
        reset(E)
    assert np.array_equal(E.download(d_x, x.shape), x)
    E.close()


def test_null_null_is_conv_slots():
    """neither a bias nor a mask: crc_conv_slots_forms bit for bit, all four form pairs"""
    import crcnn_amd as ca
    n, k, t, Cin, Cout, T, count = 4096, 2, 65537, 2, 5, 3, 2
    gs = [gm.elt_rows(n, s) for s in (1, 0, 2)]
    q, H, sk, pk, elts, gk, cg, v, x = keyed_case(n, k, t, Cin * count, gs, [1], 99)
    E = ca.Engine(n, q, t, device=0)
    w = np.random.RandomState(9).randint(-(t // 2), t // 2 + 1, size=(Cout, Cin, T)).astype(np.int64)
    d_w = E.upload(H.conv_slots_pack_weights(w)); d_cg = E.upload(cg)
    ctb = 2 * k * n * 8
    d_a = E.alloc(Cout * count * ctb); d_b = E.alloc(Cout * count * ctb)
    d_work = E.alloc(E.conv_slots_work_bytes(count, Cin, Cout, T))
    for fin in (ca.COEFF, ca.NTT):
        d_x = E.upload(x)
        if fin == ca.NTT:
            E.ntt_fwd(d_x, Cin * count)
        for fout in (ca.COEFF, ca.NTT):
            E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_a, d_work, in_form=fin, out_form=fout)
            E.L.crc_memset(E.c, d_b.ptr, 0xff, d_b.nbytes, E.stream)
            E.conv_slots_bias_mask(d_x, count, Cin, gs, d_w, Cout, None, None, d_cg, elts, d_b, d_work, in_form=fin, out_form=fout)
            assert np.array_equal(E.download(d_a, (d_a.nbytes // 8,)), E.download(d_b, (d_b.nbytes // 8,))), (fin, fout)
    E.close(); H.close()


class Net:
    """one image through two planned layers at (4096, 2 moduli, t = 65537): keys, buffers, the composition and the fused path of a layer, budgets, decryption"""
    def __init__(self, plans, couts, seed):
        import crcnn_amd as ca
        self.ca = ca
        self.n, self.k, self.t = 4096, 2, 65537
        n, k, t = self.n, self.k, self.t
        q = moduli(n, k)
        self.H = ca.Engine(n, q, t, device=-1)
        self.E = ca.Engine(n, q, t, device=0)
        H, E = self.H, self.E
        self.sk, self.pk = H.keygen(seed)
        need = sorted({g for p in plans for g in p.elements} - {1})
        self.elts, gk = H.gen_galois_keys(seed + 1, self.sk, elts=need)
        self.d_cg = E.upload(H.galois_conjugate_keys(self.elts, gk)); self.d_sk = E.upload(self.sk)
        self.rowb = k * n * 8; self.ctb = 2 * self.rowb
        cmax = max(couts)
        shapes = [(1, couts[0], len(plans[0].steps)), (couts[0], couts[1], len(plans[1].steps))]
        self.d_work = E.alloc(max(E.conv_slots_work_bytes(1, ci, co, T) for ci, co, T in shapes))
        self.d_bits = E.alloc(cmax * 4); self.d_bw = E.alloc(E.noise_budget_dev_work_bytes(cmax))
        self.d_pl = E.alloc(cmax * n * 8); self.d_o = E.alloc(cmax * n * 8); self.d_dw = E.alloc(E.decrypt_dev_work_bytes(cmax))

    def encrypt(self, plane_slots, seed):
        n = self.n
        return self.E.upload(self.H.encrypt(self.pk, self.H.slots_compose(np.asarray(plane_slots, dtype=np.int64).reshape(1, n), 1, n, n, 1), seed))

    def operands(self, plan, w, bias, masked):
        """(d_w, d_bias or None, d_mask or None, d_delta rows [Cout][k][n] or None) of one layer"""
        E, H, n, t = self.E, self.H, self.n, self.t
        d_w = E.upload(H.conv_slots_pack_weights(plan.fold(w, t)))
        d_b = d_delta = d_m = None
        if bias is not None:
            d_b = E.upload(H.conv_slots_pack_bias(bias))
            consts = np.zeros((len(bias), n), dtype=np.uint64)
            consts[:, 0] = (np.asarray(bias) % t).astype(np.uint64)
            d_delta = E.alloc(len(bias) * self.rowb)
            E.plain_to_delta(E.upload(consts), len(bias), self.ca.NTT, d_delta)
        if masked:
            d_m = E.alloc(self.rowb)
            E.plain_to_ntt(E.upload(H.slots_compose(plan.mask_slots().reshape(1, n), 1, n, n, 1)), 1, d_m)
        return d_w, d_b, d_m, d_delta

    def composed(self, d_in, Cin, plan, ops, Cout, d_out):
        E, ca = self.E, self.ca
        d_w, d_b, d_m, d_delta = ops
        E.conv_slots(d_in, 1, Cin, plan.elements, d_w, Cout, self.d_cg, self.elts, d_out, self.d_work, out_form=ca.NTT)
        if d_delta is not None:
            for co in range(Cout):
                E.add_plain(d_out.ptr + co * self.ctb, d_delta.ptr + co * self.rowb, 1, 1, 1)
        if d_m is not None:
            E.multiply_plain_ntt(d_out, d_m, Cout, Cout)
        E.ntt_inv(d_out, Cout)

    def fused(self, d_in, Cin, plan, ops, Cout, d_out):
        d_w, d_b, d_m, _ = ops
        self.E.conv_slots_bias_mask(d_in, 1, Cin, plan.elements, d_w, Cout, d_b, d_m, self.d_cg, self.elts, d_out, self.d_work)

    def budget(self, what, d_y, count):
        E = self.E
        E.noise_budget_dev(self.d_sk, d_y, count, self.d_bits, self.d_bw)
        b = E.download(self.d_bits, (count,), dtype=np.int32).tolist()
        print(what, "noise budget:", b)
        return min(b)

    def slots(self, d_y, count):
        E, n = self.E, self.n
        E.decrypt_dev(self.d_sk, d_y, count, self.d_pl, self.d_dw)
        E.slots_decompose_dev(self.d_pl, count, n, self.d_o, n, 1)
        return E.download(self.d_o, (count, n), dtype=np.int64)

    def close(self):
        self.E.close(); self.H.close()


def check_valid(got, plan, want, M, n):
    for co in range(want.shape[0]):
        for base in range(0, n, M):
            assert [int(got[co, base + s]) for s in plan.valid] == [int(v) for v in want[co].reshape(-1)], (co, base)


def test_padded_layers_through_encryption():
    """(4096, 2 moduli, t = 65537), one 12 x 12 image with a margin of one (pitch 13, origin 14), M = 256.  Layer 1 -> 2: 3 x 3, pad 1, stride 1, with a bias and
    the mask -- a 'same' layer whose result is clean.  Layer 2 -> 3: 3 x 3, pad 1, stride 2, whose padding taps read the margin the mask zeroed.  Pixels in
    [0, 3], weights in [-2, 2], bias in [-3, 3]: at most 9 . 2 . 3 + 3 = 57 after the first layer and 2 . 9 . 2 . 57 = 2052 < t / 2 after the second.  First the
    composition alone must leave a budget >= 1; then the fused path equals it bit for bit, keeps a budget >= 1, decrypts to the direct convolution at every valid
    slot of every period, and layer 1's result to 0 at every other slot.  The budgets are printed: before and after the mask, and after both layers"""
    import crcnn_amd as ca
    n, M, pitch, origin, t = 4096, 256, 13, 14, 65537
    rng = np.random.RandomState(21)
    img = rng.randint(0, 4, size=(1, 12, 12)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64); b1 = np.array([-3, 3], dtype=np.int64)
    w2 = rng.randint(-2, 3, size=(3, 2, 3, 3)).astype(np.int64)
    p1 = ca.binding.conv_slots_plan_geom(n, M, pitch, origin, 12, 12, 3, 3, 1, 1, 1)
    assert len(p1.steps) == 9 and (p1.out_h, p1.out_w, p1.out_dil) == (12, 12, 1) and p1.needs_clean_input
    p2 = ca.binding.conv_slots_plan_geom(n, M, pitch, origin, p1.out_h, p1.out_w, 3, 3, p1.out_dil, 1, 2)
    assert len(p2.steps) == 9 and (p2.out_h, p2.out_w, p2.out_dil) == (6, 6, 2)
    mid = pm.conv_direct_geom(img, w1, 1, bias=b1)
    want = pm.conv_direct_geom(mid, w2, 1, 2)
    assert int(np.abs(mid).max()) <= 57 and int(np.abs(want).max()) <= 2052 < t // 2
    N = Net([p1, p2], [2, 3], 31)
    E = N.E
    d_x = N.encrypt(pm.plane_slots_geom(img[0], n, M, pitch, origin, 1), 33)
    o1 = N.operands(p1, w1, b1, True); o1_plain = (o1[0], o1[1], None, o1[3]); o2 = N.operands(p2, w2, None, False)
    d_m = E.alloc(2 * N.ctb); d_y = E.alloc(3 * N.ctb)
    N.composed(d_x, 1, p1, o1_plain, 2, d_m)
    before = N.budget("layer 1 with its bias, no mask", d_m, 2)
    N.composed(d_x, 1, p1, o1, 2, d_m)
    after = N.budget("layer 1 with its bias and the mask (composition)", d_m, 2)
    assert before > after >= 1
    ref1 = E.download(d_m, (2 * N.ctb // 8,))
    N.composed(d_m, 2, p2, o2, 3, d_y)
    assert N.budget("composition, two layers", d_y, 3) >= 1
    ref2 = E.download(d_y, (3 * N.ctb // 8,))
    E.L.crc_memset(E.c, d_m.ptr, 0xff, d_m.nbytes, E.stream); E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    N.fused(d_x, 1, p1, o1, 2, d_m)
    assert np.array_equal(E.download(d_m, (2 * N.ctb // 8,)), ref1)
    assert N.budget("fused, layer 1", d_m, 2) >= 1
    got1 = N.slots(d_m, 2)
    check_valid(got1, p1, mid, M, n)
    outside = np.tile(1 - p1.mask_slots()[:M], n // M).astype(bool)
    assert not got1[:, outside].any()                                  # a clean plane: exactly 0 at every slot that holds no output
    N.fused(d_m, 2, p2, o2, 3, d_y)
    assert np.array_equal(E.download(d_y, (3 * N.ctb // 8,)), ref2)
    assert N.budget("fused, two layers", d_y, 3) >= 1
    check_valid(N.slots(d_y, 3), p2, want, M, n)
    N.close()


def test_strided_pooled_front_through_encryption():
    """ApproxPlainModel's front at 12 x 12, 1 -> 2 channels: a 5 x 5 convolution of stride 2 (4 x 4 outputs), a sum pool of window 2 and stride 1 on them (3 x 3
    outputs, a 7 x 7 window of 49 taps), a per-channel scale folded into the weights and a bias; then 2 -> 3 channels, 3 x 3 of stride 2 at the dilation the first
    layer left (1 x 1 output).  No padding, so no mask and no margin.  Pixels in [0, 3], weights in [-2, 2], scales in {2, 3}, bias in [-3, 3]: at most
    4 . 25 . 3 . 2 . 3 + 3 = 1803 after the first layer; 2 . 9 . 2 . 1803 = 64 908 would pass t / 2, so the second layer's weights stay in [-1, 1]: 32 454 < t / 2"""
    import crcnn_amd as ca
    n, M, pitch, t = 4096, 256, 12, 65537
    rng = np.random.RandomState(22)
    img = rng.randint(0, 4, size=(1, 12, 12)).astype(np.int64)
    scale = np.array([2, 3], dtype=np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 5, 5)).astype(np.int64) * scale.reshape(2, 1, 1, 1); b1 = np.array([3, -2], dtype=np.int64)
    w2 = rng.randint(-1, 2, size=(3, 2, 3, 3)).astype(np.int64)
    p1 = ca.binding.conv_slots_plan_geom(n, M, pitch, 0, 12, 12, 5, 5, 1, 0, 2, 2, 1)
    assert len(p1.steps) == 49 and (p1.out_h, p1.out_w, p1.out_dil) == (3, 3, 2) and not p1.needs_clean_input
    p2 = ca.binding.conv_slots_plan_geom(n, M, pitch, 0, p1.out_h, p1.out_w, 3, 3, p1.out_dil, 0, 2)
    assert len(p2.steps) == 9 and (p2.out_h, p2.out_w, p2.out_dil) == (1, 1, 4)
    mid = pm.conv_direct_geom(img, w1, 0, 2, 2, 1, bias=b1)
    want = pm.conv_direct_geom(mid, w2, 0, 2)
    assert int(np.abs(mid).max()) <= 1803 and int(np.abs(want).max()) <= 32454 < t // 2
    N = Net([p1, p2], [2, 3], 41)
    E = N.E
    d_x = N.encrypt(pm.plane_slots_geom(img[0], n, M, pitch, 0, 1), 43)
    o1 = N.operands(p1, w1, b1, False); o2 = N.operands(p2, w2, None, False)
    d_m = E.alloc(2 * N.ctb); d_y = E.alloc(3 * N.ctb)
    N.composed(d_x, 1, p1, o1, 2, d_m)
    N.composed(d_m, 2, p2, o2, 3, d_y)
    assert N.budget("composition, strided front and the layer behind it", d_y, 3) >= 1
    ref = E.download(d_y, (3 * N.ctb // 8,))
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    N.fused(d_x, 1, p1, o1, 2, d_m)
    check_valid(N.slots(d_m, 2), p1, mid, M, n)
    N.fused(d_m, 2, p2, o2, 3, d_y)
    assert np.array_equal(E.download(d_y, (3 * N.ctb // 8,)), ref)
    assert N.budget("fused, strided front and the layer behind it", d_y, 3) >= 1
    check_valid(N.slots(d_y, 3), p2, want, M, n)
    N.close()


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
    d_b = E.alloc(Cout * 8 + 64); d_m = E.alloc(n * 8 + 64)
    d_work = E.alloc(E.conv_slots_work_bytes(1, Cin, Cout, T))
    for d in (d_x, d_w, d_b, d_m):
        E.L.crc_memset(E.c, d.ptr, 0, d.nbytes, E.stream)
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    pe = pu(elts); ne = len(elts)
    no9 = np.ascontiguousarray(elts[elts != 9])
    A = lambda *g: pu(E._elts(list(g)))

    def f(gs=A(1, 3, 9), T=T, ci=Cin, co=Cout, x=d_x.ptr, y=d_y.ptr, w=d_w.ptr, b=d_b.ptr, m=d_m.ptr, ck=d_cg.ptr, e=pe, ne=ne, dbc=16, fi=0, fo=0, wk=d_work.ptr, c=None,
          cnt=1):
        return E.L.crc_conv_slots_bias_mask_forms(c or E.c, x, fi, cnt, ci, gs, T, w, co, b, m, ck, e, ne, dbc, y, fo, wk, None)
    # the new operands: misaligned, inside d_y, d_work or d_x -- each with the other absent too
    for other in (dict(), dict(m=None)):
        assert f(b=d_b.ptr + 8, **other) == -1 and f(b=d_y.ptr, **other) == -1 and f(b=d_y.ptr + Cout * ctb - 16, **other) == -1
        assert f(b=d_work.ptr + 256, **other) == -1 and f(b=d_x.ptr, **other) == -1 and f(b=d_x.ptr + Cin * ctb - 16, **other) == -1
    for other in (dict(), dict(b=None)):
        assert f(m=d_m.ptr + 8, **other) == -1 and f(m=d_y.ptr, **other) == -1 and f(m=d_y.ptr + Cout * ctb - 16, **other) == -1
        assert f(m=d_work.ptr + 256, **other) == -1 and f(m=d_x.ptr, **other) == -1 and f(m=d_x.ptr + ctb, **other) == -1
    # ... and everything crc_conv_slots_forms refuses
    assert f(e=pu(no9), ne=len(no9)) == -1 and f(gs=A(1, 3, 27)) == -1 and f(ne=0) == -1
    assert f(gs=A(1, 2, 9)) == -1 and f(gs=A(2 * n + 1, 3, 9)) == -1 and f(gs=A(0, 3, 9)) == -1 and f(gs=None) == -1
    assert f(T=0) == -1 and f(T=-1) == -1 and f(ci=0) == -1 and f(ci=-1) == -1 and f(co=0) == -1 and f(co=-1) == -1
    assert f(T=1025) == -1 and f(ci=4097) == -1 and f(co=4097) == -1
    assert f(w=d_w.ptr + 8) == -1 and f(w=None) == -1 and f(w=d_y.ptr) == -1 and f(w=d_work.ptr + 256) == -1
    assert f(wk=d_y.ptr) == -1 and f(y=d_work.ptr + 4096) == -1 and f(y=d_x.ptr) == -1 and f(wk=d_x.ptr) == -1 and f(y=d_x.ptr + ctb) == -1
    assert f(x=d_x.ptr + 8) == -1 and f(y=d_y.ptr + 8) == -1 and f(ck=d_cg.ptr + 8) == -1 and f(x=None) == -1 and f(y=None) == -1 and f(wk=None) == -1
    assert f(ck=None) == -1 and f(fi=ca.NTTP) == -1 and f(fo=ca.NTTL) == -1 and f(dbc=0) == -1 and f(dbc=61) == -1
    assert f(c=H.c) == -1                                                                        # a host-only context
    assert f(cnt=0) == 0                                                                         # an empty batch is no error
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    for kw in (dict(), dict(b=None), dict(m=None), dict(b=None, m=None)):                        # ... and the calls they all vary are valid ones
        assert f(**kw) == 0
        assert (E.download(d_y, (Cout * ctb // 8,)) == 0).all()                                  # (of zero ciphertexts, a zero bias and a zero mask)
    assert (E.download(d_y, (d_y.nbytes // 8,))[-8:] == np.uint64(FF)).all()
    E.close(); H.close()
