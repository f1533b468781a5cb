"""The dense layer over channel planes on the GPU: crc_dense_planes_forms against its composed form (crc_multiply_plain_ntt and crc_add over the channels,
crc_rotate_hoisted_forms per step, crc_add over the steps) bit for bit, the batched key switch with one key per step against the key switch per step, the prepared
keys that outlive a call, a planned network through encryption and decryption, and the refusals."""
import numpy as np
import pytest

import conv_slots_model as cm
import dense_planes_model as dm
import galois_model as gm
from test_gpu_galois import Q1, moduli

pytestmark = pytest.mark.gpu
FF = 0xffffffffffffffff
KEYS = ("sq_chunk", "relin_path", "planes_batch")
NTT_FORM = 1                                                            # crcnn_amd.NTT (the package is imported inside the tests)


def reset(E):
    for key in KEYS:
        E.set_tuning(key, 0)


def keyed_case(n, k, t, Cin, count, gs, seed):
    """host engine, conjugated keys for exactly the elements of gs, Cin x count encrypted slot vectors"""
    import crcnn_amd as ca
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(61 + seed)
    need = sorted({int(g) for g in gs} - {1})
    elts, gk = H.gen_galois_keys(62 + seed, sk, elts=need) if need else (np.zeros(0, dtype=np.uint64), np.zeros((0, 1), dtype=np.uint64))
    cg = H.galois_conjugate_keys(elts, gk) if need else gk
    rng = np.random.RandomState(seed)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(Cin * count, n)).astype(np.int64)
    x = H.encrypt(pk, H.slots_compose(v, Cin * count, n, n, 1), 600 + seed)
    return q, H, sk, pk, elts, cg, x


def plain_rows(E, H, R, Cin, n, t, seed):
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, t, size=(R * Cin, n)).astype(np.int64)
    rows[min(Cin, R * Cin - 1)] = 0; rows[0, 5] = t - 1                                   # one all-zero row, one entry t - 1
    d_p = E.alloc(R * Cin * E.k * n * 8)
    E.plain_to_ntt(E.upload(H.slots_compose(rows, R * Cin, n, n, 1)), R * Cin, d_p)
    return d_p


def composed(E, d_xn, count, Cin, gs, d_p, d_cg, elts, d_work, d_tmp, d_u, d_r, d_ref):
    """d_xn [Cin][count] in NTT form -> d_ref [count] in NTT form: per step the products with its rows summed over the channels, its hoisted rotation, the sum"""
    rowb = E.k * E.n * 8; ctb = 2 * rowb
    for j, g in enumerate(gs):
        for c in range(Cin):
            dst = d_u if c == 0 else d_tmp
            E.copy_d2d(dst, d_xn.ptr + c * count * ctb, count * ctb)
            E.multiply_plain_ntt(dst, d_p.ptr + (j * Cin + c) * rowb, count, count)
            if c:
                E.add(d_u, d_tmp, count)
        E.rotate_hoisted(d_u, count, [g], d_cg, elts, d_r, d_work, in_form=NTT_FORM, out_form=NTT_FORM)
        if j == 0:
            E.copy_d2d(d_ref, d_r, count * ctb)
        else:
            E.add(d_ref, d_r, count)


def elements(n, R, one_at=2):
    """R distinct valid elements with the element 1 at index one_at: row rotations while the ring has them, then the column swap and its products"""
    gs = [gm.elt_rows(n, s) for s in range(min(R, n // 2))]
    gs += [g for g in (2 * n - 1, 3 * (2 * n - 1) % (2 * n), 9 * (2 * n - 1) % (2 * n)) if g not in gs][:R - len(gs)]
    assert len(gs) == R and len(set(gs)) == R and all(gm.elt_valid(n, g) for g in gs)
    gs[0], gs[one_at] = gs[one_at], gs[0]                               # (at 2: the unkeyed step splits the keyed ones into two runs)
    return gs


@pytest.mark.parametrize("n,k,Cin,R,counts,chunk,one_at", [(4096, 2, 3, 5, (1, 3), 0, 2), (256, 2, 34, 11, (3,), 8, 2), (256, 2, 34, 11, (3,), 8, 0),
                                                           (256, 2, 34, 12, (3,), 8, 2), (64, 1, 2, 34, (2,), 0, 2)],
                         ids=["n4096_Cin3_R5", "n256_Cin34_R11_passes_and_sub_batches", "n256_Cin34_R11_run_cut_8_2", "n256_Cin34_R12_runs_2_8_1",
                              "n64_R34_two_sum_launches"])
def test_fused_equals_composed(n, k, Cin, R, counts, chunk, one_at):
    """the composed form is built once per count at the default tuning; the fused call must give its bits at planes_batch 1 and 2, on both key-switch paths, for
    the four form pairs, with and without prepared keys.  n = 4096: the wave-local key-switch kernels; count = 1 is the keyed K2's stream (one ciphertext per key,
    two slots per thread), count = 3 its tile of four with one idle.  n = 256 with sq_chunk = 8: 34 channels are two launches of the inner sums, a pass is
    8 . 8 / (34 + 11) = 1 ciphertext per channel (three passes, the keys of pass 0 serving the others), so a sub-batch holds rb = 8 steps: with the element 1 at
    index 2 the 10 keyed steps go as runs of 2 and 8 around it (neither longer than rb); with it first they are ONE run of 10, which the cap rb cuts into 8 and a
    short last sub-batch of 2; R = 12 with it at index 2 gives 2, then a run of 9 cut into 8 + 1.  In the last two the cap is what keeps a sub-batch inside the
    regions sized for rb ch ciphertexts.  n = 64: a workgroup of 64 threads, two launches of the sum kernel"""
    import crcnn_amd as ca
    t = 65537 if n == 4096 else ca.Engine.slots_prime(n, 20)
    gs = elements(n, R, one_at)
    E = ca.Engine(n, moduli(n, k), t, device=0)
    rowb = k * n * 8; ctb = 2 * rowb
    try:
        for count in counts:
            q, H, sk, pk, elts, cg, x = keyed_case(n, k, t, Cin, count, gs, n + R + count)
            d_p = plain_rows(E, H, R, Cin, n, t, n + Cin)
            d_cg = E.upload(cg)
            d_pk = E.galois_prepare_keys(d_cg, elts)
            d_tmp, d_u, d_r, d_ref = (E.alloc(count * ctb) for _ in range(4))
            d_y = E.alloc(count * ctb + 64)
            E.set_tuning("sq_chunk", chunk)
            d_work = E.alloc(max(E.rotate_hoisted_work_bytes(count, 1), E.dense_planes_work_bytes(count, Cin, R), E.dense_planes_work_bytes(count, Cin, R, prepared=True)))
            d_xc = E.upload(x); d_xn = E.upload(x)
            E.ntt_fwd(d_xn, Cin * count)
            composed(E, d_xn, count, Cin, gs, d_p, d_cg, elts, d_work, d_tmp, d_u, d_r, d_ref)
            want = {ca.NTT: E.download(d_ref, (count * ctb // 8,))}
            E.ntt_inv(d_ref, count)
            want[ca.COEFF] = E.download(d_ref, (count * ctb // 8,))
            for fin in (ca.COEFF, ca.NTT):
                d_x = d_xc if fin == ca.COEFF else d_xn
                for fout in (ca.COEFF, ca.NTT):
                    for path in (0, 1):
                        for batch in (1, 2):
                            for pk_given in (False, True):
                                E.set_tuning("relin_path", path); E.set_tuning("planes_batch", batch)
                                E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                                E.dense_planes(d_x, count, Cin, gs, d_p, d_cg, elts, d_y, d_work, d_pk=d_pk if pk_given else None, in_form=fin, out_form=fout)
                                E.set_tuning("relin_path", 0); E.set_tuning("planes_batch", 0)
                                got = E.download(d_y, (count * ctb // 8 + 8,))
                                what = (count, fin, fout, path, batch, pk_given)
                                assert np.array_equal(got[:-8], want[fout]), what
                                assert (got[-8:] == np.uint64(FF)).all(), what + ("wrote past the end",)
            assert np.array_equal(E.download(d_xc, x.shape), x)        # the inputs are only read
            H.close()
    finally:
        reset(E)
    E.close()


def test_keyed_key_switch_equals_the_key_switch_per_step():
    """relin_mac_keyed_f64_kernel against relin_mac_f64_kernel on the same digits: three keyed steps (three keys) and count = 2, 3, 5, 9 -- a tile of two, a tile
    of four with one idle (ciphertexts that share a key beside tiles of the next key), one full tile and a tail of one, two tiles and a tail.  Both settings
    are also held against the composed form, which shares no code with the entry point"""
    import crcnn_amd as ca
    n, k, t, Cin = 4096, 2, 65537, 1
    gs = [gm.elt_rows(n, 1), gm.elt_rows(n, 7), 2 * n - 1]
    E = ca.Engine(n, moduli(n, k), t, device=0)
    ctb = 2 * k * n * 8
    try:
        for count in (2, 3, 5, 9):
            q, H, sk, pk, elts, cg, x = keyed_case(n, k, t, Cin, count, gs, count)
            d_p = plain_rows(E, H, len(gs), Cin, n, t, count)
            d_cg = E.upload(cg); d_x = E.upload(x)
            d_pk = E.galois_prepare_keys(d_cg, elts)
            d_y = E.alloc(count * ctb + 64)
            d_work = E.alloc(max(E.rotate_hoisted_work_bytes(count, 1), E.dense_planes_work_bytes(count, Cin, len(gs), prepared=True)))
            d_xn = E.upload(x); E.ntt_fwd(d_xn, Cin * count)
            d_tmp, d_u, d_r, d_ref = (E.alloc(count * ctb) for _ in range(4))
            composed(E, d_xn, count, Cin, gs, d_p, d_cg, elts, d_work, d_tmp, d_u, d_r, d_ref)
            want = E.download(d_ref, (count * ctb // 8,))
            out = {}
            for batch in (1, 2):
                E.set_tuning("planes_batch", batch)
                E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
                E.dense_planes(d_x, count, Cin, gs, d_p, d_cg, elts, d_y, d_work, d_pk=d_pk, out_form=ca.NTT)
                E.set_tuning("planes_batch", 0)
                out[batch] = E.download(d_y, (count * ctb // 8 + 8,))
            assert np.array_equal(out[1], out[2]), count
            assert np.array_equal(out[2][:-8], want), count
            assert (out[2][-8:] == np.uint64(FF)).all() and out[2][:-8].any()
            H.close()
    finally:
        reset(E)
    E.close()


def test_one_step_of_1_is_the_plain_product():
    """R = 1 with g = 1: no key, no digits -- crc_multiply_plain_ntt summed over the channels"""
    import crcnn_amd as ca
    n, k, t, Cin, count = 4096, 2, 65537, 2, 2
    q, H, sk, pk, elts, cg, x = keyed_case(n, k, t, Cin, count, [1], 3)
    E = ca.Engine(n, q, t, device=0)
    rowb = k * n * 8; ctb = 2 * rowb
    d_p = plain_rows(E, H, 1, Cin, n, t, 4)
    d_xn = E.upload(x); E.ntt_fwd(d_xn, Cin * count)
    d_ref = E.alloc(count * ctb); d_tmp = E.alloc(count * ctb); d_y = E.alloc(count * ctb + 64)
    E.copy_d2d(d_ref, d_xn, count * ctb); E.multiply_plain_ntt(d_ref, d_p, count, count)
    E.copy_d2d(d_tmp, d_xn.ptr + count * ctb, count * ctb); E.multiply_plain_ntt(d_tmp, d_p.ptr + rowb, count, count)
    E.add(d_ref, d_tmp, count)
    d_work = E.alloc(E.dense_planes_work_bytes(count, Cin, 1))
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    E.dense_planes(E.upload(x), count, Cin, [1], d_p, None, [], d_y, d_work, out_form=ca.NTT)
    got = E.download(d_y, (count * ctb // 8 + 8,))
    assert np.array_equal(got[:-8], E.download(d_ref, (count * ctb // 8,))) and (got[-8:] == np.uint64(FF)).all()
    E.close(); H.close()


def test_prepared_keys_are_the_same_words_on_every_call():
    """two calls of crc_galois_prepare_keys_dev leave the same blob (checksum and words); that it is what pass 0 of a call prepares is the equality of the fused
    call's bits with and without d_pk in test_fused_equals_composed"""
    import crcnn_amd as ca
    n, k, t = 4096, 2, 65537
    gs = [gm.elt_rows(n, 1), 2 * n - 1]
    q, H, sk, pk, elts, cg, x = keyed_case(n, k, t, 1, 1, gs, 9)
    E = ca.Engine(n, q, t, device=0)
    words = E.galois_prepared_key_words()
    assert words == 2 * E.L.crc_evk_words(E.c, 16)
    d_cg = E.upload(cg)
    d_a = E.alloc(2 * words * 8 + 64); d_b = E.alloc(2 * words * 8 + 64)
    for d in (d_a, d_b):
        E.L.crc_memset(E.c, d.ptr, 0xff, d.nbytes, E.stream)
        E.galois_prepare_keys(d_cg, elts, d_pk=d)
    a = E.download(d_a, (2 * words + 8,)); b = E.download(d_b, (2 * words + 8,))
    assert E.checksum64(d_a, 2 * words * 8) == E.checksum64(d_b, 2 * words * 8)
    assert np.array_equal(a, b) and (a[-8:] == np.uint64(FF)).all() and not np.array_equal(a[:words], a[words:2 * words])
    assert np.array_equal(E.download(d_cg, cg.shape), cg)
    pu = ca.binding._pu
    e = E._elts(elts)
    d_s = E.alloc(E.L.crc_evk_words(E.c, 16) * 8)
    f = lambda ck=d_cg.ptr, el=pu(e), m=2, dbc=16, o=d_a.ptr, s=d_s.ptr, c=None: E.L.crc_galois_prepare_keys_dev(c or E.c, ck, el, m, dbc, o, s, None)
    assert f(ck=None) == -1 and f(o=None) == -1 and f(s=None) == -1 and f(el=None) == -1 and f(m=-1) == -1 and f(dbc=0) == -1 and f(dbc=61) == -1
    assert f(ck=d_cg.ptr + 8) == -1 and f(o=d_a.ptr + 8) == -1 and f(s=d_s.ptr + 8) == -1 and f(o=d_cg.ptr) == -1 and f(s=d_a.ptr) == -1 and f(s=d_cg.ptr) == -1
    assert f(el=pu(E._elts([1, 3]))) == -1 and f(el=pu(E._elts([2, 3]))) == -1 and f(c=H.c) == -1
    assert f(dbc=40) == -4 and E.galois_prepared_key_words(40) == 0      # 2 digits of 40 bits: beyond the fp64 key switch
    assert f(m=0) == 0 and f() == 0
    assert np.array_equal(E.download(d_a, (2 * words + 8,)), a)
    E.close(); H.close()


def test_planned_network_through_encryption():
    """(4096, 2 moduli, t = 65537), one packed image: a 6 x 6 plane (pitch 8, M = 64) through a 3 x 3 convolution 1 -> 2 with a folded 2 x 2 sum pool (2 x 2
    pixels per plane at slots 0, 2, 16, 18), the dense layer over the two planes to 6 outputs at slots 0 .. 5, and the same entry point at Cin = 1 from that
    vector to 3 outputs at slots 9, 3, 40.  Small weights.  First the parameters: the device's noise budget of the result must be positive (a failure there is a
    parameter choice); then every output slot of every period is the integer network and every other slot is 0"""
    import crcnn_amd as ca
    n, k, t, M, pitch = 4096, 2, 65537, 64, 8
    half = t // 2
    q = moduli(n, k)
    H = ca.Engine(n, q, t, device=-1)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.RandomState(77)
    img = rng.randint(0, 3, size=(1, 6, 6)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64)
    W2 = rng.randint(-2, 3, size=(6, 2, 4)).astype(np.int64)
    W3 = rng.randint(-1, 2, size=(3, 1, 6)).astype(np.int64)
    p1 = E.conv_slots_plan(M, pitch, 6, 6, 3, 3, pool=2)
    assert p1.valid == [0, 2, 16, 18]
    p2 = E.dense_planes_plan(M, p1.valid, 6)
    outs3 = [9, 3, 40]
    p3 = E.dense_planes_plan(M, p2.out_slots, outs3)
    print("steps: conv", len(p1.steps), "dense over planes", len(p2.steps), "dense on the vector", len(p3.steps))
    mid = cm.conv_direct(img, w1, 2)                                    # [2][2][2]
    v2 = dm.dense_direct(W2, mid.reshape(2, 4), t)
    v2 = [(v + half) % t - half for v in v2]
    v3 = [(v + half) % t - half for v in dm.dense_direct(W3, np.array(v2, dtype=object).reshape(1, 6), t)]
    sk, pk = H.keygen(71)
    need = sorted(set(p1.elements + p2.elements + p3.elements) - {1})
    elts, gk = H.gen_galois_keys(72, sk, elts=need)
    d_cg = E.upload(H.galois_conjugate_keys(elts, gk)); d_sk = E.upload(sk)
    d_pk = E.galois_prepare_keys(d_cg, elts)
    print("keys:", len(need), "conjugated", len(need) * E.L.crc_evk_words(E.c, 16) * 8, "bytes, prepared", len(need) * E.galois_prepared_key_words() * 8, "bytes")
    plane = cm.plane_slots(img[0], n, M, pitch, 1).astype(np.int64)
    d_x = E.upload(H.encrypt(pk, H.slots_compose(plane, 1, n, n, 1), 73))
    rowb = k * n * 8; ctb = 2 * rowb
    d_w1 = E.upload(H.conv_slots_pack_weights(p1.fold(w1, t)))

    def rows_of(plan, W):
        r = plan.fold(W, t)
        d = E.alloc(r.shape[0] * r.shape[1] * rowb)
        E.plain_to_ntt(E.upload(H.slots_compose(r.reshape(-1, n), r.shape[0] * r.shape[1], n, n, 1)), r.shape[0] * r.shape[1], d)
        return d
    d_p2, d_p3 = rows_of(p2, W2), rows_of(p3, W3)
    d_m = E.alloc(2 * ctb); d_v = E.alloc(ctb); d_y = E.alloc(ctb)
    d_work = E.alloc(max(E.conv_slots_work_bytes(1, 1, 2, len(p1.steps)), E.dense_planes_work_bytes(1, 2, len(p2.steps), prepared=True),
                         E.dense_planes_work_bytes(1, 1, len(p3.steps), prepared=True)))
    E.conv_slots(d_x, 1, 1, p1.elements, d_w1, 2, d_cg, elts, d_m, d_work)
    E.dense_planes(d_m, 1, 2, p2.elements, d_p2, d_cg, elts, d_v, d_work, d_pk=d_pk)
    E.dense_planes(d_v, 1, 1, p3.elements, d_p3, d_cg, elts, d_y, d_work, d_pk=d_pk)
    d_bits = E.alloc(4); d_bw = E.alloc(E.noise_budget_dev_work_bytes(1))
    E.noise_budget_dev(d_sk, d_y, 1, d_bits, d_bw)
    budget = int(E.download(d_bits, (1,), dtype=np.int32)[0])
    print("noise budget of the network's result:", budget)
    assert budget > 0, "the parameters leave no noise budget: choose others"
    d_pl = E.alloc(n * 8); d_o = E.alloc(n * 8); d_dw = E.alloc(E.decrypt_dev_work_bytes(1))

    def slots(d_ct):
        E.decrypt_dev(d_sk, d_ct, 1, d_pl, d_dw)
        E.slots_decompose_dev(d_pl, 1, n, d_o, n, 1)
        return [int(v) for v in E.download(d_o, (1, n), dtype=np.int64)[0]]
    expect2 = [0] * M
    for o, s in enumerate(p2.out_slots):
        expect2[s] = v2[o]
    assert slots(d_v) == expect2 * (n // M)
    expect3 = [0] * M
    for o, s in enumerate(outs3):
        expect3[s] = v3[o]
    assert slots(d_y) == expect3 * (n // M)
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
    Cin, R = 2, 3
    d_x = E.alloc(Cin * ctb + 64); d_y = E.alloc(ctb + 64); d_cg = E.upload(cg); d_p = E.alloc(R * Cin * n * 8 + 64)
    d_pk = E.galois_prepare_keys(d_cg, elts)
    d_work = E.alloc(max(E.dense_planes_work_bytes(1, Cin, R), E.dense_planes_work_bytes(1, Cin, R, prepared=True)))
    E.L.crc_memset(E.c, d_x.ptr, 0, d_x.nbytes, E.stream); E.L.crc_memset(E.c, d_p.ptr, 0, d_p.nbytes, E.stream)
    E.L.crc_memset(E.c, d_y.ptr, 0xff, d_y.nbytes, E.stream)
    pe = pu(elts); ne = len(elts)
    no9 = np.ascontiguousarray(elts[elts != 9])
    A = lambda *g: pu(E._elts(list(g)))

    def f(gs=A(1, 3, 9), R=R, ci=Cin, x=d_x.ptr, y=d_y.ptr, p=d_p.ptr, ck=d_cg.ptr, e=pe, m=ne, pk=None, dbc=16, fi=0, fo=0, wk=d_work.ptr, c=None, cnt=1):
        return E.L.crc_dense_planes_forms(c or E.c, x, fi, cnt, ci, gs, R, p, ck, e, m, pk, dbc, y, fo, wk, None)
    assert f(e=pu(no9), m=len(no9)) == -1 and f(gs=A(1, 3, 27)) == -1 and f(m=0) == -1          # a missing conjugated key
    assert f(pk=d_pk.ptr, m=0) == -1                                                             # prepared keys of an empty set while a step is keyed
    assert f(gs=A(1, 2, 9)) == -1 and f(gs=A(2 * n + 1, 3, 9)) == -1 and f(gs=A(0, 3, 9)) == -1 and f(gs=None) == -1   # an invalid element
    assert f(R=0) == -1 and f(R=-1) == -1 and f(ci=0) == -1 and f(ci=-1) == -1 and f(ci=4097) == -1 and f(R=65537) == -1
    assert f(p=d_p.ptr + 8) == -1 and f(p=None) == -1                                            # a misaligned or absent d_p_ntt
    assert f(p=d_y.ptr) == -1 and f(p=d_work.ptr + 256) == -1 and f(p=d_x.ptr) == -1            # d_p_ntt inside d_y, d_work or d_x
    assert f(pk=d_pk.ptr + 8) == -1 and f(pk=d_y.ptr) == -1 and f(pk=d_x.ptr) == -1 and f(pk=d_p.ptr) == -1 and f(pk=d_work.ptr + 512) == -1
    assert f(wk=d_y.ptr) == -1 and f(y=d_work.ptr + 4096) == -1 and f(y=d_x.ptr) == -1 and f(wk=d_x.ptr) == -1
    assert f(y=d_x.ptr + ctb) == -1                                                              # d_y over the second input channel
    assert f(x=d_x.ptr + 8) == -1 and f(y=d_y.ptr + 8) == -1 and f(ck=d_cg.ptr + 8) == -1 and f(x=None) == -1 and f(y=None) == -1 and f(wk=None) == -1
    assert f(ck=None) == -1 and f(fi=ca.NTTP) == -1 and f(fo=ca.NTTL) == -1 and f(dbc=0) == -1 and f(dbc=61) == -1
    assert f(c=H.c) == -1                                                                        # a host-only context
    assert f(cnt=0) == 0                                                                         # an empty batch is no error
    assert (E.download(d_y, (d_y.nbytes // 8,)) == np.uint64(FF)).all()
    assert f() == 0 and f(pk=d_pk.ptr) == 0                                                      # ... and the call they all vary is a valid one
    assert (E.download(d_y, (ctb // 8,)) == 0).all()                                             # (of zero ciphertexts)
    assert (E.download(d_y, (d_y.nbytes // 8,))[-8:] == np.uint64(FF)).all()
    E.close(); H.close()
