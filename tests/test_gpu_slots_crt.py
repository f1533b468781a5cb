"""Slot batching over several plain moduli on the GPU: slots_crt_decompose_kernel and slots_crt_act_kernel (crc_slots_crt_decompose_dev / crc_slots_crt_act_dev) bit
for bit against their host twins -- which tests/test_slots_crt_cpu.py holds against the integer model --, crc_slots_crt_refresh[_sym]_dev_key against the public
calls it is defined as, and a small network whose integers no single modulus could carry, end to end against Python integers."""
import numpy as np
import pytest

import slots_crt_model as cm
from test_gpu_slots_rescale import DIVISORS, GUARD, Q1, Q2
from test_slots_crt_cpu import make_base, close, rows_for

pytestmark = pytest.mark.gpu
ALL_ONES = np.uint64(0xffffffffffffffff)
KEY = bytes(range(7, 39))


def kernel_cases():
    """every pass structure of the row transform and both lane shares (4 pairs up to n = 8192, 8 at 16384); r = 3 twenty-bit primes up to n = 4096, r = 2
    thirty-one-bit primes above; the r = 4 base and the base of unequal sizes at n = 256"""
    import crcnn_amd as ca
    P = ca.SlotsCrt.primes
    return [(64, P(64, 3, 20)), (256, P(256, 3, 20)), (256, [15361, 13313, 12289, 11777]), (256, [ca.Engine.slots_prime(256, 40), 7681]), (2048, P(2048, 3, 20)),
            (4096, P(4096, 3, 20)), (8192, P(8192, 2, 31)), (16384, P(16384, 2, 31))]


def guarded(E, words):
    d = E.alloc((words + GUARD) * 8)
    E.L.crc_memset(E.c, d.ptr, 0xff, (words + GUARD) * 8, E.stream)
    return d


@pytest.mark.parametrize("case", range(8))
def test_device_kernels_equal_the_host_twins(case):
    n, ts = kernel_cases()[case]
    B, H = make_base(n, ts, device=0), make_base(n, ts)
    assert B.supported and H.supported
    E, r = B.E[0], B.r
    half = (B.T - 1) // 2
    cap = min(1000, half)
    for D in [d for d in DIVISORS if d <= half]:
        rows, _ = rows_for(H, D, 17, 13 * n + D % 1000)
        want_v = H.decompose(rows, n, n, 1).reshape(17, n)
        want_a = {(relu, c): H.act(rows, D, relu, c) for relu, c in ((0, 0), (1, cap))}
        for count in (3, 17):                                  # 17 crosses one XCD group of 16
            words = count * n
            d_in = [E.upload(rows[j, :count]) for j in range(r)]
            # decompose: item-major with all slots, image-major with fewer slots than n
            d_v = guarded(E, words)
            B.decompose_dev(d_in, count, n, d_v, n, 1)
            got = E.download(d_v, (words + GUARD,), dtype=np.int64)
            assert np.array_equal(got[:words].reshape(count, n), want_v[:count]), (n, ts, D, count, "item-major")
            assert (got[words:] == -1).all(), (n, ts, D, count, "guard words")
            part = n - 5
            d_v = guarded(E, part * count)
            B.decompose_dev(d_in, count, part, d_v, 1, count)
            got = E.download(d_v, (part * count + GUARD,), dtype=np.int64)
            assert np.array_equal(got[:part * count].reshape(part, count).T, want_v[:count, :part]), (n, ts, D, count, "image-major")
            assert (got[part * count:] == -1).all(), (n, ts, D, count, "guard words")
            # the activation: out of place with guards, the inputs untouched; in place
            for (relu, c), want in want_a.items():
                d_out = [guarded(E, words) for _ in range(r)]
                B.act_dev(d_in, count, D, relu, c, d_out)
                for j in range(r):
                    got = E.download(d_out[j], (words + GUARD,))
                    assert np.array_equal(got[:words].reshape(count, n), want[j, :count]), (n, ts, D, count, relu, c, j, "out of place")
                    assert (got[words:] == ALL_ONES).all(), (n, ts, D, count, j, "guard words")
                    assert np.array_equal(E.download(d_in[j], (count, n)), rows[j, :count]), (n, ts, D, count, j, "an input was written")
            d_io = [E.upload(rows[j, :count]) for j in range(r)]
            B.act_dev(d_io, count, D, 1, cap, d_io)
            for j in range(r):
                assert np.array_equal(E.download(d_io[j], (count, n)), want_a[(1, cap)][j, :count]), (n, ts, D, count, j, "in place")
    close(B); close(H)


def test_one_modulus_is_the_existing_device_calls():
    """r = 1: crc_slots_decompose_dev and crc_slots_act_dev on a 1 x 1 window, to the bit, at a lazy and at a strict modulus and both lane shares"""
    import crcnn_amd as ca
    for n, bits in ((256, 60), (2048, 30), (16384, 60)):
        t = ca.Engine.slots_prime(n, bits)
        B = make_base(n, [t], device=0)
        E = B.E[0]
        count = 5
        rows, _ = rows_for(make_base(n, [t]), 1 << 7, count, n)
        d_in = E.upload(rows[0])
        d_a, d_b = E.alloc(count * n * 8), E.alloc(count * n * 8)
        B.decompose_dev([d_in], count, n, d_a, n, 1); E.slots_decompose_dev(d_in, count, n, d_b, n, 1)
        assert np.array_equal(E.download(d_a, (count, n), dtype=np.int64), E.download(d_b, (count, n), dtype=np.int64))
        for relu, cap in ((0, 0), (1, 50)):
            B.act_dev([d_in], count, 1 << 7, relu, cap, [d_a]); E.slots_act_dev(d_in, count, (1, 1, 1, 1, 1, 1), 1 << 7, relu, cap, d_b)
            assert np.array_equal(E.download(d_a, (count, n)), E.download(d_b, (count, n))), (n, t, relu, cap)
        close(B)


def test_device_refusals():
    import ctypes
    import crcnn_amd as ca
    n = 2048
    VP = ctypes.c_void_p
    ts = ca.SlotsCrt.primes(n, 3, 20)
    B = make_base(n, ts, device=0)
    E, L = B.E[0], B.L
    nos = ca.Engine(n, Q1, 1 << 20, device=0)
    count = 2
    d = [E.alloc(count * n * 8 + 16) for _ in range(3)]; o = [E.alloc(count * n * 8 + 16) for _ in range(3)]
    for x in d + o:
        E.L.crc_memset(E.c, x.ptr, 0, count * n * 8 + 16, E.stream)
    arr = lambda es: (VP * len(es))(*[e.c if e is not None else None for e in es])
    ptr = lambda ps: (VP * len(ps))(*ps)
    pd, po = [x.ptr for x in d], [x.ptr for x in o]
    act = lambda es, r, i=pd, out=po, D=3, relu=0, cap=0, cnt=count: L.crc_slots_crt_act_dev(arr(es), r, ptr(i), cnt, D, relu, cap, ptr(out), None)
    dec = lambda es, r, i=pd, v=po[0], slots=n, ist=n, sst=1, cnt=count: L.crc_slots_crt_decompose_dev(arr(es), r, ptr(i), cnt, slots, v, ist, sst, None)
    assert act(B.E, 0) == -1 and act(B.E + [nos], 5, i=pd + [pd[0]], out=po + [po[0]]) == -1 and act([B.E[0], None, B.E[2]], 3) == -1
    assert act([B.E[0], nos, B.E[2]], 3) == -2 and act([B.E[0], B.E[0], B.E[2]], 3, D=0) == -2 and dec([B.E[0], nos, B.E[2]], 3, slots=0) == -2
    assert act(B.E, 3, D=0) == -1 and act(B.E, 3, D=(1 << 62) + 1) == -1 and act(B.E, 3, relu=2) == -1 and act(B.E, 3, cap=(B.T - 1) // 2 + 1) == -1
    assert act(B.E, 3, i=[pd[0] + 8, pd[1], pd[2]]) == -1 and act(B.E, 3, out=[po[0], po[1] + 8, po[2]]) == -1 and act(B.E, 3, out=[po[0], None, po[2]]) == -1
    assert act(B.E, 3, out=[pd[1], pd[0], po[2]]) == -1 and act(B.E, 3, out=[po[0], po[0], po[2]]) == -1 and act(B.E, 3, out=[pd[0] + 16, po[1], po[2]]) == -1
    assert dec(B.E, 3, slots=0) == -1 and dec(B.E, 3, slots=n + 1) == -1 and dec(B.E, 3, ist=0) == -1 and dec(B.E, 3, sst=0) == -1 and dec(B.E, 3, v=None) == -1
    assert dec(B.E, 3, i=[pd[0], pd[1] + 8, pd[2]]) == -1 and dec(B.E, 3, v=po[0] + 4) == -1
    assert all(not E.download(x, (count * n + 2,)).any() for x in o)                     # nothing was written
    assert act(B.E, 3, cnt=0) == 0 and dec(B.E, 3, cnt=0) == 0 and not E.download(o[0], (count * n,)).any()
    assert act(B.E, 3, D=1 << 62, relu=1, cap=(B.T - 1) // 2) == 0 and act(B.E, 3, out=pd) == 0 and dec(B.E, 3) == 0
    f = L.crc_slots_crt_refresh_sym_dev_key
    key = ca.Engine._key(KEY)
    assert f(arr(B.E), 3, pd[0], ptr(pd), 1, ca.COEFF, 0, 0, 0, key, 0, ca.COEFF, ptr(po), po[0], None) == -1
    assert f(arr(B.E), 3, pd[0], ptr(pd), 1, ca.NTTP, 3, 0, 0, key, 0, ca.COEFF, ptr(po), po[0], None) == -1
    assert f(arr(B.E), 3, pd[0], ptr(pd), 1, ca.COEFF, 3, 0, 0, None, 0, ca.COEFF, ptr(po), po[0], None) == -1
    assert f(arr([B.E[0], nos]), 2, pd[0], ptr(pd), 1, ca.COEFF, 0, 0, 0, key, 0, ca.COEFF, ptr(po), po[0], None) == -2
    assert f(arr(B.E), 3, pd[0], ptr(pd), 0, ca.COEFF, 3, 0, 0, key, 0, ca.COEFF, ptr(po), po[0], None) == 0
    nos.close(); close(B)


# ---- the refresh ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2048, 4096], ids=lambda n: f"n{n}")
def pset(request):
    import crcnn_amd as ca
    n = request.param
    ts = ca.SlotsCrt.primes(n, 3, 20)
    B = make_base(n, ts, device=0, q=Q2)
    E = B.E[0]
    sk, pk = E.keygen(5)                                       # the keys do not involve t: one set serves all r engines
    count, D, cap = 5, 1 << 8, 3000
    half = (B.T - 1) // 2
    rng = np.random.RandomState(n)
    v = (rng.randint(0, 1 << 62, size=(count, n), dtype=np.int64) % (2 * half + 1) - half).astype(np.int64)
    v[0, :8] = [half, -half, 0, D // 2, -(D // 2), cap * D, (cap + 1) * D, -3 * (D // 2)]
    d_v = E.upload(v)
    d_pl = [E.alloc(count * n * 8) for _ in range(3)]
    B.compose_dev(d_v, count, n, n, 1, d_pl)
    d_pk = E.upload(pk)
    cts = []
    for j, e in enumerate(B.E):
        d_ct = E.alloc(count * 2 * e.k * n * 8)
        e.encrypt_dev_forms(d_pk, d_pl[j], count, 99 + j, ca.COEFF, d_ct, E.alloc(e.encrypt_dev_work_bytes(count)))
        cts.append(e.download(d_ct, (count, 2, e.k, n)))
    yield dict(n=n, B=B, E=E, sk=sk, pk=pk, count=count, D=D, cap=cap, v=v, ct=cts, d_sk=E.upload(sk), d_pk=d_pk)
    close(B)


def _composed(P, ct_in, fin, fout, sym, base, relu, cap):
    """crc_decrypt_dev on every engine -> crc_slots_crt_act_dev -> crc_encrypt[_sym]_dev_key_forms on every engine with stream base base + j count"""
    B, E, count, n = P["B"], P["E"], P["count"], P["n"]
    d_pl = [E.alloc(count * n * 8) for _ in range(B.r)]
    for j, e in enumerate(B.E):
        e.decrypt_dev(P["d_sk"], E.upload(ct_in[j]), count, d_pl[j], E.alloc(e.decrypt_dev_work_bytes(count, 2, fin)), in_form=fin)
    B.act_dev(d_pl, count, P["D"], relu, cap, d_pl)
    out = []
    for j, e in enumerate(B.E):
        d_out = E.alloc(count * 2 * e.k * n * 8)
        if sym:
            e.encrypt_sym_dev_key_forms(P["d_sk"], d_pl[j], count, KEY, base + j * count, fout, d_out, E.alloc(e.encrypt_sym_dev_work_bytes(count)))
        else:
            e.encrypt_dev_key_forms(P["d_pk"], d_pl[j], count, KEY, base + j * count, fout, d_out, E.alloc(e.encrypt_dev_work_bytes(count)))
        out.append(e.download(d_out, (count, 2, e.k, n)))
    return out


def _refresh(P, ct_in, fin, fout, sym, base, relu, cap, in_place=False):
    B, E, count, n = P["B"], P["E"], P["count"], P["n"]
    d_in = [E.upload(c) for c in ct_in]
    d_out = d_in if in_place else [E.alloc(count * 2 * E.k * n * 8) for _ in range(B.r)]
    d_work = E.alloc(B.refresh_dev_work_bytes(count, fin))
    if sym:
        B.refresh_sym_dev(P["d_sk"], d_in, count, P["D"], relu, cap, KEY, base, d_out, d_work, in_form=fin, out_form=fout)
    else:
        B.refresh_dev(P["d_sk"], P["d_pk"], d_in, count, P["D"], relu, cap, KEY, base, d_out, d_work, in_form=fin, out_form=fout)
    return [E.download(d, (count, 2, E.k, n)) for d in d_out]


@pytest.mark.parametrize("sym", [False, True], ids=["public_key", "secret_key"])
def test_refresh_is_the_public_calls(pset, sym):
    import crcnn_amd as ca
    P = pset
    B, E, n, count, D, cap = P["B"], P["E"], P["n"], P["count"], P["D"], P["cap"]
    ntt = []
    for c in P["ct"]:
        d = E.upload(c); E.ntt_fwd(d, count); ntt.append(E.download(d, c.shape))
    forms = {ca.COEFF: P["ct"], ca.NTT: ntt}
    eq = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    for f in (ca.COEFF, ca.NTT):                               # COEFF -> COEFF and NTT -> NTT
        want = _composed(P, forms[f], f, f, sym, 77, 1, cap)
        assert eq(_refresh(P, forms[f], f, f, sym, 77, 1, cap), want), (f, "out of place")
        assert eq(_refresh(P, forms[f], f, f, sym, 77, 1, cap, in_place=True), want), (f, "d_ct_out[j] == d_ct_in[j]")
        assert not eq(_refresh(P, forms[f], f, f, sym, 78, 1, cap), want)                # another stream base, other ciphertexts
    # what the refreshed ciphertexts decrypt to: the model's integers in every slot
    for relu, c in ((1, cap), (0, 0)):
        got_ct = _refresh(P, P["ct"], ca.COEFF, ca.COEFF, sym, 7, relu, c)
        d_pl = [E.alloc(count * n * 8) for _ in range(B.r)]
        for j, e in enumerate(B.E):
            e.decrypt_dev(P["d_sk"], E.upload(got_ct[j]), count, d_pl[j], E.alloc(e.decrypt_dev_work_bytes(count)))
        d_v = E.alloc(count * n * 8)
        B.decompose_dev(d_pl, count, n, d_v, n, 1)
        got = E.download(d_v, (count, n), dtype=np.int64)
        assert got.tolist() == [[cm.act_value(int(x), D, relu, c) for x in row] for row in P["v"]]
        assert (got.min() == 0 and got.max() == cap) if relu else got.min() < 0


def test_one_modulus_refresh_is_the_existing_call(pset):
    """r = 1: crc_slots_refresh_act[_sym]_dev_key on a 1 x 1 window, to the bit"""
    import crcnn_amd as ca
    P = pset
    E, n, count, D, cap = P["E"], P["n"], P["count"], P["D"], 100
    one = ca.SlotsCrt([E])
    for sym in (False, True):
        d_a, d_b = E.alloc(count * 2 * E.k * n * 8), E.alloc(count * 2 * E.k * n * 8)
        d_in = E.upload(P["ct"][0])
        if sym:
            one.refresh_sym_dev(P["d_sk"], [d_in], count, D, 1, cap, KEY, 5, [d_a], E.alloc(one.refresh_dev_work_bytes(count)))
            E.slots_refresh_act_sym_dev(P["d_sk"], d_in, count, (1, 1, 1, 1, 1, 1), D, 1, cap, 0, d_b, E.alloc(E.slots_refresh_act_sym_dev_work_bytes(count, (1, 1, 1, 1, 1, 1))),
                                        key=KEY, stream_base=5)
        else:
            one.refresh_dev(P["d_sk"], P["d_pk"], [d_in], count, D, 1, cap, KEY, 5, [d_a], E.alloc(one.refresh_dev_work_bytes(count)))
            E.slots_refresh_act_dev(P["d_sk"], P["d_pk"], d_in, count, (1, 1, 1, 1, 1, 1), D, 1, cap, 0, d_b, E.alloc(E.slots_refresh_act_dev_work_bytes(count, (1, 1, 1, 1, 1, 1))),
                                    key=KEY, stream_base=5)
        assert np.array_equal(E.download(d_a, (count, 2, E.k, n)), E.download(d_b, (count, 2, E.k, n))), sym


# ---- host classes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 1])
def test_host_classes_over_a_plain_base(r):
    """test_host plain_base: encryptImageSlotsCrt -> decryptSlotsCrt gives the pixels mod T, rescaleSlotsCrt under either key the model's integers, member 0 is a
    tensor of the global context holding the residues mod t_0, one modulus is encryptImageSlots -> decryptSlots, a stale base is refused"""
    import os
    import subprocess
    import crcnn_amd as ca
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, S, D, cap = 2048, 5, 1 << 8, 1 << 30
    ts = ca.SlotsCrt.primes(n, 3, 20)[:r]
    T = cm.product(ts)
    half = (T - 1) // 2
    cap = min(cap, half)
    out = subprocess.run([os.path.join(root, "crcnn_amd", "lib", "test_host"), "plain_base", str(n), str(S), str(D), str(cap)] + [str(t) for t in ts],
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    images = [[(4 * s + p) * 0x9E3779B97F4A7C15 % (1 << 64) % T - half for p in range(4)] for s in range(S)]
    images[0] = [half, -half, 0, D // 2]
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if len(w) == 6:
            got.setdefault(w[0], []).append([int(x) for x in w[2:]])
    assert got["lifted"] == images
    want = [[cm.act_value(v, D, 1, cap) for v in im] for im in images]
    assert got["act"] == want and got["sym"] == want and got["back"] == want
    assert got["rescale"] == [[cm.act_value(v, D) for v in im] for im in images]
    assert got["part0"] == [[cm.centre(v, ts[0]) for v in im] for im in want]
    assert max(max(im) for im in want) > (max(ts) - 1) // 2 or r == 1
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines() if " " in l)
    assert lines["one_modulus_equal"] == "1" and int(lines["budget"]) > 0
    assert lines["plain_base"] == f"ok refused {7 if r > 1 else 6}"


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------------
def _const_rows(w, q, n):
    """integer weights [out][in] -> constant NTT rows [out][in][k][n]"""
    out = np.empty(w.shape + (len(q), n), dtype=np.uint64)
    for i, qi in enumerate(q):
        out[..., i, :] = np.array([[int(x) % qi for x in row] for row in w], dtype=np.uint64)[..., None]
    return out


def test_a_network_no_single_modulus_could_carry():
    """64 images in the slots; 4 pixels of 4 bits -> dense 4 -> 4, |w| <= 31 -> square + relinearise -> CRT refresh (D = 2^8, relu) -> dense 4 -> 2 -> square +
    relinearise -> CRT decompose, on r = 3 engines through the existing Engine calls: the integers are the Python-integer network's, and both in front of the
    refresh and at the output some of them lie outside every single modulus' range"""
    import crcnn_amd as ca
    n, S, D = 2048, 64, 1 << 8
    ts = ca.SlotsCrt.primes(n, 3, 20)
    B = make_base(n, ts, device=0, q=Q2)
    E = B.E[0]
    q = [int(x) for x in E.q]
    sk, pk = E.keygen(11)
    evk = E.gen_evk(12, sk)
    d_sk, d_pk, d_evk = E.upload(sk), E.upload(pk), E.upload(evk)
    rng = np.random.RandomState(3)
    x = rng.randint(0, 16, size=(4, S)).astype(np.int64); x[:, 0] = 15          # pixel-major: item = pixel, slot = image
    W1 = rng.randint(-31, 32, size=(4, 4)).astype(np.int64); W1[0] = 31
    W2 = rng.randint(-31, 32, size=(2, 4)).astype(np.int64); W2[0] = 31
    # the Python-integer network
    h1 = [[sum(int(W1[o, i]) * int(x[i, s]) for i in range(4)) ** 2 for s in range(S)] for o in range(4)]
    h2 = [[cm.act_value(v, D, 1, 0) for v in row] for row in h1]
    want = [[sum(int(W2[o, i]) * h2[i][s] for i in range(4)) ** 2 for s in range(S)] for o in range(2)]
    single = (max(ts) - 1) // 2
    assert max(max(r) for r in h1) > single and max(max(r) for r in want) > single and max(max(r) for r in want) < (B.T - 1) // 2
    print("largest integer in front of the refresh", max(max(r) for r in h1), "at the output", max(max(r) for r in want), "largest (t_j - 1) / 2", single)
    d_x = E.upload(x)
    d_w1, d_w2 = E.upload(_const_rows(W1, q, n)), E.upload(_const_rows(W2, q, n))
    d_zero = E.upload(np.zeros((4, E.k, n), dtype=np.uint64))
    ctb = 2 * E.k * n * 8
    mid, fin, budgets = [], [], []
    d_bits = E.alloc(4 * 4)
    for j, e in enumerate(B.E):
        d_pl = E.alloc(4 * n * 8)
        e.slots_compose_dev(d_x, 4, S, S, 1, d_pl)
        d_ct = E.alloc(4 * ctb)
        e.encrypt_dev_forms(d_pk, d_pl, 4, 40 + j, ca.NTT, d_ct, E.alloc(e.encrypt_dev_work_bytes(4)))
        d_y = E.alloc(4 * ctb)
        e.dense(d_ct, d_w1, d_zero, 1, 4, 4, ca.NTT, ca.NTT, d_y, E.alloc(e.dense_work_bytes(1, 4, 4, ca.NTT)))
        d_s = E.alloc(4 * ctb)
        e.square_relin(d_y, 4, d_evk, d_s, E.alloc(e.square_relin_work_bytes(4)), in_form=ca.NTT, out_form=ca.NTT)
        e.noise_budget_dev(d_sk, d_s, 4, d_bits, E.alloc(e.noise_budget_dev_work_bytes(4, 2, ca.NTT)), in_form=ca.NTT)
        budgets.append(E.download(d_bits, (4,), dtype=np.int32).tolist())
        mid.append(d_s)
    B.refresh_dev(d_sk, d_pk, mid, 4, D, 1, 0, KEY, 0, mid, E.alloc(B.refresh_dev_work_bytes(4, ca.NTT)), in_form=ca.NTT, out_form=ca.NTT)
    for j, e in enumerate(B.E):
        d_y = E.alloc(2 * ctb)
        e.dense(mid[j], d_w2, d_zero, 1, 4, 2, ca.NTT, ca.NTT, d_y, E.alloc(e.dense_work_bytes(1, 4, 2, ca.NTT)))
        d_s = E.alloc(2 * ctb)
        e.square_relin(d_y, 2, d_evk, d_s, E.alloc(e.square_relin_work_bytes(2)), in_form=ca.NTT, out_form=ca.COEFF)
        e.noise_budget_dev(d_sk, d_s, 2, d_bits, E.alloc(e.noise_budget_dev_work_bytes(2)))
        budgets.append(E.download(d_bits, (2,), dtype=np.int32).tolist())
        d_pl = E.alloc(2 * n * 8)
        e.decrypt_dev(d_sk, d_s, 2, d_pl, E.alloc(e.decrypt_dev_work_bytes(2)))
        fin.append(d_pl)
    print("noise budget in front of the refresh", budgets[:3], "at the output", budgets[3:])
    assert min(min(b) for b in budgets) > 0
    d_v = E.alloc(2 * S * 8)
    B.decompose_dev(fin, 2, S, d_v, S, 1)
    assert E.download(d_v, (2, S), dtype=np.int64).tolist() == want
    close(B)
