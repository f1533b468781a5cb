"""Modulus switching on the GPU: crc_mod_switch_forms bit for bit against its host twin and against tests/mod_switch_model.py for every form pair, both sizes
and every ring size's row transform; a computation that goes on at the lower level (evaluation key generated there from the prefix secret key); and a switch on a
stream of the caller's own."""
import ctypes

import numpy as np
import pytest

import mod_switch_model as mm

pytestmark = pytest.mark.gpu
COEFF, NTT = 0, 1
SMALL = [0xffffe80001, 0xffffc40001, 0xffffffffffc0001]          # the moduli of the ops_n256_* goldens below 2^41, and the 60-bit one
T = 65537
GUARD = 8
FILL = 0xffffffffffffffff
COUNT = 3


def default_primes(n, k):
    """k primes of crc_default_coeff_modulus_128: this ring's own, then those of the larger rings (1 mod 2 n as well)"""
    import crcnn_amd as ca
    out = []
    for m in (n, 8192, 16384):
        if m >= max(n, 1024):
            out += [p for p in ca.default_coeff_modulus_128(m) if p not in out]
    assert len(out) >= k
    return out[:k]


CASES = [("n256_3to2", 256, SMALL, 2), ("n256_3to1", 256, SMALL, 1), ("n256_2to1", 256, SMALL[:2], 1), ("n4096_3to2", 4096, 3, 2), ("n4096_3to1", 4096, 3, 1),
         ("n8192_5to3", 8192, 5, 3), ("n16384_4to3", 16384, 4, 3)]


def inputs(q, n, size, seed):
    """random canonical residues; ciphertext 0: polynomial 0 all zero, polynomial 1 every residue q_i - 1 (composes to q - 1, which rounds to q_to = 0);
    ciphertext 1, polynomial 0: the last residue runs over {0, h, h + 1, p - 1 - h, p - 1}"""
    rng = np.random.RandomState(seed)
    k = len(q)
    x = np.zeros((COUNT, size, k, n), dtype=np.uint64)
    for i, qi in enumerate(q):
        x[:, :, i, :] = (rng.randint(0, 1 << 62, size=(COUNT, size, n), dtype=np.int64) % qi).astype(np.uint64)
    x[0, 0] = 0
    for i, qi in enumerate(q):
        x[0, 1, i, :] = qi - 1
    p = q[-1]; h = p >> 1
    x[1, 0, k - 1, :] = np.resize(np.array([0, h, h + 1, p - 1 - h, p - 1], dtype=np.uint64), n)
    return x


def model_columns(x, q, kept, cols):
    """the definition (CRT composition, iterated rounded division) on the chosen coefficient positions of a coefficient-form tensor"""
    out = np.zeros(x.shape[:2] + (kept, len(cols)), dtype=np.uint64)
    for c in range(x.shape[0]):
        for p in range(x.shape[1]):
            rows = [[int(x[c, p, i, s]) for s in cols] for i in range(len(q))]
            out[c, p] = np.array(mm.switch_rows(rows, q, kept), dtype=np.uint64)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_the_host_twin_and_the_model(case):
    import crcnn_amd as ca
    _, n, q, kept = case
    q = default_primes(n, q) if isinstance(q, int) else q
    A = ca.Engine(n, q, T, device=0); B = A.level(kept)
    assert A.mod_switch_supported(B) and B.k == kept and B.device == A.device
    cols = list(range(n))
    for size in (2, 3):
        x = inputs(q, n, size, 17 * size + n + kept)
        d_x = A.upload(x)
        # coefficient form of x taken as an NTT-form tensor, by the row transform this ring has had all along
        d_t = A.upload(x); A.ntt_inv(d_t, COUNT, size); x_inv = A.download(d_t, x.shape)
        twin = A.mod_switch(B, x, size=size)
        assert np.array_equal(twin[..., cols], model_columns(x, q, kept, cols)), (case, size, "host twin against the model")
        assert not twin[0, :2].any()
        twin_inv = A.mod_switch(B, x_inv, size=size)
        assert np.array_equal(twin_inv[..., cols], model_columns(x_inv, q, kept, cols)), (case, size, "host twin against the model, transformed input")
        words = COUNT * size * kept * n
        for in_form in (COEFF, NTT):
            for out_form in (COEFF, NTT):
                want = A.mod_switch(B, x, size=size, in_form=in_form, out_form=out_form)
                # ... which is the model between the existing transforms: inverse on A in front, forward on B behind
                ref = twin_inv if in_form == NTT else twin
                if out_form == NTT:
                    d_r = B.upload(ref); B.ntt_fwd(d_r, COUNT, size); ref = B.download(d_r, ref.shape)
                assert np.array_equal(want, ref), (case, size, in_form, out_form, "host twin against the model around the device transforms")
                wb = A.mod_switch_work_bytes(B, COUNT, size=size, in_form=in_form, out_form=out_form)
                assert wb >= 256
                d_w = A.alloc(wb)
                d_o = A.alloc((words + GUARD) * 8); A.L.crc_memset(A.c, d_o.ptr, 0xff, (words + GUARD) * 8, A.stream)
                A.mod_switch_dev(B, d_x, COUNT, d_o, d_w, size=size, in_form=in_form, out_form=out_form)
                got = A.download(d_o, (words + GUARD,))
                assert np.array_equal(got[:words].reshape(want.shape), want), (case, size, in_form, out_form, "device against the host twin")
                assert (got[words:] == np.uint64(FILL)).all(), (case, size, in_form, out_form, "guard words")
                assert np.array_equal(A.download(d_x, x.shape), x), (case, size, in_form, out_form, "the input was written")
    A.close(); B.close()


def test_device_refusals_write_nothing():
    import crcnn_amd as ca
    n = 256
    A = ca.Engine(n, SMALL, T, device=0); B = A.level(2); H = ca.Engine(n, SMALL, T, device=-1)
    x = inputs(SMALL, n, 2, 3)
    d_x = A.upload(x); words = COUNT * 2 * 2 * n
    d_o = A.alloc(words * 8 + 16); A.L.crc_memset(A.c, d_o.ptr, 0xff, words * 8 + 16, A.stream)
    d_w = A.alloc(A.mod_switch_work_bytes(B, COUNT, in_form=NTT, out_form=COEFF))
    call = lambda f, t, i, fi, cnt, size, o, fo, w: A.L.crc_mod_switch_forms(f, t, i, fi, cnt, size, o, fo, w, None)
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr, 2, d_w.ptr) == -1 and call(A.c, B.c, d_x.ptr, 3, COUNT, 2, d_o.ptr, COEFF, d_w.ptr) == -1
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 1, d_o.ptr, COEFF, d_w.ptr) == -1 and call(A.c, B.c, d_x.ptr, COEFF, COUNT, 4, d_o.ptr, COEFF, d_w.ptr) == -1
    assert call(B.c, A.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr, COEFF, d_w.ptr) == -1 and call(A.c, A.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr, COEFF, d_w.ptr) == -1
    assert call(H.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr, COEFF, d_w.ptr) == -1                      # a host-only context has no device entry points
    assert call(A.c, B.c, None, COEFF, COUNT, 2, d_o.ptr, COEFF, d_w.ptr) == -1 and call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, None, COEFF, d_w.ptr) == -1
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr, COEFF, None) == -1
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_o.ptr + 8, COEFF, d_w.ptr) == -1                 # not 16-byte aligned
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_x.ptr, COEFF, d_w.ptr) == -1                     # in place
    assert call(A.c, B.c, d_x.ptr, COEFF, COUNT, 2, d_x.ptr + x.nbytes - 16, COEFF, d_w.ptr) == -1     # the output starts inside the input
    assert call(A.c, B.c, d_x.ptr, NTT, COUNT, 2, d_o.ptr, COEFF, d_x.ptr) == -1                       # the work space is the input
    assert call(A.c, B.c, d_x.ptr, COEFF, 0, 2, d_o.ptr, COEFF, d_w.ptr) == 0
    assert (A.download(d_o, (words + 2,)) == np.uint64(FILL)).all() and np.array_equal(A.download(d_x, x.shape), x)
    # a prefix context on the host only is as good a target: only its parameters are read
    HB = H.level(2)
    A.mod_switch_dev(HB, d_x, COUNT, d_o, d_w)
    assert np.array_equal(A.download(d_o, (COUNT, 2, 2, n)), H.mod_switch(HB, x))
    A.close(); B.close(); H.close(); HB.close()


def sparse(n, terms, rng, lo, hi):
    p = np.zeros(n, dtype=np.int64)
    for pos in rng.choice(n, size=terms, replace=False):
        p[pos] = rng.randint(lo, hi)
    return p


def sparse_negacyclic(a, b, t):
    n = len(a); out = [0] * n
    for i in np.nonzero(a)[0]:
        for j in np.nonzero(b)[0]:
            v = int(a[i]) * int(b[j])
            if i + j < n:
                out[i + j] += v
            else:
                out[i + j - n] -= v
    return np.array([v % t for v in out], dtype=np.int64)


def test_a_computation_continues_at_the_lower_level():
    """encrypt, multiply_plain and add under three moduli; switch; square + relinearise under two, with an evaluation key generated there from the prefix rows of the
    secret key; decrypt there.  The budget right after the switch is at least the derived bound less 2 bits"""
    import crcnn_amd as ca
    n, kept = 4096, 2
    q = default_primes(n, 3)
    A = ca.Engine(n, q, T, device=0); B = A.level(kept)
    sk, pk = A.keygen(5)
    skB = np.ascontiguousarray(sk[:kept])
    rng = np.random.RandomState(8)
    m1, m2, w = sparse(n, 8, rng, 1, T), sparse(n, 8, rng, 1, T), sparse(n, 4, rng, 1, 6)
    cts = A.encrypt(pk, np.stack([m1, m2]).astype(np.uint64), 9)
    d_a, d_b = A.upload(cts[0:1]), A.upload(cts[1:2])
    d_w = A.alloc(A.k * n * 8); A.plain_to_ntt(A.upload(w.astype(np.uint64)[None]), 1, d_w)
    A.multiply_plain(d_a, d_w, 1, 1); A.add(d_a, d_b, 1)
    before = A.download(d_a, (1, 2, A.k, n))
    expect1 = (sparse_negacyclic(m1, w, T) + m2) % T
    assert np.array_equal(A.decrypt(sk, before)[0].astype(np.int64), expect1)
    b_from = A.noise_budget(sk, before[0])
    d_low = A.alloc(2 * kept * n * 8)
    A.mod_switch_dev(B, d_a, 1, d_low, A.alloc(A.mod_switch_work_bytes(B, 1)))
    A.sync()
    d_skB = B.upload(skB); d_bits = B.alloc(4)
    B.noise_budget_dev(d_skB, d_low, 1, d_bits, B.alloc(B.noise_budget_dev_work_bytes(1)))
    b_to = int(B.download(d_bits, (1,), dtype=np.int32)[0])
    bound = mm.budget_bound(b_from, T, n, mm.product(q[:kept]))
    print(f"budget {b_from} bits under 3 moduli, {b_to} under 2; derived bound {bound}")
    assert b_to >= bound - 2 and bound - 2 > 40
    low = B.download(d_low, (1, 2, kept, n))
    assert np.array_equal(low, A.mod_switch(B, before)) and np.array_equal(B.decrypt(skB, low)[0].astype(np.int64), expect1)
    evkB = B.gen_evk(13, skB)
    d_y = B.alloc(2 * kept * n * 8)
    B.square_relin(d_low, 1, B.upload(evkB), d_y, B.alloc(B.square_relin_work_bytes(1)))
    y = B.download(d_y, (1, 2, kept, n))
    assert B.noise_budget(skB, y[0]) > 0
    assert np.array_equal(B.decrypt(skB, y)[0].astype(np.int64), sparse_negacyclic(expect1, expect1, T))
    A.close(); B.close()


def test_a_switch_on_a_stream_of_the_callers_own():
    """the same bytes as alone when the switch runs on a non-default stream between the transforms of another tensor"""
    import crcnn_amd as ca
    n, kept = 8192, 2
    q = default_primes(n, 3)
    A = ca.Engine(n, q, T, device=0); B = A.level(kept)
    x = inputs(q, n, 2, 99)
    rng = np.random.RandomState(4)
    other = np.stack([(rng.randint(0, 1 << 62, size=(64, 2, n), dtype=np.int64) % qi).astype(np.uint64) for qi in q], axis=2)
    d_x, d_other = A.upload(x), A.upload(other)
    words = COUNT * 2 * kept * n
    alone = {}
    for fi, fo in ((COEFF, COEFF), (NTT, NTT)):
        d_o = A.alloc(words * 8)
        A.mod_switch_dev(B, d_x, COUNT, d_o, A.alloc(A.mod_switch_work_bytes(B, COUNT, in_form=fi, out_form=fo)), in_form=fi, out_form=fo)
        alone[fi, fo] = A.download(d_o, (COUNT, 2, kept, n))
        assert np.array_equal(alone[fi, fo], A.mod_switch(B, x, in_form=fi, out_form=fo))
    s = ctypes.c_void_p()
    assert A.L.crc_stream_create(A.c, ctypes.byref(s)) == 0
    A.sync()
    A.stream = s
    try:
        for fi, fo in ((COEFF, COEFF), (NTT, NTT)):
            d_o = A.alloc(words * 8); d_w = A.alloc(A.mod_switch_work_bytes(B, COUNT, in_form=fi, out_form=fo))
            A.ntt_fwd(d_other, 64)
            A.mod_switch_dev(B, d_x, COUNT, d_o, d_w, in_form=fi, out_form=fo)
            A.ntt_inv(d_other, 64)
            assert np.array_equal(A.download(d_o, (COUNT, 2, kept, n)), alone[fi, fo]), (fi, fo)
            assert np.array_equal(A.download(d_other, other.shape), other)
    finally:
        A.sync()
        A.stream = None
        A.L.crc_stream_destroy(A.c, s)
    A.close(); B.close()
