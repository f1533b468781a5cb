"""Noise flooding on the GPU: crc_flood_dev bit for bit against its host twin for every ring size's path, both forms and the word boundaries of the flood
width, with guard words around the tensor and the work space; against tests/flood_model.py (the definition from the raw keystream) on the whole grid at n = 256
and on ciphertext 0 at every width and form at the larger rings (the streams of the other ciphertexts differ in the nonce only, which n = 256
covers); the two forms against each other; a
chain encrypt -> multiply_plain -> add -> flood -> mod-switch -> decrypt with every budget inside its derived bounds; a flood on a stream of the caller's own;
refusals that launch nothing."""
import ctypes

import numpy as np
import pytest

import flood_model as fm
import mod_switch_model as mm

pytestmark = pytest.mark.gpu
COEFF, NTT = 0, 1
T = 65537
GUARD = 32                     # words: 256 bytes, the alignment of a work-space region
FILL = 0xffffffffffffffff
INVALID, UNSUPPORTED = -1, -4


def default_primes(n, k):
    import crcnn_amd as ca
    out = []
    for m in (n, 8192, 16384):
        if m >= max(n, 1024):
            out += [p for p in ca.default_coeff_modulus_128(m) if p not in out]
    assert len(out) >= k
    return out[:k]


def largest_bits(E):
    return max(B for B in range(1, 127) if E.flood_supported(B))


def tensor(q, n, count, seed):
    """random canonical residues; ciphertext 0 all zero (the flood alone: a fresh encryption of zero)"""
    rng = np.random.RandomState(seed)
    x = np.stack([(rng.randint(0, 1 << 62, size=(count, 2, n), dtype=np.int64) % qi).astype(np.uint64) for qi in q], axis=2)
    x[0] = 0
    return np.ascontiguousarray(x)


def flood_guarded(E, d_pk, x, B, form, seed=None, key=None, stream_base=0):
    """the device call on a tensor and a work space that both sit between guard words; returns the flooded tensor after checking all four guards"""
    count = x.shape[0]; words = x.size
    buf = np.full(words + 2 * GUARD, FILL, dtype=np.uint64); buf[GUARD:GUARD + words] = x.reshape(-1)
    d_t = E.upload(buf)
    wb = E.flood_dev_work_bytes(count, form)
    assert wb == 256 + 8 * (-(-count * E.k * E.n // 32) * 32 + -(-count * 2 * E.k * E.n // 32) * 32)
    d_w = E.alloc(wb + 2 * 8 * GUARD); E.L.crc_memset(E.c, d_w.ptr, 0xff, wb + 2 * 8 * GUARD, E.stream)
    assert d_t.ptr % 256 == 0 and d_w.ptr % 256 == 0
    E.flood_dev(d_pk, d_t.ptr + 8 * GUARD, count, B, d_w.ptr + 8 * GUARD, form=form, seed=seed, key=key, stream_base=stream_base)
    got = E.download(d_t, (words + 2 * GUARD,))
    assert (got[:GUARD] == np.uint64(FILL)).all() and (got[GUARD + words:] == np.uint64(FILL)).all(), "guard words of the tensor"
    work = E.download(d_w, (wb // 8 + 2 * GUARD,))
    assert (work[:GUARD] == np.uint64(FILL)).all() and (work[wb // 8:] == np.uint64(FILL)).all(), "guard words of the work space"
    return got[GUARD:GUARD + words].reshape(x.shape)


# The ring sizes at which the row transform of the ternary rows takes another kernel (n = 256: the generic row kernel; 4096, 8192: wave-local; 16384 with k = 4
# and count 2: the large-ring path).  The join kernel itself runs the generic LDS passes at every one of them, with another pass structure at each
# (log2 n = 8, 12, 13, 14: two, four, four and a radix-2, four and a radix-4 pass)
SHAPES = [("n256", 256, 2, (1, 3)), ("n4096", 4096, 2, (1, 3)), ("n8192", 8192, 3, (1, 3)), ("n16384", 16384, 4, (2,))]


@pytest.mark.parametrize("form", [COEFF, NTT], ids=["coeff", "ntt"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_device_equals_the_host_twin_and_the_model(shape, form):
    import crcnn_amd as ca
    _, n, k, counts = shape
    q = default_primes(n, k)
    E = ca.Engine(n, q, T, device=0)
    _, pk = E.keygen(3)
    d_pk = E.upload(pk)
    top = largest_bits(E)
    assert fm.admissible(q, T, n, top) and not fm.admissible(q, T, n, top + 1)
    for count in counts:
        x = tensor(q, n, count, n + count)
        for B in (1, 64, 65, top):
            seed = 1000 + B
            want = E.flood(pk, x, B, form=form, seed=seed)
            got = flood_guarded(E, d_pk, x, B, form, seed=seed)
            assert np.array_equal(got, want), (shape[0], form, count, B, "device against the host twin")
            assert not np.array_equal(got[0], x[0])
            # the model (pure Python) on ciphertext 0 at every width, once per shape and form; at n = 256 for every count as well
            if n == 256 or count == counts[0]:
                m = fm.flood(E, pk, x[:1], form, B, fm.seed_key(seed))
                assert np.array_equal(want[:1], m), (shape[0], form, count, B, "host twin against the model")
    # the key form: ciphertext m of a call at stream_base has the stream of ciphertext 0 of a call at stream_base + m
    key = bytes(range(32)); x = tensor(q, n, counts[-1], 7)
    got = flood_guarded(E, d_pk, x, 65, form, key=key, stream_base=(1 << 32) - 1)
    assert np.array_equal(got, E.flood(pk, x, 65, form=form, key=key, stream_base=(1 << 32) - 1))
    assert np.array_equal(got[1:2], E.flood(pk, x[1:2], 65, form=form, key=key, stream_base=1 << 32))
    E.close()


@pytest.mark.parametrize("n,k", [(256, 2), (4096, 2)], ids=["n256", "n4096"])
def test_the_two_forms_agree(n, k):
    """flood an NTT-form tensor; flood the same tensor in coefficient form under the same key; the residues agree through crc_ntt_fwd"""
    import crcnn_amd as ca
    q = default_primes(n, k)
    E = ca.Engine(n, q, T, device=0)
    _, pk = E.keygen(3); d_pk = E.upload(pk)
    x = tensor(q, n, 3, 21)                                           # coefficient form
    d_n = E.upload(x); E.ntt_fwd(d_n, 3); x_ntt = E.download(d_n, x.shape)
    d_w = E.alloc(E.flood_dev_work_bytes(3, NTT))
    key = bytes(range(1, 33))
    E.flood_dev(d_pk, d_n, 3, 65, d_w, form=NTT, key=key, stream_base=5)
    d_c = E.upload(x)
    E.flood_dev(d_pk, d_c, 3, 65, d_w, form=COEFF, key=key, stream_base=5)
    E.ntt_fwd(d_c, 3)
    a, b = E.download(d_n, x.shape), E.download(d_c, x.shape)
    assert np.array_equal(a, b) and not np.array_equal(a, x_ntt)
    E.close()


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


def chain_budget_bound(q, t, n, w_l1):
    """the budget, derived, of  encrypt(m1) * w + encrypt(m2)  for a plaintext w with sum |w_j| <= w_l1 (coefficients below t / 2).  The budget measures
    N = |t (c0 + c1 s) mod q|.  Fresh: c0 + c1 s = Delta m + w0 with |w0| <= 19 (2 n + 1) and t Delta m = -(q mod t) m (mod q), so N0 <= 19 t (2 n + 1) + t^2.
    Times w: the noise part grows by at most w_l1, and m1 w = (m1 w mod t) + t K contributes (q mod t) (m1 w) with |m1 w| <= w_l1 t: N1 <= w_l1 N0.
    Plus the second ciphertext: N <= (w_l1 + 1) N0, and the budget is at least bits(q) - bits(N) - 1"""
    N = (w_l1 + 1) * (19 * t * (2 * n + 1) + t * t)
    return mm.product(q).bit_length() - N.bit_length() - 1


def test_chain_flood_switch_decrypt():
    import crcnn_amd as ca
    n = 4096
    q = default_primes(n, 2)
    A = ca.Engine(n, q, T, device=0); L = A.level(1)
    sk, pk = A.keygen(5)
    rng = np.random.RandomState(8)
    m1, m2, w = sparse(n, 8, rng, 1, T), sparse(n, 8, rng, 1, T), sparse(n, 4, rng, 1, 6)
    cts = A.encrypt(pk, np.stack([m1, m2]).astype(np.uint64), 9)
    d_a, d_b = A.upload(cts[0:1]), A.upload(cts[1:2])
    d_w = A.alloc(A.k * n * 8); A.plain_to_ntt(A.upload(w.astype(np.uint64)[None]), 1, d_w)
    A.multiply_plain(d_a, d_w, 1, 1); A.add(d_a, d_b, 1)
    before = A.download(d_a, (1, 2, A.k, n))
    expect = (sparse_negacyclic(m1, w, T) + m2) % T
    assert np.array_equal(A.decrypt(sk, before)[0].astype(np.int64), expect)
    b0 = chain_budget_bound(q, T, n, 4 * 5)
    b_meas = A.noise_budget(sk, before[0])
    # the server floods by the A-PRIORI budget b0, never by the measured one
    B = A.flood_bits(b0, 40)
    assert B == fm.flood_bits(q, T, n, b0, 40) and A.flood_supported(B)
    A.flood_dev(A.upload(pk), d_a, 1, B, A.alloc(A.flood_dev_work_bytes(1, COEFF)), form=COEFF, key=bytes(32), stream_base=0)
    flooded = A.download(d_a, (1, 2, A.k, n))
    assert np.array_equal(flooded, A.flood(pk, before, B, form=COEFF, key=bytes(32)))
    assert np.array_equal(A.decrypt(sk, flooded)[0].astype(np.int64), expect)
    b1 = A.noise_budget(sk, flooded[0])
    lo1, hi1 = fm.budget_lower(b0, T, n, q, B), fm.budget_upper(b0, T, n, q, B)
    assert lo1 == A.flood_budget_bound(b0, B) and hi1 is not None
    d_low = A.alloc(2 * n * 8)
    A.mod_switch_dev(L, d_a, 1, d_low, A.alloc(A.mod_switch_work_bytes(L, 1)))
    low = A.download(d_low, (1, 2, 1, n))
    skL = np.ascontiguousarray(sk[:1])
    b2 = L.noise_budget(skL, low[0])
    lo2 = mm.budget_bound(lo1 - 1, T, n, q[0])                        # (the flooded ciphertext has at least lo1 - 1 bits: flood_model's docstring)
    hi2 = fm.budget_upper_after_switch(b0, T, n, q, B, 1)
    print(f"budget: a priori {b0}, measured {b_meas}; flood_bits {B}; after the flood {b1} in [{lo1} - 2, {hi1}]; after the switch {b2} in [{lo2} - 2, {hi2}]")
    assert b_meas >= b0 > 0
    assert lo1 - 2 <= b1 <= hi1 and lo1 - 2 > 0
    # After the switch only the lower bound binds in this chain: the flood, divided by the dropped 54-bit prime, is t 2^62 / 2^54 ~ 2^25 and lies BELOW the
    # switch's own rounding term t (n + 1) ~ 2^28, which has no lower bound of its own -- budget_upper_after_switch says so by returning None.  It is asserted
    # where it exists (tests/test_flood_cpu.py has a chain at three moduli where the flood survives the division and the bound binds)
    assert lo2 - 2 <= b2 and lo2 - 2 > 0 and (hi2 is None or b2 <= hi2)
    assert np.array_equal(L.decrypt(skL, low)[0].astype(np.int64), expect)
    A.close(); L.close()


def test_a_flood_on_a_stream_of_the_callers_own():
    """the same bytes as alone when the flood runs on a non-default stream between the transforms of another tensor"""
    import crcnn_amd as ca
    n = 8192
    q = default_primes(n, 3)
    E = ca.Engine(n, q, T, device=0)
    _, pk = E.keygen(3); d_pk = E.upload(pk)
    x = tensor(q, n, 3, 99)
    rng = np.random.RandomState(4)
    other = np.stack([(rng.randint(0, 1 << 62, size=(64, 2, n), dtype=np.int64) % qi).astype(np.uint64) for qi in q], axis=2)
    d_other = E.upload(other)
    want = {f: E.flood(pk, x, 70, form=f, seed=11) for f in (COEFF, NTT)}
    s = ctypes.c_void_p()
    assert E.L.crc_stream_create(E.c, ctypes.byref(s)) == 0
    E.sync()
    E.stream = s
    try:
        for f in (COEFF, NTT):
            d_x = E.upload(x); d_w = E.alloc(E.flood_dev_work_bytes(3, f))
            E.ntt_fwd(d_other, 64)
            E.flood_dev(d_pk, d_x, 3, 70, d_w, form=f, seed=11)
            E.ntt_inv(d_other, 64)
            assert np.array_equal(E.download(d_x, x.shape), want[f]), f
            assert np.array_equal(E.download(d_other, other.shape), other)
    finally:
        E.sync()
        E.stream = None
        E.L.crc_stream_destroy(E.c, s)
    E.close()


def test_device_refusals_launch_nothing():
    import crcnn_amd as ca
    n = 256
    q = default_primes(n, 2)
    E = ca.Engine(n, q, T, device=0); H = ca.Engine(n, q, T, device=-1)
    _, pk = E.keygen(3); d_pk = E.upload(pk)
    x = tensor(q, n, 3, 5); words = x.size
    buf = np.full(words + 2 * GUARD, FILL, dtype=np.uint64); buf[GUARD:GUARD + words] = x.reshape(-1)
    d_t = E.upload(buf); ct = d_t.ptr + 8 * GUARD
    wb = E.flood_dev_work_bytes(3, COEFF)
    d_w = E.alloc(wb); E.L.crc_memset(E.c, d_w.ptr, 0xff, wb, E.stream)
    top = largest_bits(E)
    call = lambda c, p, t, cnt, form, B, w: E.L.crc_flood_dev(c, p, t, cnt, form, B, 1, w, None)
    for B in (0, -1, 127, top + 1):
        assert call(E.c, d_pk.ptr, ct, 3, COEFF, B, d_w.ptr) == INVALID and call(E.c, d_pk.ptr, ct, 3, NTT, B, d_w.ptr) == INVALID, B
    for form in (2, 3, 4, 5, 6, -1):
        assert call(E.c, d_pk.ptr, ct, 3, form, 40, d_w.ptr) == UNSUPPORTED and E.flood_dev_work_bytes(3, form) == 0
    assert call(H.c, d_pk.ptr, ct, 3, COEFF, 40, d_w.ptr) == INVALID                                  # a host-only context has no device entry points
    assert call(E.c, None, ct, 3, COEFF, 40, d_w.ptr) == INVALID and call(E.c, d_pk.ptr, None, 3, COEFF, 40, d_w.ptr) == INVALID
    assert call(E.c, d_pk.ptr, ct, 3, COEFF, 40, None) == INVALID
    assert call(E.c, d_pk.ptr, ct + 8, 3, COEFF, 40, d_w.ptr) == INVALID                              # not 16-byte aligned
    assert call(E.c, d_pk.ptr, ct, 3, COEFF, 40, ct) == INVALID and call(E.c, ct, ct, 3, COEFF, 40, d_w.ptr) == INVALID      # work space / key inside the tensor
    assert E.L.crc_flood_dev_key(E.c, d_pk.ptr, ct, 3, COEFF, 40, None, 0, d_w.ptr, None) == INVALID
    assert call(E.c, d_pk.ptr, ct, 0, COEFF, 40, d_w.ptr) == 0 and call(E.c, None, None, 0, 5, 0, None) == 0 and call(H.c, d_pk.ptr, ct, 0, COEFF, 40, d_w.ptr) == INVALID
    assert np.array_equal(E.download(d_t, buf.shape), buf), "a refusal wrote to the tensor or its guard words"
    assert (E.download(d_w, (wb // 8,)) == np.uint64(FILL)).all(), "a refusal wrote to the work space"
    E.close(); H.close()
