"""GPU exactness of the fp64 key switch of relinearisation at its integer bound and at its admission limits.

kernels_relin64.hip forms R_j = sum_g digit_g (*) key_g[j] ((*): negacyclic product, keys as centred residues of q_j, digits below 2^dbc) as an INTEGER
polynomial modulo two fp64 primes p0, p1 < 2^47 and lifts it by CRT: exact only while |R_j| < p0 p1 / 2 ~ 2^93.  Two host predicates decide which parameter
sets may take that path; every other set takes the key switch over the coefficient moduli (relin_path = 1), which has no integer bound:
  * k_relin64_supported:      B = logn + ceil(log2 D) + dbc + qbits <= 91, D <= 48   (D digit polynomials, qbits the width of the largest q_i);
  * k_relin64_pool_supported: B + ceil(log2 W) <= 92 for a pooling window of W ciphertexts, dbc <= 20, at most 4 digits per residue, W <= 64.

Where each ring sits (default moduli, 55- and 54-bit):
  ring (n, k)          B at dbc 16   last dbc admitted / first refused   pooled B at W = 4   pooled limit (B = 92) at dbc 16 / first refused
  (4096, 2)            86            21 (91) / 22                         88                  W = 36..64 / none (W <= 64)
  (8192, 3), (8192, 4) 88            19 (91) / 20                         90                  3 x 3, 4 x 4 / 5 x 4
  (16384, 4)           89            18 (91) / 19                         91                  3 x 2, 4 x 2 / 3 x 3
  (16384, 8)           90            17 (91) / 18; dbc 10 (D = 48)        92                  2 x 2 (shipped) / 3 x 2
                                     admitted, dbc 9 (D = 54) refused by both paths
Two 60-bit primes at n = 4096 reach B = 91 at dbc 16 through qbits; two 40-bit primes take the CRT lift's branch where |a0| >= q.

Operands.  Keys all-equal in coefficient form, +(q_j - 1) / 2 for output polynomial 0 and (q_j + 1) / 2 (centred -(q_j - 1) / 2) for polynomial 1, brought to
NTT form by the ORACLE's transform; also handed over lazily (r + q_j, as SEAL does), and NTT-form rows at q_j - 1 / at the limb-extreme residue (the largest
per-term products of the fallback's 28-bit-limb MAC).  c2 is chosen so that its premultiplied form c2 (q/q_i)^-1 mod q_i is the largest residue below q_i
whose low L_i - 1 digits are all 2^dbc - 1; next to it c2 = 0, random c2 and c0 = c1 = q - 1.  With all-equal operands R_j at coefficient n - 1 is
n K_j sum_g e_g, no wrap-around: the test asserts 2 |R_j| >= 2^(B - 1.5) (the predicate rounds D up and counts every digit as 2^dbc), and |R_j| < p0 p1 / 2
where the set is admitted.  Behind a square the digits cannot be chosen: c2 is read back through crc_square and its digits summed, 2 |R_j| >= 2^(B - 2.5).

References: relin_path = 1 on the same inputs (pooled: crc_square_relin_forms under relin_path = 1, then crc_pool), and at n <= 4096 the CPU oracle with the
same dbc.  Every case runs under f64_radix 3 (f64_wave default and 0: the wave-local and the register-holding kernels), 4 and 5, each with relin_mac_ct 4
and 8.  Past each limit the engine takes the fallback today; those cases still compare the default path with the references, so a predicate relaxed past
the bound fails numerically.  Which kernels each test reaches: profiles/relin_bounds_kernels_by_test.txt."""
import math

import numpy as np
import pytest

from netcommon import limb_extreme

pytestmark = pytest.mark.gpu

P60 = [0xffffffffffc0001, 0xfffffffff840001]            # SEAL's small_mods_60bit[0:2]: 1 mod 2^18
P40 = [0xffffe80001, 0xffffc40001]                      # small_mods_40bit[0:2]
T_PLAIN = 1 << 20
# the tuning variants every case runs under: (f64_radix, f64_wave, relin_mac_ct); -1 / 0: the defaults
VARIANTS = [(r, w, ct) for (r, w) in ((3, -1), (3, 0), (4, -1), (5, -1)) for ct in (4, 8)]


def moduli(n, k):
    import crcnn_amd as ca
    return [int(v) for v in ca.default_coeff_modulus_128(n)[:k]]


# ---- the predicates, restated ---------------------------------------------------------------------------------------------------------------------------
def digits(q, dbc):
    L = 0
    while q:
        L += 1; q >>= dbc
    return L


def clog2(x):
    return (x - 1).bit_length()


def bound(n, q, dbc, window=1):
    """(B, D): the left-hand side of the predicate (with ceil(log2 W) for a pooled key switch) and the number of digit polynomials"""
    D = sum(digits(x, dbc) for x in q)
    return int(math.log2(n)) + clog2(D) + dbc + max(x.bit_length() for x in q) + clog2(window), D


def admitted(n, q, dbc):
    B, D = bound(n, q, dbc)
    return 1 <= dbc <= 32 and D <= 48 and B <= 91


def pool_admitted(n, q, dbc, window):
    return (admitted(n, q, dbc) and 1 <= window <= 64 and dbc <= 20 and all(digits(x, dbc) <= 4 for x in q)
            and bound(n, q, dbc, window)[0] <= 92)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------
def qhat(q, i):
    r = 1
    for l, x in enumerate(q):
        if l != i:
            r = r * x % q[i]
    return r


def digit_extreme(qi, dbc):
    """the largest residue below q_i whose low L_i - 1 digits are all 2^dbc - 1"""
    s = (digits(qi, dbc) - 1) * dbc
    v = ((qi - 1) >> s << s) | ((1 << s) - 1)
    if v >= qi:
        v -= 1 << s
    assert v < qi and all((v >> (d * dbc)) & ((1 << dbc) - 1) == (1 << dbc) - 1 for d in range(digits(qi, dbc) - 1))
    assert v + (1 << s) >= qi                                            # no larger top digit
    return v


def extreme_keys(O, E, dbc, kind):
    """the key blob, rows [(2 g + poly)][j][n]: 'coeff' all-equal +-(q_j - 1) / 2 in coefficient form, 'lazy' the same plus q_j, 'ntt' NTT-form rows at
    q_j - 1 (poly 0) and at the limb-extreme residue (poly 1)"""
    q, n, k = [int(v) for v in E.q], E.n, E.k
    rows = np.empty((E.L.crc_evk_words(E.c, dbc) // (k * n), k, n), dtype=np.uint64)
    assert rows.shape[0] == 2 * bound(n, q, dbc)[1]
    for j in range(k):
        if kind == "ntt":
            rows[0::2, j] = np.uint64(q[j] - 1); rows[1::2, j] = np.uint64(limb_extreme(q[j]))
            continue
        for poly, c in ((0, (q[j] - 1) // 2), (1, (q[j] + 1) // 2)):
            coef = np.full(n, c, dtype=np.uint64)
            f = O.ntt_fwd(j, coef)
            assert np.array_equal(O.ntt_inv(j, f), coef)
            rows[poly::2, j] = f + np.uint64(q[j] if kind == "lazy" else 0)
    return rows.reshape(-1)


def relin_inputs(E, dbc, rng):
    """size-3 ciphertexts: [extreme c2 with c0 = c1 = q - 1, c2 = 0, random c2]; and the digit sums of the extreme one"""
    q, n, k = [int(v) for v in E.q], E.n, E.k
    x3 = np.empty((3, 3, k, n), dtype=np.uint64)
    for i in range(k):
        x3[:, :, i] = rng.integers(0, q[i], size=(3, 3, n), dtype=np.uint64)
        x3[0, :2, i] = np.uint64(q[i] - 1)
        v = digit_extreme(q[i], dbc)
        x3[0, 2, i] = np.uint64(v * qhat(q, i) % q[i])
        assert int(x3[0, 2, i, 0]) * pow(qhat(q, i), -1, q[i]) % q[i] == v
    x3[1, 2] = 0
    esum = sum((digit_extreme(qi, dbc) >> (d * dbc)) & ((1 << dbc) - 1) for qi in q for d in range(digits(qi, dbc)))
    return x3, n * esum


def digit_sum(E, c2, dbc):
    """sum over every digit polynomial and coefficient of c2 (q/q_i)^-1 mod q_i, per ciphertext: R_j at coefficient n - 1 is K_j times this"""
    q = [int(v) for v in E.q]
    out = np.zeros(c2.shape[0], dtype=object)
    for i in range(E.k):
        inv = pow(qhat(q, i), -1, q[i])
        e = np.array((c2[:, i].astype(object) * inv) % q[i], dtype=np.uint64)
        for d in range(digits(q[i], dbc)):
            out += ((e >> np.uint64(d * dbc)) & np.uint64((1 << dbc) - 1)).astype(np.uint64).sum(axis=1).astype(object)
    return out


def reach(n, q, dbc, S, window, slack):
    """|R_j| = (q_j - 1) / 2 S at coefficient n - 1 (the largest q_j): asserted to reach the predicate's bound within `slack` bits"""
    B = bound(n, q, dbc, window)[0]
    R = max((qj - 1) // 2 for qj in q) * int(S)
    assert math.log2(2 * R) >= B - slack, (n, len(q), dbc, window, math.log2(2 * R), B)
    return R


def crt_half(E):
    p0, p1 = [int(v) for v in E.table("f64_primes")[:2]]
    return p0 * p1 // 2


def set_variant(E, v):
    E.set_tuning("f64_radix", v[0]); E.set_tuning("f64_wave", v[1]); E.set_tuning("relin_mac_ct", v[2])


def reset_tuning(E):
    for name, val in (("f64_radix", 0), ("f64_wave", -1), ("relin_mac_ct", 0), ("relin_path", 0)):
        E.set_tuning(name, val)


# ---- unpooled: crc_relinearize and crc_square_relin_forms ----------------------------------------------------------------------------------------------
# (n, moduli, [dbc...]): the shipped dbc 16, the last admitted, the first refused; (16384, 8) also D = 48 and the steps where the worst case passes p0 p1 / 2
RELIN = [(4096, 2, [16, 21, 22]), (8192, 3, [16, 19, 20]), (8192, 4, [16, 19, 20]), (16384, 4, [16, 18, 19]), (16384, 8, [16, 17, 18, 10, 21, 22]),
         (4096, "p60", [16, 17]), (4096, "p40", [16])]


@pytest.mark.parametrize("n,k,dbcs", RELIN, ids=[f"n{n}_{k if isinstance(k, str) else 'k%d' % k}" for n, k, _ in RELIN])
def test_key_switch_at_the_integer_bound(n, k, dbcs):
    import crcnn_amd as ca
    from oracle import orc
    q = P60 if k == "p60" else P40 if k == "p40" else moduli(n, k)
    E = ca.Engine(n, q, T_PLAIN, device=0)
    O = orc.Oracle(n, q, T_PLAIN)
    try:
        rng = np.random.default_rng(n + len(q))
        for dbc in dbcs:
            adm = admitted(n, q, dbc)
            x3, S = relin_inputs(E, dbc, rng)
            R = reach(n, q, dbc, S, 1, 1.5)
            if not adm and dbc >= 21 and n == 16384:
                assert R > crt_half(E), (dbc, math.log2(R))             # past the CRT's range: only the predicate keeps this off the fp64 path
            x = np.ascontiguousarray(x3[:, :2])                                # (square inputs: c0 = c1 = q - 1, then two random ciphertexts)
            d_x3, d_x = E.upload(x3), E.upload(x)
            d_xn = E.upload(x); E.ntt_fwd(d_xn, 3)
            d_w = E.alloc(E.square_relin_work_bytes(3, dbc))
            d_y = E.alloc(x.nbytes); d_y3 = E.alloc(x3.nbytes)
            # the square's c2, premultiplied, digit-summed: what the key switch behind crc_square_relin_forms meets
            E.square(d_x, 3, d_y3, d_w)
            Rsq = reach(n, q, dbc, max(digit_sum(E, E.download(d_y3, x3.shape)[:, 2], dbc)), 1, 2.5)
            for kind in ("coeff", "lazy", "ntt"):
                evk = extreme_keys(O, E, dbc, kind)
                d_evk = E.upload(evk)
                # references, once per case: the key switch over the coefficient moduli, and the oracle at n <= 4096
                E.set_tuning("relin_path", 1)
                E.relinearize(d_x3, 3, d_evk, d_y, d_w, dbc=dbc)
                want = E.download(d_y, x.shape)
                E.square_relin(d_x, 3, d_evk, d_y, d_w, dbc=dbc)
                want_sq = E.download(d_y, x.shape)
                E.set_tuning("relin_path", 0)
                if n <= 4096:
                    for c in range(3):
                        assert np.array_equal(want[c], O.relinearize(x3[c], evk, dbc)), ("oracle", dbc, kind, c)
                    assert np.array_equal(want_sq, O.square_layer(x, evk, dbc, threads=3)), ("oracle square", dbc, kind)
                for v in (VARIANTS if kind == "coeff" else VARIANTS[:1]):
                    set_variant(E, v)
                    E.L.crc_memset(E.c, E.p(d_y), 0xff, x.nbytes, E.stream)
                    E.relinearize(d_x3, 3, d_evk, d_y, d_w, dbc=dbc)
                    got = E.download(d_y, x.shape)
                    for c in range(3):
                        assert np.array_equal(got[c], want[c]), ("relinearize", dbc, kind, v, c)
                    for fin, fout in ((ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT), (ca.NTT, ca.COEFF), (ca.COEFF, ca.NTT)):
                        E.L.crc_memset(E.c, E.p(d_y), 0xff, x.nbytes, E.stream)
                        E.square_relin(d_xn if fin == ca.NTT else d_x, 3, d_evk, d_y, d_w, dbc=dbc, in_form=fin, out_form=fout)
                        if fout == ca.NTT:
                            E.ntt_inv(d_y, 3)
                        got = E.download(d_y, x.shape)
                        for c in range(3):
                            assert np.array_equal(got[c], want_sq[c]), ("square_relin", dbc, kind, v, fin, fout, c)
                reset_tuning(E)
                d_evk.free()
            for b in (d_x3, d_x, d_xn, d_w, d_y, d_y3):
                b.free()
            if adm:                                                      # (after the numeric checks: a narrower CRT fails those first)
                assert max(R, Rsq) < crt_half(E), (dbc, math.log2(max(R, Rsq)))
    finally:
        reset_tuning(E)
        E.close()


# ---- pooled: crc_square_pool_relin_forms -------------------------------------------------------------------------------------------------------------------
# (n, k, dbc, xf, yf): the pooled window limits (two-field digit kernel except where noted), the largest dbc at W = 4 (one-word kernel), the shipped 2 x 2;
# then one step past each limit and (16384, 8) at 8 x 8, where the worst case passes p0 p1 / 2 -- run only if the engine admits them
POOL = [(4096, 2, 16, 8, 8), (4096, 2, 20, 2, 2), (4096, 2, 16, 2, 2), (8192, 3, 16, 4, 4), (8192, 3, 18, 2, 2), (8192, 4, 16, 4, 4), (16384, 4, 16, 4, 2),
        (16384, 4, 16, 2, 2), (16384, 8, 16, 2, 2),
        (8192, 3, 16, 5, 4), (8192, 3, 19, 2, 2), (16384, 4, 16, 3, 3), (16384, 8, 16, 3, 2), (16384, 8, 16, 8, 8)]


def _one_word(q, dbc, W):
    """k_relinearize64's choice of the one-word digit packing"""
    F = dbc + clog2(W)
    return F <= 32 and all((digits(x, dbc) - 1) * F + (x.bit_length() - (digits(x, dbc) - 1) * dbc + clog2(W)) <= 64 for x in q)


@pytest.mark.parametrize("n,k,dbc,xf,yf", POOL, ids=[f"n{c[0]}_k{c[1]}_dbc{c[2]}_{c[3]}x{c[4]}" for c in POOL])
def test_pooled_key_switch_at_the_integer_bound(n, k, dbc, xf, yf):
    import crcnn_amd as ca
    from oracle import orc
    q = moduli(n, k)
    W = xf * yf
    E = ca.Engine(n, q, T_PLAIN, device=0)
    try:
        if not E.square_pool_relin_supported(xf, yf, dbc):
            return                                                       # (refused: test_admission_limits; a relaxed predicate runs the checks below)
        O = orc.Oracle(n, q, T_PLAIN)
        rng = np.random.default_rng(n * 7 + k + dbc + W)
        B_, zd, xd, yd, xs, ys = 1, 2, xf, yf, 1, 1                       # two planes of one window each: two pooled ciphertexts
        cnt, ocnt = zd * xd * yd, zd
        qa = np.array(q, dtype=np.uint64).reshape(1, 1, k, 1)
        x = (rng.integers(0, 1 << 62, size=(cnt, 2, k, n), dtype=np.uint64) % qa)
        x[0] = qa[0] - np.uint64(1)
        x = np.ascontiguousarray(x)
        d_x = E.upload(x); d_xn = E.upload(x); E.ntt_fwd(d_xn, cnt)
        d_w = E.alloc(max(E.square_relin_work_bytes(cnt, dbc), E.square_pool_relin_work_bytes(B_, zd, xd, yd, xs, ys, xf, yf, dbc)))
        d_r = E.alloc(x.nbytes); d_y3 = E.alloc(cnt * 3 * k * n * 8)
        oshape = (ocnt, 2, k, n)
        d_p = E.alloc(ocnt * 2 * k * n * 8); d_f = E.alloc(ocnt * 2 * k * n * 8)
        # the integer: per window, K_j times the digit sums of its ciphertexts' c2
        E.square(d_x, cnt, d_y3, d_w)
        # (the predicate counts ceil(log2 W) bits for the window: a W that is no power of two stays below that by log2 of the ratio)
        R = reach(n, q, dbc, max(digit_sum(E, E.download(d_y3, (cnt, 3, k, n))[:, 2], dbc).reshape(zd, W).sum(axis=1)), W, 2.5 + clog2(W) - math.log2(W))
        pl, _ = E.encode(np.array([1.0 / W], dtype=np.float32))
        d_div = E.alloc(k * n * 8); E.plain_to_ntt(E.upload(pl), 1, d_div)
        for kind in ("coeff", "lazy"):
            evk = extreme_keys(O, E, dbc, kind)
            d_evk = E.upload(evk)
            # references: square + relinearise over the coefficient moduli, then crc_pool (sum; average in NTT form)
            E.set_tuning("relin_path", 1)
            E.square_relin(d_x, cnt, d_evk, d_r, d_w, dbc=dbc)
            E.set_tuning("relin_path", 0)
            E.pool(d_r, B_, zd, xd, yd, xs, ys, xf, yf, None, ca.COEFF, d_p)
            want = E.download(d_p, oshape)
            if n <= 4096:
                ow = np.asarray(O.pool(O.square_layer(x.reshape(zd, xd, yd, 2, k, n), evk, dbc, threads=8), xs, ys, xf, yf))
                assert np.array_equal(want, ow.reshape(oshape)), ("oracle", kind)
            E.ntt_fwd(d_r, cnt)
            E.pool(d_r, B_, zd, xd, yd, xs, ys, xf, yf, d_div, ca.NTT, d_p)
            want_avg = E.download(d_p, oshape)
            for v in (VARIANTS if kind == "coeff" else VARIANTS[:1]):
                set_variant(E, v)
                for fin, fout in ((ca.COEFF, ca.COEFF), (ca.NTT, ca.NTT), (ca.NTT, ca.COEFF), (ca.COEFF, ca.NTT)):
                    E.L.crc_memset(E.c, E.p(d_f), 0xff, ocnt * 2 * k * n * 8, E.stream)
                    E.square_pool_relin(d_xn if fin == ca.NTT else d_x, B_, zd, xd, yd, xs, ys, xf, yf, d_evk, d_f, d_w, dbc=dbc, in_form=fin, out_form=fout)
                    if fout == ca.NTT:
                        E.ntt_inv(d_f, ocnt)
                    assert np.array_equal(E.download(d_f, oshape), want), ("sum", kind, v, fin, fout)
                E.L.crc_memset(E.c, E.p(d_f), 0xff, ocnt * 2 * k * n * 8, E.stream)
                E.square_pool_relin(d_xn, B_, zd, xd, yd, xs, ys, xf, yf, d_evk, d_f, d_w, dbc=dbc, in_form=ca.NTT, out_form=ca.NTT, d_div=d_div)
                assert np.array_equal(E.download(d_f, oshape), want_avg), ("average", kind, v)
            reset_tuning(E)
            d_evk.free()
        if pool_admitted(n, q, dbc, W):                                  # (after the numeric checks, as above)
            assert R < crt_half(E), (n, k, dbc, W, math.log2(R))
    finally:
        reset_tuning(E)
        E.close()


# ---- which sets are admitted --------------------------------------------------------------------------------------------------------------------------------
def test_admission_limits():
    """the table of the module docstring, as the engine answers it: the pooled predicate one step past each window and dbc limit and for 5-digit residues,
    crc_square_pool_relin_forms / crc_relinearize refusing there (on the host, before any launch), and dbc outside 1..60 refused as an invalid argument"""
    import crcnn_amd as ca
    UNSUP, INVAL = -4, -1
    # unpooled limits (the pooled predicate at W = 1 is the unpooled one for dbc <= 20 and 4-digit residues)
    for n, k, last in ((4096, 2, 21), (8192, 3, 19), (8192, 4, 19), (16384, 4, 18), (16384, 8, 17)):
        q = moduli(n, k)
        assert admitted(n, q, last) and not admitted(n, q, last + 1) and bound(n, q, last)[0] == 91, (n, k)
        assert bound(n, q, 16)[0] == {4096: 86, 8192: 88, 16384: 89 if k == 4 else 90}[n]
    assert admitted(4096, P60, 16) and bound(4096, P60, 16)[0] == 91 and not admitted(4096, P60, 17)
    q8 = moduli(16384, 8)
    assert bound(16384, q8, 10)[1] == 48 and admitted(16384, q8, 10) and bound(16384, q8, 9)[1] == 54 and not admitted(16384, q8, 9)
    assert bound(16384, q8, 16, 4)[0] == 92
    # which pooled digit kernel each numeric case meets: the one-word packing at the shipped (16384, 8) 2 x 2, two fields at the wide windows
    assert _one_word(q8, 16, 4) and _one_word(moduli(4096, 2), 20, 4) and _one_word(moduli(8192, 3), 18, 4)
    assert not _one_word(moduli(4096, 2), 16, 64) and not _one_word(moduli(8192, 3), 16, 16) and not _one_word(moduli(16384, 4), 16, 8)
    for n, k, adm, ref in ((4096, 2, [(8, 8), (6, 6)], []), (8192, 3, [(3, 3), (4, 4)], [(5, 4)]), (8192, 4, [(4, 4)], [(5, 4)]),
                           (16384, 4, [(3, 2), (4, 2)], [(3, 3)]), (16384, 8, [(2, 2)], [(3, 2), (8, 8)])):
        q = moduli(n, k)
        E = ca.Engine(n, q, T_PLAIN, device=0)
        try:
            for (n2, k2, dbc, xf, yf) in POOL:                          # the numeric cases' admission, as the restated predicate has it
                if (n2, k2) == (n, k):
                    assert E.square_pool_relin_supported(xf, yf, dbc) == pool_admitted(n, q, dbc, xf * yf), (n, k, dbc, xf, yf)
            for xf, yf in adm:
                assert E.square_pool_relin_supported(xf, yf, 16) and bound(n, q, 16, xf * yf)[0] == 92, (n, k, xf, yf)
            for xf, yf in ref:
                assert not E.square_pool_relin_supported(xf, yf, 16), (n, k, xf, yf)
            # the largest dbc at W = 4, one past it, and 5-digit residues (dbc 13)
            last = {4096: 20, 8192: 18, 16384: 17 if k == 4 else 16}[n]
            assert E.square_pool_relin_supported(2, 2, last) and not E.square_pool_relin_supported(2, 2, last + 1), (n, k)
            assert not E.square_pool_relin_supported(1, 1, 13) and not E.square_pool_relin_supported(2, 2, 13)
            for d in range(14, 21):
                assert E.square_pool_relin_supported(1, 1, d) == admitted(n, q, d), (n, k, d)
            # the pooled entry point refuses what the predicate refuses
            cnt = 4
            x = np.zeros((cnt * 16, 2, k, n), dtype=np.uint64)
            d_x = E.upload(x); d_y = E.alloc(x.nbytes)
            for (xf, yf, dbc) in [r + (16,) for r in ref] + [(2, 2, last + 1), (2, 2, 13)]:
                d_w = E.alloc(E.square_pool_relin_work_bytes(1, 1, xf, yf, 1, 1, xf, yf, dbc))
                d_evk = E.alloc(E.L.crc_evk_words(E.c, dbc) * 8)
                rc = E.L.crc_square_pool_relin_forms(E.c, E.p(d_x), ca.COEFF, 1, 1, xf, yf, 1, 1, xf, yf, E.p(d_evk), dbc, None, E.p(d_y), ca.COEFF,
                                                     E.p(d_w), E.stream)
                assert rc == UNSUP, (n, k, xf, yf, dbc, rc)
                d_w.free(); d_evk.free()
            # invalid decomposition bit counts: refused as arguments, and every size query is 0
            d_w = E.alloc(1 << 20); d_evk = E.alloc(1 << 20)
            for dbc in (0, -1, 61, 64):
                assert E.L.crc_evk_words(E.c, dbc) == 0 and E.L.crc_seal_evk_bytes(E.c, dbc) == 0
                assert E.square_relin_work_bytes(4, dbc) == 0 and E.square_pool_relin_work_bytes(1, 1, 2, 2, 1, 1, 2, 2, dbc) == 0
                assert not E.square_pool_relin_supported(2, 2, dbc)
                assert E.L.crc_relinearize(E.c, E.p(d_x), 1, E.p(d_evk), dbc, E.p(d_y), E.p(d_w), E.stream) == INVAL, dbc
                assert E.L.crc_square_relin_forms(E.c, E.p(d_x), ca.COEFF, 1, E.p(d_evk), dbc, E.p(d_y), ca.COEFF, E.p(d_w), E.stream) == INVAL, dbc
                assert E.L.crc_square_pool_relin_forms(E.c, E.p(d_x), ca.COEFF, 1, 1, 2, 2, 1, 1, 2, 2, E.p(d_evk), dbc, None, E.p(d_y), ca.COEFF,
                                                       E.p(d_w), E.stream) == INVAL, dbc
            # D = 54 digit polynomials: more than either path sums
            if (n, k) == (16384, 8):
                d_w9 = E.alloc(E.square_relin_work_bytes(1, 9)); d_evk9 = E.alloc(E.L.crc_evk_words(E.c, 9) * 8)
                assert E.L.crc_relinearize(E.c, E.p(d_x), 1, E.p(d_evk9), 9, E.p(d_y), E.p(d_w9), E.stream) == UNSUP
                E.sync()
        finally:
            E.close()
