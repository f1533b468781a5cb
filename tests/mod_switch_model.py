"""Modulus switching in Python integers: the definition of include/crcnn_hip.h (CRT composition, the iterated rounded division, the reduction mod q_to), the
residue form the kernels compute, the noise bound, and the row transforms around them for the NTT-form sides.  Nothing here is fast."""
from fractions import Fraction
from functools import lru_cache, reduce


def product(xs):
    return reduce(lambda a, b: a * b, xs, 1)


@lru_cache(maxsize=None)
def crt_weights(q):
    """(prod q, the integers that are 1 mod q_i and 0 mod the others)"""
    Q = product(q)
    return Q, tuple((Q // qi) * pow(Q // qi, -1, qi) for qi in q)


def crt_compose(residues, q):
    """the integer in [0, prod q) with these residues"""
    Q, w = crt_weights(tuple(q))
    return sum(int(r) * wi for r, wi in zip(residues, w)) % Q


def switch_integer(c, q, kept):
    """c in [0, prod q) -> the coefficient over the first `kept` moduli: drop the moduli last to first, rounding each division to nearest (ties up)"""
    for p in reversed(q[kept:]):
        c = (c + (p >> 1)) // p
    return c % product(q[:kept])


def switch_rows(rows, q, kept):
    """the definition: rows [k][n] (coefficient form) -> [kept][n]"""
    n = len(rows[0])
    out = [[0] * n for _ in range(kept)]
    for s in range(n):
        c = switch_integer(crt_compose([rows[i][s] for i in range(len(q))], q), q, kept)
        for i in range(kept):
            out[i][s] = c % q[i]
    return out


def switch_rows_residues(rows, q, kept):
    """the same in residues: the centred remainder of the last row, subtracted from every row below it, which is then divided by the dropped modulus"""
    rows = [[int(v) for v in r] for r in rows]
    for top in range(len(q) - 1, kept - 1, -1):
        p = q[top]; h = p >> 1
        for s in range(len(rows[0])):
            r = (rows[top][s] + h) % p - h
            for i in range(top):
                rows[i][s] = (rows[i][s] - r) * pow(p, -1, q[i]) % q[i]
    return rows[:kept]


def switch_rows_correction(rows, q, kept):
    """... and with one correction per kept row: c'_i = (c_i - R) P^-1, R = r_1 + p_1 r_2 + p_1 p_2 r_3 + ...; only the dropped rows are updated one by one"""
    k = len(q)
    drop = [[int(v) for v in rows[i]] for i in range(kept, k)]
    n = len(rows[0])
    R = [0] * n
    scale = 1
    for top in range(k - 1, kept - 1, -1):
        p = q[top]; h = p >> 1
        for s in range(n):
            r = (drop[top - kept][s] + h) % p - h
            R[s] += scale * r
            for i in range(kept, top):
                drop[i - kept][s] = (drop[i - kept][s] - r) * pow(p, -1, q[i]) % q[i]
        scale *= p
    return [[(int(rows[i][s]) - R[s]) * pow(scale, -1, q[i]) % q[i] for s in range(n)] for i in range(kept)]


def budget_bound(b_from, t, n, q_to):
    """a ciphertext with b_from bits under `from` keeps at least floor(-log2(2^-b_from + t (n + 1) / q_to)) bits.  The switch moves every coefficient of c0 and
    c1 by less than (1 + 1/p) / 2; under a ternary key c0 + c1 s moves by less than (n + 1) (1 + 1/p) / 2 < n + 1 per coefficient, which is t (n + 1) / q_to in
    invariant noise.  The budget measurement floors two bit counts, so a test allows 2 bits under this"""
    v = Fraction(1, 1 << b_from) + Fraction(t * (n + 1), q_to)
    bits = 0
    while v * 2 <= 1:                 # floor(-log2 v) for v <= 1
        v *= 2; bits += 1
    return bits


# ---- the row transforms (SEAL's negacyclic Harvey butterflies on the context's own tables: crc_ctx_table "root_powers:i" / "inv_root_powers_div_two:i") --------
def ntt_fwd(row, rp, q):
    a = [int(v) for v in row]; n = len(a)
    t, m = n, 1
    while m < n:
        t >>= 1
        for i in range(m):
            W = int(rp[m + i]); j1 = 2 * i * t
            for j in range(j1, j1 + t):
                U, V = a[j], a[j + t] * W % q
                a[j], a[j + t] = (U + V) % q, (U - V) % q
        m <<= 1
    return a


def ntt_inv(row, irp2, q):
    a = [int(v) for v in row]; n = len(a)
    half = (q + 1) >> 1
    t, m = 1, n
    while m > 1:
        h = m >> 1; j1 = 0
        for i in range(h):
            W = int(irp2[h + i])
            for j in range(j1, j1 + t):
                U, V = a[j], a[j + t]
                a[j], a[j + t] = (U + V) * half % q, (U - V) * W % q
            j1 += 2 * t
        t <<= 1; m >>= 1
    return a
