"""Key-switching keys of a lower level derived from the upper level's, in Python integers.  TEST INFRASTRUCTURE ONLY.

A key over the gadget moduli key_q = (q_0 .. q_{K-1}), Q = prod key_q, holds for pair p = (l, d)
    first = -(A s + e) + E w,   second = A,   E = (Q / q_l) 2^(dbc d) mod Q,
and E is non-zero in residue row l alone.  Over the level q_0 .. q_{k-1}, k < K, the identity holds as it stands (q_0 .. q_{k-1} divides Q): pairs with l >= k
carry E = 0, the rest are the first Sum_{l < k} L_l pairs, rows [0, k) of each polynomial.  The key switch cuts digit (l, d) from [c (Q / q_l)^-1]_{q_l}.

Here: the gadget factors and pre-scale constants of a key-modulus list, restriction by slicing, and a key switch that takes the key blob and the pre-scale
constants as arguments (the one of galois_model.GaloisModel.apply has the level's own constants built in)."""
import numpy as np

from bfv_multiply_model import negacyclic_product
from galois_model import digits, sigma_row
from mod_switch_model import product


def gadget_factors(key_q, k, dbc):
    """[(l, d, (Q_key / q_l) 2^(dbc d) mod q_l)] for l < k in the blob's order"""
    out = []
    for l in range(k):
        ql = int(key_q[l])
        f = product([int(v) for j, v in enumerate(key_q) if j != l]) % ql
        for d in range(digits(ql, dbc)):
            out.append((l, d, f * pow(2, dbc * d, ql) % ql))
    return out


def prescale(key_q, k):
    """[(Q_key / q_l)^-1 mod q_l] for l < k: what a polynomial is multiplied by before its digits are cut"""
    out = []
    for l in range(k):
        ql = int(key_q[l])
        out.append(pow(product([int(v) for j, v in enumerate(key_q) if j != l]) % ql, -1, ql) if len(key_q) > 1 else 1)
    return out


def pairs(q, k, dbc):
    return sum(digits(int(q[l]), dbc) for l in range(k))


def restrict(blobs, n, q, kept, dbc):
    """blobs [..][P][2][k][n] of the moduli q (any leading shape, flat rows accepted) -> [..][P'][2][kept][n] flattened per key: numpy slicing"""
    k = len(q)
    P, Pk = pairs(q, k, dbc), pairs(q, kept, dbc)
    b = np.asarray(blobs, dtype=np.uint64).reshape(-1, P, 2, k, n)
    return np.ascontiguousarray(b[:, :Pk, :, :kept, :]).reshape(b.shape[0], Pk * 2 * kept * n)


def key_coeff(O, key, dbc):
    """a key blob of the oracle's context (k moduli, pairs(q, k, dbc) pairs) -> [(first[k][n], second[k][n])] per pair, coefficient form, python ints"""
    n, k = O.n, O.k
    q = [int(v) for v in O.q]
    P = pairs(q, k, dbc)
    key = np.asarray(key, dtype=np.uint64).reshape(P, 2, k, n)
    return [tuple([[int(v) for v in O.ntt_inv(j, key[p, poly, j])] for j in range(k)] for poly in range(2)) for p in range(P)]


def key_switch(O, poly, key, pre, dbc=16, kc=None):
    """poly [k][n] coefficient form -> (acc0, acc1) [k][n] python ints:  Sum_{l, d} digit_{l,d}(poly[l] pre[l] mod q_l) * (first_{l,d}, second_{l,d}) mod q_j"""
    n, k = O.n, O.k
    q = [int(v) for v in O.q]
    kc = kc if kc is not None else key_coeff(O, key, dbc)
    acc = [[np.zeros(n, dtype=object) for _ in range(k)] for _ in range(2)]
    p = 0
    for l in range(k):
        pm = [int(v) * pre[l] % q[l] for v in poly[l]]
        for d in range(digits(q[l], dbc)):
            dig = [(v >> (dbc * d)) & ((1 << dbc) - 1) for v in pm]
            first, second = kc[p]; p += 1
            for j in range(k):
                acc[0][j] = acc[0][j] + negacyclic_product(dig, first[j], q[j])
                acc[1][j] = acc[1][j] + negacyclic_product(dig, second[j], q[j])
    return [[[int(v) % q[j] for v in acc[c][j]] for j in range(k)] for c in range(2)]


def relinearize(O, ct3, key, pre, dbc=16):
    """ct3 [3][k][n] coefficient form -> (c0, c1) + key_switch(c2)"""
    k = O.k
    q = [int(v) for v in O.q]
    a = key_switch(O, np.asarray(ct3)[2], key, pre, dbc)
    out = np.zeros((2, k, O.n), dtype=np.uint64)
    for c in range(2):
        for j in range(k):
            out[c, j] = np.array([(int(x) + y) % q[j] for x, y in zip(np.asarray(ct3)[c, j], a[c][j])], dtype=np.uint64)
    return out


def apply_galois(O, ct, g, key, pre, dbc=16):
    """ct [2][k][n] coefficient form -> (sigma_g(c0), 0) + key_switch(sigma_g(c1)) with the key of g"""
    k = O.k
    q = [int(v) for v in O.q]
    ct = np.asarray(ct, dtype=np.uint64)
    if g == 1:
        return ct.copy()
    t0 = [sigma_row(ct[0, i], g, q[i]) for i in range(k)]
    t1 = [sigma_row(ct[1, i], g, q[i]) for i in range(k)]
    a = key_switch(O, t1, key, pre, dbc)
    out = np.zeros((2, k, O.n), dtype=np.uint64)
    for j in range(k):
        out[0, j] = np.array([(x + y) % q[j] for x, y in zip(t0[j], a[0][j])], dtype=np.uint64)
        out[1, j] = np.array(a[1][j], dtype=np.uint64)
    return out
