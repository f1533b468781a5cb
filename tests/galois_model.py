"""Evaluator::apply_galois of SEAL 2.3.1 (evaluator.cpp:1587-1834) restated in Python integers, with the rotation planner and the slot statement.
TEST INFRASTRUCTURE ONLY.

    sigma_g on a coefficient row mod q (util::apply_galois, util/polyarithsmallmod.h:313-360): for each i, r = i g; out[r mod n] = in[i] where bit log2 n of r is
    clear, (q - in[i]) mod q where it is set.
    apply_galois(ct, g, key) = (sigma(c0), 0) + Sum_{l, d} digit_{l,d}(sigma(c1) (q/q_l)^-1 mod q_l) * (first_{l,d}, second_{l,d})   in Z_q[x]/(x^n + 1)

The model keeps no transform of its own: key rows come to coefficient form through the oracle's inverse transform, ring products are negacyclic_product's big-
integer ones (bfv_multiply_model.py), and the inner products are summed as integers and reduced once -- the residue SEAL's lazy 128-bit sums reduce to.
Slot statement (slot i = p(psi^(3^i)), slot n/2 + i = p(psi^(-3^i))): rotate_rows(s) puts old slot (i + s) mod n/2 at slot i of each half,
rotate_columns swaps the halves.
"""
import numpy as np

from bfv_multiply_model import negacyclic_product


def elt_valid(n, g):
    return g % 2 == 1 and 1 <= g < 2 * n


def elt_rows(n, steps):
    """0 for a step count too large"""
    if abs(steps) >= n // 2:
        return 0
    return pow(3, steps if steps >= 0 else n // 2 + steps, 2 * n)


def elt_columns(n):
    return 2 * n - 1


def default_elts(n):
    logn = n.bit_length() - 1
    out = [2 * n - 1]
    for i in range(logn - 1):
        for e in (pow(3, 1 << i, 2 * n), pow(pow(3, -1, 2 * n), 1 << i, 2 * n)):
            if e not in out:                                # SEAL keeps a map: 3^(n/4) is its own inverse and appears once
                out.append(e)
    return out


def plan(n, g, elts):
    """indices into elts, in order; None where a key is missing (evaluator.cpp:1623-1661)"""
    assert elt_valid(n, g)
    elts = [int(e) for e in elts]
    if g == 1:
        return []
    if g in elts:
        return [elts.index(g)]
    m, half = 2 * n, n // 2
    log = {}
    for o1 in range(half):                                  # Zmstar_to_generator_: g = 3^o1 (-1)^o2
        p = pow(3, o1, m)
        log[p] = (o1, 0); log[m - p] = (o1, 1)
    o1, o2 = log[g]
    gen = 3
    if bin(half - o1).count("1") < bin(o1).count("1"):
        o1, gen = half - o1, pow(3, -1, m)
    out = []
    while o1:
        if o1 & 1:
            if gen not in elts:
                return None
            out.append(elts.index(gen))
        gen = gen * gen % m
        o1 >>= 1
    if o2:
        if m - 1 not in elts:
            return None
        out.append(elts.index(m - 1))
    return out


def sigma_row(row, g, q):
    """python-int restatement of util::apply_galois on one row"""
    n = len(row)
    out = [0] * n
    for i in range(n):
        r = i * g
        v = int(row[i])
        out[r % n] = v if not (r & n) else (q - v) % q
    return out


def sigma_rows_np(x, g, q):
    """the same on numpy rows [..][k][n] with moduli q[k] (vectorised: the permute kernel's reference at n = 16384)"""
    x = np.asarray(x, dtype=np.uint64)
    n = x.shape[-1]
    i = np.arange(n, dtype=np.int64)
    r = i * int(g)
    dst = r % n
    neg = (r & n) != 0
    qq = np.asarray(q, dtype=np.uint64).reshape((-1, 1))
    negx = np.where(x == 0, np.uint64(0), qq - x)
    out = np.empty_like(x)
    out[..., dst] = np.where(neg, negx, x)
    return out


def digits(q, dbc):
    L = 0
    while q:
        L += 1
        q >>= dbc
    return L


def evk_words(n, q, dbc):
    return sum(2 * digits(int(ql), dbc) * len(q) * n for ql in q)


class GaloisModel:
    def __init__(self, oracle):
        self.O = oracle
        self.n, self.k = oracle.n, oracle.k
        self.q = [int(v) for v in oracle.q]

    def key_coeff(self, key, dbc):
        """a key blob -> {(l, d): (first[k][n], second[k][n])} in coefficient form, python ints"""
        n, k = self.n, self.k
        key = np.asarray(key, dtype=np.uint64)
        assert key.size == evk_words(n, self.q, dbc)
        out, off = {}, 0
        for l in range(k):
            for d in range(digits(self.q[l], dbc)):
                pair = []
                for _ in range(2):
                    rows = key[off:off + k * n].reshape(k, n); off += k * n
                    pair.append([[int(v) for v in self.O.ntt_inv(j, rows[j])] for j in range(k)])
                out[(l, d)] = tuple(pair)
        return out

    def apply(self, ct, g, key, dbc=16, key_coeff=None):
        """ct [2][k][n] canonical coefficient form -> apply_galois(ct, g) with the key blob of g; g = 1: the ciphertext itself"""
        n, k, q = self.n, self.k, self.q
        ct = np.asarray(ct, dtype=np.uint64)
        if g == 1:
            return ct.copy()
        kc = key_coeff if key_coeff is not None else self.key_coeff(key, dbc)
        t0 = [sigma_row(ct[0, i], g, q[i]) for i in range(k)]
        t1 = [sigma_row(ct[1, i], g, q[i]) for i in range(k)]
        acc = [[np.zeros(n, dtype=object) for _ in range(k)] for _ in range(2)]
        for l in range(k):
            qhat = 1
            for j in range(k):
                if j != l:
                    qhat = qhat * q[j] % q[l]
            inv = pow(qhat, -1, q[l]) if k > 1 else 1
            pm = [v * inv % q[l] for v in t1[l]]
            for d in range(digits(q[l], dbc)):
                dig = [(v >> (dbc * d)) & ((1 << dbc) - 1) for v in pm]
                first, second = kc[(l, d)]
                for j in range(k):
                    acc[0][j] = acc[0][j] + negacyclic_product(dig, first[j], q[j])
                    acc[1][j] = acc[1][j] + negacyclic_product(dig, second[j], q[j])
        out = np.zeros((2, k, n), dtype=np.uint64)
        for j in range(k):
            out[0, j] = np.array([(int(a) + b) % q[j] for a, b in zip(acc[0][j], t0[j])], dtype=np.uint64)
            out[1, j] = np.array([int(a) % q[j] for a in acc[1][j]], dtype=np.uint64)
        return out

    def apply_planned(self, ct, g, elts, keys, dbc=16):
        """the planner's steps one after the other; keys [n_elts][words]"""
        steps = plan(self.n, g, elts)
        assert steps is not None
        for s in steps:
            ct = self.apply(ct, int(elts[s]), keys[s], dbc)
        return np.asarray(ct, dtype=np.uint64).copy()

    def add(self, a, b):
        qq = np.array(self.q, dtype=object).reshape(1, -1, 1)
        return ((np.asarray(a).astype(object) + np.asarray(b).astype(object)) % qq).astype(np.uint64)


def rotate_rows_slots(v, steps):
    """the slot statement on integer rows [..][n]: new slot i of each half = old slot (i + steps) mod n/2"""
    v = np.asarray(v)
    h = v.shape[-1] // 2
    return np.concatenate([np.roll(v[..., :h], -steps, axis=-1), np.roll(v[..., h:], -steps, axis=-1)], axis=-1)


def rotate_columns_slots(v):
    v = np.asarray(v)
    h = v.shape[-1] // 2
    return np.concatenate([v[..., h:], v[..., :h]], axis=-1)
