"""The hoisted rotation H_g and the diagonal matrix-vector product restated in Python integers, on top of tests/galois_model.py.  TEST INFRASTRUCTURE ONLY.

    K'_g = sigma_g^-1(K_g): sigma_{g^-1 mod 2n} of every polynomial of the key blob of g
    H_g(ct) = sigma_g( (c0, 0) + KeySwitch(c1; K'_g) )

The model keeps no key switch of its own.  GaloisModel.apply(x, g, key) is (sigma_g(x0), 0) + KeySwitch(sigma_g(x1); key), so with x = sigma_{g^-1}(ct) it is
exactly the bracket above, and H_g(ct) = sigma_g(apply(sigma_{g^-1}(ct), g, K'_g)).  Keys are conjugated in coefficient form through the oracle's transforms --
the definition, not the engine's index table.
"""
import numpy as np

import galois_model as gm


def inv_elt(n, g):
    return pow(int(g), -1, 2 * n)


def ntt_sigma_rows(O, rows, g):
    """NTT(sigma_g(INTT(rows))) of NTT-form rows [..][k][n] with the oracle's transforms: the definition of the NTT-domain automorphism"""
    rows = np.asarray(rows, dtype=np.uint64)
    flat = rows.reshape(-1, O.k, O.n)
    out = np.empty_like(flat)
    for r in range(flat.shape[0]):
        for j in range(O.k):
            c = O.ntt_inv(j, np.ascontiguousarray(flat[r, j]))
            out[r, j] = O.ntt_fwd(j, np.array(gm.sigma_row(c, g, int(O.q[j])), dtype=np.uint64))
    return out.reshape(rows.shape)


def conjugate_key(O, key, g):
    """K'_g from the blob of g, by the definition"""
    key = np.asarray(key, dtype=np.uint64)
    return ntt_sigma_rows(O, key.reshape(-1, O.k, O.n), inv_elt(O.n, g)).reshape(-1)


def conjugate_key_coeff(M, kc, g):
    """the same on GaloisModel.key_coeff's coefficient-form dictionary"""
    h = inv_elt(M.n, g)
    return {ld: tuple([gm.sigma_row(poly[j], h, M.q[j]) for j in range(M.k)] for poly in pair) for ld, pair in kc.items()}


def hoisted(M, ct, g, ckey, dbc=16, key_coeff=None):
    """ct [2][k][n] canonical coefficient form -> H_g(ct) with the CONJUGATED key blob (or its coefficient form); g = 1: the ciphertext itself"""
    ct = np.asarray(ct, dtype=np.uint64)
    if g == 1:
        return ct.copy()
    pre = np.stack([gm.sigma_rows_np(ct[p], inv_elt(M.n, g), M.q) for p in range(2)])
    z = M.apply(pre, g, ckey, dbc, key_coeff=key_coeff)
    return np.stack([gm.sigma_rows_np(z[p], g, M.q) for p in range(2)])


def matvec(W, x, t):
    """W x mod t in Python integers"""
    return [sum(int(w) * int(v) for w, v in zip(row, x)) % t for row in W]


def diag_matvec_slots(steps, rows, x_slots, t):
    """Sum_r rows[r] (.) rotate_rows(x, steps[r]) mod t on integer slot vectors [n], in Python integers"""
    n = len(x_slots)
    acc = [0] * n
    for d, row in zip(steps, rows):
        rot = gm.rotate_rows_slots(np.asarray(x_slots, dtype=object), d)
        acc = [(a + int(p) * int(v)) % t for a, p, v in zip(acc, row, rot)]
    return acc
