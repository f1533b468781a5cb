"""The dense layer over channel planes restated in Python integers, on top of tests/galois_hoisted_model.py.  TEST INFRASTRUCTURE ONLY.

    u_j = Sum_c P[j][c] (*) x[c]        (a product of NTT-form rows, element by element mod q_i)
    y   = Sum_j H_{gs[j]}(u_j)

H_g is galois_hoisted_model.hoisted; the transforms are the oracle's; products and sums are Python integers mod q_i.  dense_slots is the plan's statement on
integer slot vectors (what y decrypts to), dense_direct the layer it must equal at the output slots.
"""
import numpy as np

import bsgs_model as bm
import galois_hoisted_model as hm
import galois_model as gm


def dense_planes(M, x, gs, p_ntt, key_coeffs, dbc=16):
    """x [Cin][2][k][n] canonical coefficient form, p_ntt [R][Cin][k][n] NTT-form plaintext rows, key_coeffs {g: CONJUGATED key in coefficient form} for every
    g != 1 -> y [2][k][n] coefficient form"""
    O = M.O
    p_ntt = np.asarray(p_ntt, dtype=np.uint64)
    assert p_ntt.shape == (len(gs), len(x), M.k, M.n)
    xh = [bm._transform(O, np.asarray(xc, dtype=np.uint64), True).astype(object) for xc in x]
    qq = np.array(M.q, dtype=object).reshape(1, -1, 1)
    y = None
    for j, g in enumerate(gs):
        u = np.zeros((2, M.k, M.n), dtype=object)
        for c in range(len(x)):
            u = (u + p_ntt[j, c].astype(object)[None] * xh[c]) % qq
        z = hm.hoisted(M, bm._transform(O, u.astype(np.uint64), False), g, None, dbc, key_coeff=key_coeffs.get(g))
        y = z if y is None else M.add(y, z)
    return y


def vector_slots(values, slots, n, M, junk=None):
    """values [P] at `slots` of every period M of [n] slots; the other slots 0, or junk [M]"""
    row = np.zeros(M, dtype=object) if junk is None else np.asarray(junk, dtype=object).copy()
    for v, s in zip(values, slots):
        row[s] = int(v)
    return np.tile(row, n // M)


def dense_slots(plan, rows, planes, t):
    """rows [R][Cin][n] (DensePlanesPlan.fold), planes [Cin][n] integer slots -> [n] = Sum_j rotate_rows( Sum_c rows[j][c] (.) planes[c], steps[j] ) mod t"""
    out = np.zeros(len(planes[0]), dtype=object)
    for j, s in enumerate(plan.steps):
        inner = np.zeros(len(planes[0]), dtype=object)
        for c, p in enumerate(planes):
            inner = (inner + np.asarray(rows[j][c]).astype(object) * np.asarray(p, dtype=object)) % t
        out = (out + gm.rotate_rows_slots(inner, s)) % t
    return out


def dense_direct(W, xs, t):
    """W [O][Cin][P], xs [Cin][P] -> [O]: Sum_c Sum_p W[o][c][p] xs[c][p] mod t in Python integers"""
    W = np.asarray(W).astype(object); xs = np.asarray(xs).astype(object)
    return [int((W[o] * xs).sum()) % t for o in range(W.shape[0])]
