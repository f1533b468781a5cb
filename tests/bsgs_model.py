"""The baby-step / giant-step diagonal product restated in Python integers, on top of tests/galois_hoisted_model.py.  TEST INFRASTRUCTURE ONLY.

    u_j = Sum_b P[j][b] (*) H_{gb[b]}(x)        (a product of NTT-form rows, element by element mod q_i)
    y   = Sum_j H_{gg[j]}(u_j)

H_g is galois_hoisted_model.hoisted; the transforms are the oracle's; products and sums are Python integers mod q_i.  bsgs_slots is the plan's statement on
integer slot vectors: what y decrypts to.
"""
import numpy as np

import galois_hoisted_model as hm
import galois_model as gm


def _transform(O, ct, fwd):
    """[2][k][n] canonical residues through the oracle's forward or inverse transform, row by row"""
    out = np.empty((2, O.k, O.n), dtype=np.uint64)
    for p in range(2):
        for i in range(O.k):
            row = np.ascontiguousarray(ct[p, i], dtype=np.uint64)
            out[p, i] = O.ntt_fwd(i, row) if fwd else O.ntt_inv(i, row)
    return out


def bsgs(M, ct, gb, gg, p_ntt, key_coeffs, dbc=16):
    """ct [2][k][n] canonical coefficient form, p_ntt [G][B][k][n] NTT-form plaintext rows, key_coeffs {g: CONJUGATED key in coefficient form
    (galois_hoisted_model.conjugate_key_coeff)} for every g != 1 -> y [2][k][n] coefficient form"""
    O = M.O
    p_ntt = np.asarray(p_ntt, dtype=np.uint64)
    assert p_ntt.shape == (len(gg), len(gb), M.k, M.n)
    rot = [_transform(O, hm.hoisted(M, ct, g, None, dbc, key_coeff=key_coeffs.get(g)), True).astype(object) for g in gb]
    qq = np.array(M.q, dtype=object).reshape(1, -1, 1)
    y = None
    for j, g in enumerate(gg):
        u = np.zeros((2, M.k, M.n), dtype=object)
        for b in range(len(gb)):
            u = (u + p_ntt[j, b].astype(object)[None] * rot[b]) % qq
        z = hm.hoisted(M, _transform(O, u.astype(np.uint64), False), g, None, dbc, key_coeff=key_coeffs.get(g))
        y = z if y is None else M.add(y, z)
    return y


def bsgs_slots(baby_steps, giant_steps, rows, x_slots, t):
    """Sum_j rotate_rows( Sum_b rows[j][b] (.) rotate_rows(x, baby_steps[b]), giant_steps[j] ) mod t on an integer slot vector [n], in Python integers"""
    n = len(x_slots)
    x = np.asarray([int(v) for v in x_slots], dtype=object)
    acc = [0] * n
    for j, gs in enumerate(giant_steps):
        inner = hm.diag_matvec_slots(baby_steps, rows[j], x, t)
        rot = gm.rotate_rows_slots(np.asarray(inner, dtype=object), gs)
        acc = [(a + int(v)) % t for a, v in zip(acc, rot)]
    return acc
