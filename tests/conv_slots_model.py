"""The packed convolution over slots restated in Python integers, on top of tests/galois_hoisted_model.py.  TEST INFRASTRUCTURE ONLY.

    y[co] = Sum_ci Sum_tau w[i][co][ci][tau] . H_{gs[tau]}(x[ci])   mod q_i

A constant plaintext's NTT-form row holds one word at every position, so the product with it is the same scalar on every coefficient: the model stays in
coefficient form and needs no transform.  H_g is galois_hoisted_model.hoisted.  lift() is the definition of that word; conv_plan_slots is the plan's statement on
integer slot vectors (what y decrypts to), conv_direct the convolution and sum pool it must equal at the valid positions.
"""
import numpy as np

import galois_hoisted_model as hm
import galois_model as gm


def lift(w, t, q):
    """the word crc_plain_to_ntt puts at every position of the row of the constant plaintext w mod t, for the modulus q"""
    c = int(w) % t
    return (c + q - t) % q if c >= (t + 1) // 2 else c % q


def conv_slots(M, x, gs, w, key_coeffs, dbc=16):
    """x [Cin][2][k][n] canonical coefficient form, w [k][Cout][Cin][T] lifted residues, key_coeffs {g: CONJUGATED key in coefficient form} for every g != 1
    -> y [Cout][2][k][n] coefficient form"""
    w = np.asarray(w, dtype=np.uint64)
    k, Cout, Cin, T = w.shape
    assert k == M.k and Cin == len(x) and T == len(gs)
    rot = [[hm.hoisted(M, x[ci], g, None, dbc, key_coeff=key_coeffs.get(g)).astype(object) for g in gs] for ci in range(Cin)]
    qq = np.array(M.q, dtype=object).reshape(1, -1, 1)
    y = np.zeros((Cout, 2, M.k, M.n), dtype=object)
    for co in range(Cout):
        for ci in range(Cin):
            for tau in range(T):
                ws = np.array([int(w[i, co, ci, tau]) for i in range(M.k)], dtype=object).reshape(1, -1, 1)
                y[co] = (y[co] + ws * rot[ci][tau]) % qq
    return y.astype(np.uint64)


def plane_slots(plane, n, M, pitch, dil, junk=None):
    """an H x W integer plane -> [n] slots: pixel (y, x) at dil (y pitch + x) of every period M; the other slots 0, or junk [M]"""
    plane = np.asarray(plane)
    row = np.zeros(M, dtype=object) if junk is None else np.asarray(junk, dtype=object).copy()
    for y in range(plane.shape[0]):
        for x in range(plane.shape[1]):
            row[dil * (y * pitch + x)] = int(plane[y, x])
    return np.tile(row, n // M)


def conv_plan_slots(plan, wf, planes, t):
    """wf [Cout][Cin][T] (ConvSlotsPlan.fold), planes [Cin][n] integer slots -> [Cout][n] = Sum_ci Sum_tau wf . rotate_rows(planes[ci], steps[tau]) mod t"""
    wf = np.asarray(wf)
    out = np.zeros((wf.shape[0], len(planes[0])), dtype=object)
    for ci, p in enumerate(planes):
        for tau, s in enumerate(plan.steps):
            rot = gm.rotate_rows_slots(np.asarray(p, dtype=object), s)
            for co in range(wf.shape[0]):
                out[co] = (out[co] + int(wf[co, ci, tau]) * rot) % t
    return out


def conv_direct(img, w, pool, t=None):
    """img [Cin][H][W], w [Cout][Cin][fh][fw] -> [Cout][oh][ow]: the 'valid' stride-1 convolution (out(y, x) = Sum w[a][b] img(y + a, x + b)), then a pool x pool
    sum pool of stride pool; Python integers, mod t where one is given"""
    img = np.asarray(img).astype(object); w = np.asarray(w).astype(object)
    Cout, Cin, fh, fw = w.shape
    H, W = img.shape[1:]
    ch, cw = H - fh + 1, W - fw + 1
    c = np.zeros((Cout, ch, cw), dtype=object)
    for co in range(Cout):
        for ci in range(Cin):
            for a in range(fh):
                for b in range(fw):
                    c[co] += w[co, ci, a, b] * img[ci, a:a + ch, b:b + cw]
    oh, ow = ch // pool, cw // pool
    out = np.zeros((Cout, oh, ow), dtype=object)
    for u in range(pool):
        for v in range(pool):
            out += c[:, u:u + pool * oh:pool, v:v + pool * ow:pool]
    return out % t if t else out
