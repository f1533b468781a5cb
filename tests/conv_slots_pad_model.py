"""The packed convolution with strides, zero padding, a bias and an output mask, restated in Python integers on top of tests/conv_slots_model.py.
TEST INFRASTRUCTURE ONLY.

conv_direct_geom is the convolution itself (zero padding, conv stride, a sum pool of its own window and stride, a bias per output channel and pooled output);
plane_slots_geom lays a plane out at an origin; conv_bias_mask_slots is the statement of crc_conv_slots_bias_mask_forms on integer slot vectors,

    y[co] = mask (.) ( Sum_ci Sum_tau wf[co][ci][tau] rotate_rows(x[ci], steps[tau]) + b[co] )   mod t

and bias_word the definition of the word crc_conv_slots_pack_bias returns.
"""
import numpy as np

import conv_slots_model as cm


def bias_word(b, t, qs, i):
    """every position of crc_plain_to_delta(form = NTT) of the constant plaintext c = b mod t, for modulus i of qs: floor(q / t) c + (q mod t for the upper half)
    mod q_i, q the product of qs"""
    c = int(b) % t
    q = 1
    for v in qs:
        q *= int(v)
    return ((q // t) * c + (q % t if c >= (t + 1) // 2 else 0)) % int(qs[i])


def conv_direct_geom(img, w, pad=0, stride=1, pool=1, pool_stride=None, bias=None, t=None):
    """img [Cin][H][W], w [Cout][Cin][fh][fw] -> [Cout][oh][ow]: `pad` zero pixels on every side, out(y, x) = Sum w[a][b] img(stride y + a - pad, stride x + b - pad),
    then a pool x pool sum pool of stride pool_stride (default: pool), then + bias[co]; Python integers, mod t where one is given"""
    img = np.asarray(img).astype(object); w = np.asarray(w).astype(object)
    Cout, Cin, fh, fw = w.shape
    H, W = img.shape[1:]
    ps = pool_stride or pool
    big = np.zeros((Cin, H + 2 * pad, W + 2 * pad), dtype=object)
    big[:, pad:pad + H, pad:pad + W] = img
    ch, cw = (H + 2 * pad - fh) // stride + 1, (W + 2 * pad - fw) // stride + 1
    c = np.zeros((Cout, ch, cw), dtype=object)
    for co in range(Cout):
        for ci in range(Cin):
            for a in range(fh):
                for b in range(fw):
                    c[co] += w[co, ci, a, b] * big[ci, a:a + stride * (ch - 1) + 1:stride, b:b + stride * (cw - 1) + 1:stride]
    oh, ow = (ch - pool) // ps + 1, (cw - pool) // ps + 1
    out = np.zeros((Cout, oh, ow), dtype=object)
    for u in range(pool):
        for v in range(pool):
            out += c[:, u:u + ps * (oh - 1) + 1:ps, v:v + ps * (ow - 1) + 1:ps]
    if bias is not None:
        out += np.asarray(bias).astype(object).reshape(-1, 1, 1)
    return out % t if t else out


def plane_slots_geom(plane, n, M, pitch, origin, dil, junk=None):
    """an H x W integer plane -> [n] slots: pixel (y, x) at origin + dil (y pitch + x) of every period M; the other slots 0 (a clean plane), or junk [M]"""
    plane = np.asarray(plane)
    row = np.zeros(M, dtype=object) if junk is None else np.asarray(junk, dtype=object).copy()
    for y in range(plane.shape[0]):
        for x in range(plane.shape[1]):
            row[origin + dil * (y * pitch + x)] = int(plane[y, x])
    return np.tile(row, n // M)


def conv_bias_mask_slots(plan, wf, planes, t, bias=None, mask=None):
    """wf [Cout][Cin][T] (plan.fold), planes [Cin][n] integer slots, bias [Cout] or None, mask [n] or None -> [Cout][n] mod t: the rotations and the channel mix,
    then the bias on every slot, then the mask"""
    out = cm.conv_plan_slots(plan, wf, planes, t)
    if bias is not None:
        out = (out + np.asarray(bias).astype(object).reshape(-1, 1)) % t
    if mask is not None:
        out = (out * np.asarray(mask).astype(object).reshape(1, -1)) % t
    return out
