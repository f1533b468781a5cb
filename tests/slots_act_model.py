"""Independent model of the client-side activation of slot-batched networks (ReLU with an optional cap, max pooling over a window of plaintext rows), in Python
integers.  act_value / act_rows are built from slots_model.compose / decompose; ledger and network_forward are slots_rescale_model's with the kinds `client_relu`
and `client_maxpool` added (that file is shared with the older tests and stays as it is: the new kinds are handled here, stretches of other layers go through it)."""
import numpy as np

import slots_rescale_model as rm
from slots_model import compose, decompose

CLIENT = ("client_relu", "client_maxpool")


def act_value(m, D, relu, cap):
    """what the client makes of a window's centred maximum m: floor(m / D + 1/2), ReLU, cap (0: none)"""
    r = (m + (D >> 1)) // D
    if relu:
        r = max(r, 0)
    if cap:
        r = min(r, cap)
    return r


def out_dims(window):
    xd, yd, xs, ys, xf, yf = window
    return (xd - xf) // xs + 1, (yd - yf) // ys + 1


def act_slots(v, planes, window, D, relu, cap, divide_first=False):
    """v: centred slot values [planes][xd][yd][n] (nested lists) -> [planes][xo][yo][n].  divide_first: every value is rescaled on its own and the maximum taken
    behind the division (rounding is non-decreasing, so both orders agree)"""
    xd, yd, xs, ys, xf, yf = window
    xo, yo = out_dims(window)
    n = len(v[0][0][0])
    out = []
    for pl in range(planes):
        plane = []
        for i in range(xo):
            row = []
            for j in range(yo):
                cells = [v[pl][i * xs + a][j * ys + b] for a in range(xf) for b in range(yf)]
                if divide_first:
                    row.append([act_value(max(rm.rescale_value(c[s], D) for c in cells), 1, relu, cap) for s in range(n)])
                else:
                    row.append([act_value(max(c[s] for c in cells), D, relu, cap) for s in range(n)])
            plane.append(row)
        out.append(plane)
    return out


def act_rows(p, planes, window, n, t, D, relu, cap):
    """plaintext rows [planes * xd * yd][n] (any words, taken mod t) -> the rows [planes * xo * yo][n] crc_slots_act is defined to give (O(n^2) a row)"""
    xd, yd = window[0], window[1]
    v = [[[decompose([int(c) % t for c in p[(pl * xd + i) * yd + j]], n, t) for j in range(yd)] for i in range(xd)] for pl in range(planes)]
    r = act_slots(v, planes, window, D, relu, cap)
    return [compose(cell, n, t) for plane in r for row in plane for cell in row]


def cap_units(a):
    """`cap C` of a description line in slot units of the scale 2^bits behind the layer: nearbyint(C 2^bits); 0 without a cap"""
    return 0 if a.get("cap") is None else int(np.rint(a["cap"] * float(1 << a["bits"])))


def _as_rescale(layers):
    return [("rescale", name, dict(bits=a["bits"])) if kind in CLIENT else (kind, name, a) for kind, name, a in layers]


def ledger(layers, input_bits, weight_bits):
    """slots_rescale_model.ledger with the two client kinds: they set the scale exactly as `rescale` does"""
    return rm.ledger(_as_rescale(layers), input_bits, weight_bits)


def network_forward(layers, weights, images, t, input_bits, weight_bits):
    """slots_rescale_model.network_forward with the two client kinds: centred outputs [S][outputs] and the final scale.  The stretches of other layers between
    client layers run through that function as it is.  A stretch behind a client layer starts from integers r at the scale 2^bits; it is entered with the
    float32 images r / 2^bits and input_bits = bits, which quantise back to r exactly while |r| < 2^24 (asserted: float32 carries 24 bits)"""
    from numpy.lib.stride_tricks import sliding_window_view
    from crcnn_amd import netrun
    layers = list(layers)
    scales = ledger(layers, input_bits, weight_bits)
    x, bits, start = np.asarray(images, dtype=np.float32), input_bits, 0
    shape = tuple(x.shape[1:])
    for at in [i for i, (k, _, _) in enumerate(layers) if k in CLIENT] + [len(layers)]:
        flat, scale = rm.network_forward(layers[start:at], weights, x, t, bits, weight_bits)
        assert scale == scales[at]
        if at == len(layers):
            return flat, scale
        for kind, _, a in layers[start:at]:
            shape = netrun.out_shape(kind, a, shape)
        kind, _, a = layers[at]
        v = np.array(flat, dtype=object).reshape((len(flat),) + shape)
        D, cap = scale >> a["bits"], cap_units(a)
        if kind == "client_maxpool":
            v = sliding_window_view(v, (a["xf"], a["yf"]), axis=(2, 3))[:, :, ::a["xs"], ::a["ys"]].max(axis=(4, 5))
        relu = True if kind == "client_relu" else a["relu"]
        r = np.vectorize(lambda z: act_value(int(z), D, relu, cap), otypes=[object])(v)
        assert all(abs(int(z)) < 1 << 24 for z in r.reshape(-1))
        bits, start, shape = a["bits"], at + 1, tuple(r.shape[1:])
        x = (r.astype(np.float64) / float(1 << bits)).astype(np.float32)
