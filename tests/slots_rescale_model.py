"""Independent model of the slot-wise rescale and of slot-batched networks that contain `rescale` layers, in Python integers.  rescale(p, n, t, D) is built from
slots_model.decompose / compose and Python's floor division; ledger and network_forward are slots_model's layer loops with the `rescale` kind added (that file
is shared with the older tests and stays as it is)."""
from slots_model import centre, compose, decompose, quantise


def rescale_value(v, D):
    """floor(v / D + 1/2): floor division, ties towards +infinity"""
    return (v + (D >> 1)) // D


def rescale(p, n, t, D):
    """coefficients of the plaintext whose slots are the rescaled centred slots of p (O(n^2): n up to a few hundred)"""
    return compose([rescale_value(v, D) for v in decompose([int(c) % t for c in p], n, t)], n, t)


def ledger(layers, input_bits, weight_bits):
    """scale in front of every layer of a (kind, name, args) list, and behind the last one; ValueError for a scale that is no exact double below 2^62"""
    W = 1 << weight_bits
    s = 1 << input_bits
    out = []
    for kind, _, a in layers:
        out.append(s)
        if kind in ("conv", "fc", "bn"):
            s *= W
        elif kind == "avgpool":
            s *= a["xf"] * a["yf"]
        elif kind == "square":
            s *= s
        elif kind == "poly":
            s = s * s * W
        elif kind == "poly3":
            s = s * s * s * W
        elif kind == "rescale":
            target = 1 << a["bits"]
            if s < target or s % target:
                raise ValueError("rescale does not divide the scale")
            s = target
        if s >= 1 << 62 or int(float(s)) != s:
            raise ValueError("scale out of range")
    return out + [s]



def network_forward(layers, weights, images, t, input_bits, weight_bits):
    """layers: (kind, name, args) list; weights: {dataset name: float32 array}; images: [S][zd][xd][yd] floats.  Returns the centred outputs [S][outputs] of the
    integer network mod t and the final scale.  int64 arithmetic while every product sum stays below 2^62, Python integers otherwise"""
    import numpy as np
    from numpy.lib.stride_tricks import sliding_window_view
    small = t < (1 << 25)
    dt = np.int64 if small else object

    def q(values, scale):
        return (quantise(values, scale) % t).astype(dt)
    scales = ledger(layers, input_bits, weight_bits)
    W = 1 << weight_bits
    x = q(np.asarray(images, dtype=np.float32), 1 << input_bits)
    for (kind, name, a), s in zip(layers, scales):
        if kind in ("conv", "fc"):
            if kind == "fc":
                x = x.reshape(x.shape[0], a["in_dim"], 1, 1)
                w = q(weights[name + ".weight"], W).reshape(a["out_dim"], a["in_dim"], 1, 1)
                xs = ys = 1
            else:
                w = q(weights[name + ".weight"], W).reshape(a["nf"], a["zd"], a["xf"], a["yf"])
                xs, ys = a["xs"], a["ys"]
            b = q(weights[name + ".bias"], s * W)
            p = sliding_window_view(x, w.shape[2:], axis=(2, 3))[:, :, ::xs, ::ys]                     # [S][zd][xo][yo][xf][yf]
            y = np.tensordot(p, w, axes=([1, 4, 5], [1, 2, 3]))                                        # [S][xo][yo][nf]
            x = (np.moveaxis(y, 3, 1) + b.reshape(1, -1, 1, 1)) % t
        elif kind in ("pool", "avgpool"):
            p = sliding_window_view(x, (a["xf"], a["yf"]), axis=(2, 3))[:, :, ::a["xs"], ::a["ys"]]
            x = p.sum(axis=(4, 5)) % t
        elif kind == "bn":
            inv = np.float32(1.0 / np.sqrt(np.asarray(weights[name + ".running_var"]).astype(np.float64) + 0.00001))
            m = q(weights[name + ".running_mean"], s).reshape(1, -1, 1, 1)
            x = (x - m) % t * q(inv, W).reshape(1, -1, 1, 1) % t
        elif kind == "pad":
            x = np.pad(x, ((0, 0), (0, 0), (a["px"], a["px"]), (a["py"], a["py"])))
        elif kind == "square":
            x = x * x % t
        elif kind == "poly":
            c2, c1, c0 = (int(q([a["c2"]], W)[0]), int(q([a["c1"]], W * s)[0]), int(q([a["c0"]], W * s * s)[0]))
            x = ((x * x % t * c2 + x * c1) % t + c0) % t
        elif kind == "poly3":
            c3, c2, c1, c0 = (int(q([a[k]], W * s ** i)[0]) for i, k in enumerate(("c3", "c2", "c1", "c0")))
            x2 = x * x % t
            x = ((x2 * x % t * c3 + x2 * c2) % t + x * c1 + c0) % t
        elif kind == "rescale":
            D = s >> a["bits"]
            x = (np.vectorize(lambda v: rescale_value(centre(int(v), t), D) % t, otypes=[object])(x)).astype(dt)
        else:
            raise ValueError(kind)
    flat = x.reshape(x.shape[0], -1)
    half = (t - 1) // 2
    return [[int(v) - t if int(v) > half else int(v) for v in row] for row in flat], scales[-1]
