"""Independent model of slot batching in Python integers: the minimal primitive 2n-th root of unity mod t, slots as evaluations of the plaintext polynomial
(slot i = p(psi^(3^i)), slot n/2 + i = p(psi^(-3^i))), and the slot-wise integer arithmetic a batched ciphertext must carry.  Nothing here shares code with the
engine: no transform, no index map, no tables."""


def is_prime(n):
    if n < 2:
        return False
    i = 2
    while i * i <= n:
        if n % i == 0:
            return False
        i += 1
    return True


def minimal_root(n, t):
    """numerically smallest primitive 2n-th root of unity mod t (t prime, t = 1 mod 2n)"""
    assert (t - 1) % (2 * n) == 0
    e = (t - 1) // (2 * n)
    g = 2
    while True:
        c = pow(g, e, t)
        if pow(c, n, t) == t - 1:
            break
        g += 1
    # every primitive 2n-th root is an odd power of c
    best, cur, sq = c, c, c * c % t
    for _ in range(n):
        best = min(best, cur)
        cur = cur * sq % t
    return best


def slot_points(n, t):
    """the n evaluation points: psi^(3^i) for slots 0 .. n/2 - 1, psi^(-3^i) for slots n/2 .. n - 1"""
    psi = minimal_root(n, t)
    m = 2 * n
    pts, neg = [], []
    e = 1
    for _ in range(n // 2):
        pts.append(pow(psi, e, t)); neg.append(pow(psi, m - e, t))
        e = e * 3 % m
    return pts + neg


def centre(v, t):
    v %= t
    return v - t if v > (t - 1) // 2 else v


def evaluate(p, x, t):
    r = 0
    for c in reversed(p):
        r = (r * x + int(c)) % t
    return r


def decompose(p, n, t, slots=None):
    """centred slot values of the coefficient list p (Horner at every point: O(n^2), for n up to about 1024)"""
    pts = slot_points(n, t)
    return [centre(evaluate(p, x, t), t) for x in pts[: n if slots is None else slots]]


def compose(values, n, t):
    """coefficients of the unique polynomial of degree < n with the given slots (missing slots are zero): interpolation through the adjoint evaluation
    p_j = n^-1 sum_i v_i x_i^-j -- the x_i are the n roots of X^n + 1, for which sum_i x_i^(j - l) = n [j == l]"""
    pts = slot_points(n, t)
    v = [int(x) % t for x in values] + [0] * (n - len(values))
    ninv = pow(n, t - 2, t)
    out = []
    xinv = [pow(x, t - 2, t) for x in pts]
    cur = [1] * n
    for _ in range(n):
        out.append(sum(a * b for a, b in zip(v, cur)) % t * ninv % t)
        cur = [a * b % t for a, b in zip(cur, xinv)]
    return out


def slots_prime(n, bits):
    """largest prime below 2**bits that is 1 mod 2n, by trial"""
    c = (1 << bits) - 1
    while c > 2 * n:
        if c % (2 * n) == 1 and is_prime(c):
            return c
        c -= 1
    return None


# ---- the quantised integer network a slot-batched forward must compute, slot by slot, mod t ------------------------------------------------------------------
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
        if s >= 1 << 62 or int(float(s)) != s:
            raise ValueError("scale out of range")
    return out + [s]


def quantise(values, scale):
    """nearbyint(double(v) * scale), round half even, as Python integers (object array of the same shape)"""
    import numpy as np
    v = np.asarray(values, dtype=np.float64) * float(scale)
    return np.vectorize(lambda x: int(round(x)), otypes=[object])(v) if v.size else v.astype(object)


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
        else:
            raise ValueError(kind)
    flat = x.reshape(x.shape[0], -1)
    half = (t - 1) // 2
    return [[int(v) - t if int(v) > half else int(v) for v in row] for row in flat], scales[-1]
