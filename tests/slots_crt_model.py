"""Independent model of slot batching over several plain moduli in Python integers: the Chinese-remainder lift of r residues to the integer mod T = t_0 ... t_{r-1},
its centring, the client's division floor(V / D + 1/2) with ReLU and cap, and the residues of the result.  The lift is the textbook sum over M_j = T / t_j, not the
mixed-radix recurrence the engine runs; nothing here shares code with it."""


def product(ts):
    T = 1
    for t in ts:
        T *= int(t)
    return T


def centre(v, T):
    v %= T
    return v - T if v > (T - 1) // 2 else v


def crt_lift(residues, ts):
    """the centred integer mod T with the given residues (any integers, taken mod t_j)"""
    T = product(ts)
    x = 0
    for a, t in zip(residues, ts):
        t = int(t)
        M = T // t
        x += int(a) % t * M * pow(M % t, t - 2, t)
    return centre(x, T)


def act_value(V, D, relu=0, cap=0):
    """floor(V / D + 1/2): floor division, ties towards +infinity; then max(., 0) if relu; then min(., cap) if cap"""
    rho = (2 * V + D) // (2 * D)
    if relu:
        rho = max(rho, 0)
    if cap:
        rho = min(rho, cap)
    return rho


def residues(v, ts):
    """centred residues of the integer v mod every t_j"""
    return [centre(v, int(t)) for t in ts]


def decompose(slot_rows, ts):
    """slot_rows[j][i]: slot i mod t_j (any representative) -> the centred integers mod T"""
    return [crt_lift([row[i] for row in slot_rows], ts) for i in range(len(slot_rows[0]))]


def act(slot_rows, ts, D, relu=0, cap=0):
    """slot_rows as decompose's -> [r][slots] centred residues of act_value of the lifted integers"""
    rho = [act_value(V, D, relu, cap) for V in decompose(slot_rows, ts)]
    return [[centre(v, int(t)) for v in rho] for t in ts]
