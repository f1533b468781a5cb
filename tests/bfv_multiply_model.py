"""Evaluator::multiply of SEAL 2.3.1 (evaluator.cpp:356-700) for size-2 ciphertexts, restated in Python integers.  TEST INFRASTRUCTURE ONLY.

An independent reference for the engine's ciphertext x ciphertext multiply: it shares no code with the oracle's square (and does not call it).  It takes two
things from the oracle, its tables `q` and `bsk` -- SEAL's own auxiliary base B U {m_sk} --, and derives every other BEHZ constant from them as a modular
inverse or a product.  Where SEAL sums residues lazily and reduces, the model keeps the integer the sum stands for and reduces that: the same residue.

    step 0/1  fastbconv_mtilde + mont_rq   c' = (S + q r) / m~,  S = Sum_i |x m~ (q/q_i)^-1|_{q_i} (q/q_i),  r = -S q^-1 mod m~      (m~ = 2^32)
    step 2    the tensor product (ac, ad + bc, bd) in q and in Bsk (SEAL: Karatsuba for the middle term, the same residue)
    step 3    x t, fast_floor            (x_Bsk - fastbconv(x_q)) q^-1 mod Bsk
    step 4    fastbconv_sk               back to q, corrected by alpha from the residue mod m_sk

Ring products are formed by Kronecker substitution, one big-integer product per modulus, so n = 16384 takes seconds.
"""
import numpy as np

M_TILDE = 1 << 32


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _pack(v, width):
    """coefficients (python ints below 2^(8 width)) -> the integer Sum_s v[s] 2^(8 width s)"""
    n = len(v)
    buf = np.zeros((n, width), dtype=np.uint8)
    lo = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in v], dtype=np.uint64)
    buf[:, :8] = lo.view(np.uint8).reshape(n, 8)
    hi = np.array([int(x) >> 64 for x in v], dtype=np.uint64)          # (sums of two residues: one more bit)
    buf[:, 8:16] = hi.view(np.uint8).reshape(n, 8)
    return int.from_bytes(buf.tobytes(), "little")


def _unpack(z, count, width):
    raw = np.frombuffer(z.to_bytes(count * width, "little"), dtype=np.uint8).reshape(count, width)
    out = np.zeros(count, dtype=object)
    for w0 in range(0, width, 8):
        chunk = np.zeros((count, 8), dtype=np.uint8)
        w1 = min(w0 + 8, width)
        chunk[:, :w1 - w0] = raw[:, w0:w1]
        out = out + (chunk.reshape(-1).view(np.uint64).astype(object) << (8 * w0))
    return out


def negacyclic_product(a, b, m):
    """a b mod (x^n + 1, m) for coefficient vectors of python ints below 2 m"""
    n = len(a)
    width = (2 * (int(m).bit_length() + 1) + n.bit_length() + 7) // 8 + 1
    if width < 17:
        width = 17
    z = _unpack(_pack(a, width) * _pack(b, width), 2 * n, width)
    return (z[:n] - z[n:]) % m


class MultiplyModel:
    def __init__(self, oracle):
        self.n, self.k, self.t = oracle.n, oracle.k, int(oracle.t)
        self.q = [int(v) for v in oracle.table("q")]
        bsk = [int(v) for v in oracle.table("bsk")]
        self.B, self.msk = bsk[:-1], bsk[-1]
        self.bsk = bsk
        self.Q = 1
        for v in self.q:
            self.Q *= v
        self.M = 1
        for v in self.B:
            self.M *= v
        self.qhat = [self.Q // v for v in self.q]
        self.mhat = [self.M // v for v in self.B]

    # -- per-polynomial base conversions: residues are lists of object arrays
    def _lift(self, xq):
        """steps 0 and 1: base q -> Bsk"""
        S = 0
        for i, qi in enumerate(self.q):
            tr = xq[i] * (M_TILDE * pow(self.qhat[i], -1, qi) % qi) % qi
            S = S + tr * self.qhat[i]
        r = (-(S % M_TILDE) * pow(self.Q, -1, M_TILDE)) % M_TILDE
        c = (S + self.Q * r) // M_TILDE
        return [c % m for m in self.bsk]

    def _floor_back(self, xq, xb):
        """steps 3 and 4 on the products (already multiplied by t): fast_floor, then fastbconv_sk"""
        S = 0
        for i, qi in enumerate(self.q):
            S = S + (xq[i] * pow(self.qhat[i], -1, qi) % qi) * self.qhat[i]
        fl = [(xb[j] - S) * pow(self.Q, -1, m) % m for j, m in enumerate(self.bsk)]
        S3 = 0
        for j, bj in enumerate(self.B):
            S3 = S3 + (fl[j] * pow(self.mhat[j], -1, bj) % bj) * self.mhat[j]
        alpha = (S3 - fl[-1]) * pow(self.M, -1, self.msk) % self.msk
        neg = alpha > (self.msk >> 1)
        corr = np.where(neg, self.M * (self.msk - alpha), -(self.M * alpha))
        return [(S3 + corr) % qi for qi in self.q]

    def multiply(self, x, y):
        """x, y: [2][k][n] uint64 coefficient-form ciphertexts -> [3][k][n] uint64"""
        k, n = self.k, self.n
        xq = [[_obj(x[p][i]) for i in range(k)] for p in range(2)]
        yq = [[_obj(y[p][i]) for i in range(k)] for p in range(2)]
        xb = [self._lift(xq[p]) for p in range(2)]
        yb = [self._lift(yq[p]) for p in range(2)]

        def tensor(a, b, c, d, m):
            ac = negacyclic_product(a, c, m); bd = negacyclic_product(b, d, m)
            mid = (negacyclic_product(a + b, c + d, m) - ac - bd) % m
            return [ac * self.t % m, mid * self.t % m, bd * self.t % m]
        pq = [tensor(xq[0][i], xq[1][i], yq[0][i], yq[1][i], m) for i, m in enumerate(self.q)]
        pb = [tensor(xb[0][j], xb[1][j], yb[0][j], yb[1][j], m) for j, m in enumerate(self.bsk)]
        out = np.zeros((3, k, n), dtype=np.uint64)
        for p in range(3):
            res = self._floor_back([pq[i][p] for i in range(k)], [pb[j][p] for j in range(len(self.bsk))])
            for i in range(k):
                out[p, i] = np.array([int(v) for v in res[i]], dtype=np.uint64)
        return out


def plain_negacyclic(a, b, t):
    """the product of two plaintext polynomials mod (x^n + 1, t), coefficient for coefficient"""
    return np.array([int(v) for v in negacyclic_product(_obj(a), _obj(b), int(t))], dtype=np.uint64)


def golden_pairs(g, O):
    """the ciphertext pairs (ct_in[i], ct_in[(i + 1) % nct]) of an op-level golden set with the plaintext polynomials under them; the one-ciphertext set gets
    a second ciphertext, encrypted by the oracle from the set's public key and second plaintext"""
    cts = np.ascontiguousarray(g["ct_in"]); msgs = np.ascontiguousarray(g["msgs"])
    if len(cts) == 1:
        cts = np.concatenate([cts, O.encrypt(np.ascontiguousarray(g["pk"]), np.ascontiguousarray(g["plains"][1]), 4242)[None]])
        msgs = np.concatenate([msgs, np.ascontiguousarray(g["plains"][1])[None]])
    nct = len(cts)
    x = cts
    y = np.ascontiguousarray(cts[[(i + 1) % nct for i in range(nct)]])
    my = np.ascontiguousarray(msgs[[(i + 1) % nct for i in range(nct)]])
    return x, y, msgs, my


_PRODUCTS = {}


def golden_products(name, g, O):
    """model(x_i, y_i) of golden_pairs, computed once per set and shared by the tests of a session; callers must not write to it"""
    if name not in _PRODUCTS:
        x, y, _, _ = golden_pairs(g, O)
        M = MultiplyModel(O)
        p = np.stack([M.multiply(x[i], y[i]) for i in range(len(x))])
        p.setflags(write=False)
        _PRODUCTS[name] = p
    return _PRODUCTS[name]
