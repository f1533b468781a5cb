"""The last step of BFV decryption in Python integers: SEAL's gamma-corrected scaling of v = c0 + c1 s (+ c2 s^2) by t / q (decryptor.cpp:107-236,
baseconverter.cpp:744-797), the rounding it approximates, the band around the half-integers in which the two may differ, and ciphertexts constructed so that
every input of that step is reached through the public entry points: (c0 = v, c1 = 0) decrypts with V = v exactly, whatever the secret key.  Nothing here
is fast."""
import random
from collections import namedtuple
from functools import lru_cache

import numpy as np

from mod_switch_model import ntt_fwd, ntt_inv, product

GAMMA = 0x1fffffffffc80001            # kGamma of crcnn_amd/csrc/ctx.cpp: SEAL's auxiliary prime of the correction

Constants = namedtuple("Constants", "Q yc qhat ninv_q_t ninv_q_g inv_gamma_t")
# kind: "uniform", "extreme", "rounding", "gamma" or "accumulator"; v: the integer in [0, Q) (None where the case is given as residues); res: its residues;
# m, r_gamma: what scale() makes of them
Case = namedtuple("Case", "kind v res m r_gamma")


@lru_cache(maxsize=None)
def constants(q, t):
    """the constants of one (q, t): t gamma (q/q_i)^-1 mod q_i, q/q_i, (-q)^-1 mod t and mod gamma, gamma^-1 mod t"""
    Q = product(q)
    qhat = tuple(Q // qi for qi in q)
    yc = tuple(t * GAMMA % qi * pow(h % qi, -1, qi) % qi for qi, h in zip(q, qhat))
    return Constants(Q, yc, qhat, pow(-Q % t, -1, t), pow(-Q % GAMMA, -1, GAMMA), pow(GAMMA % t, -1, t))


def scale(res, q, t):
    """residues of v -> (plaintext coefficient, r_gamma before centring)"""
    c = constants(tuple(q), t)
    S = sum(int(v) * y % qi * h for v, y, qi, h in zip(res, c.yc, q, c.qhat))          # exact, not reduced: below k q
    r_t = S % t * c.ninv_q_t % t
    r_g = S % GAMMA * c.ninv_q_g % GAMMA
    centred = r_g - GAMMA if r_g > GAMMA >> 1 else r_g
    return (r_t - centred) * c.inv_gamma_t % t, r_g


def scale_rows(rows, q, t):
    """rows [k][n] (coefficient form) -> the n plaintext coefficients"""
    cols = zip(*[[int(v) for v in r] for r in rows])
    return [scale(col, q, t)[0] for col in cols]


def true_round(v, Q, t):
    """round(t v / Q) mod t, ties up"""
    return ((2 * t * v + Q) // (2 * Q)) % t


def outside_band(v, Q, t, k):
    """t v / Q is further than (k + 1) / gamma from a half-integer: there the scaling is the rounding"""
    return abs(2 * (t * v % Q) - Q) * GAMMA > 2 * (k + 1) * Q


def residues(v, q):
    return tuple(v % qi for qi in q)


def _gamma_boundary(q, t, target):
    """v with r_gamma = target.  With a = floor(t gamma v / Q) and S = (t gamma v mod Q) + alpha Q, r_gamma = a - alpha mod gamma; where gamma t < Q the
    smallest v with a = 5 gamma + target + alpha is ceil((5 gamma + target + alpha) Q / (gamma t)), and alpha (0 .. k) is tried.  Reduced mod Q (for t < 6 it
    is above Q): that changes a by a multiple of gamma and S not at all"""
    Q = product(q)
    for alpha in range(len(q) + 1):
        for d in (0, 1, -1):
            v = (-(-(5 * GAMMA + target + alpha) * Q // (GAMMA * t)) + d) % Q
            if scale(residues(v, q), q, t)[1] == target:
                return v
    return None


@lru_cache(maxsize=None)
def cases(q, t, seed):
    """the scalar cases of one parameter set (a tuple of Case): 200 uniform values, the ends and the middle of [0, Q), five values around each of seven
    rounding boundaries, r_gamma at and just above gamma >> 1 (where they exist), and the largest accumulator"""
    q = tuple(int(p) for p in q)
    Q, k = product(q), len(q)
    rng = random.Random(seed)
    out = []

    def add(kind, v):
        v %= Q
        res = residues(v, q)
        out.append(Case(kind, v, res, *scale(res, q, t)))

    for _ in range(200):
        add("uniform", rng.randrange(Q))
    for v in (0, 1, Q - 1, Q // 2, Q // 2 + 1):
        add("extreme", v)
    for M in (0, 1, t // 2 - 1, t // 2, t - 2, t - 1, rng.randrange(t)):
        M = min(max(M, 0), t - 1)
        first = -(-(2 * M + 1) * Q // (2 * t))                     # the smallest v with t v / Q >= M + 1/2
        for d in range(-2, 3):
            add("rounding", first + d)
    if GAMMA * t < Q:
        for target in (GAMMA >> 1, (GAMMA >> 1) + 1):
            v = _gamma_boundary(q, t, target)
            assert v is not None, (q, t, target)
            add("gamma", v)
    # else (the one-modulus sets, and two moduli under t = 2^60 - 1): floor(t gamma v / Q) moves by more than 1 per unit of v, so a chosen r_gamma is in
    # general not reachable -- no such pair
    c = constants(q, t)
    res = tuple((qi - 1) * pow(y, -1, qi) % qi for qi, y in zip(q, c.yc))          # y_i = q_i - 1 for every i
    out.append(Case("accumulator", None, res, *scale(res, q, t)))
    return tuple(out)


def place(cs, q, n):
    """ciphertexts [count][2][k][n] with c1 = 0 and case j at coefficient (7 j) mod n of c0, and the plaintexts [count][n] they decrypt to"""
    cts = np.zeros((len(cs), 2, len(q), n), dtype=np.uint64)
    want = np.zeros((len(cs), n), dtype=np.uint64)
    for j, c in enumerate(cs):
        s = 7 * j % n
        cts[j, 0, :, s] = np.array(c.res, dtype=np.uint64)
        want[j, s] = c.m
    return cts, want


def uniform_rows(rng, q, lead, n):
    """canonical uniform residues [..lead..][k][n] (rng: a numpy Generator)"""
    return np.stack([rng.integers(0, qi, size=tuple(lead) + (n,), dtype=np.uint64) for qi in q], axis=-2)


def dense_case(q, n, size, rp, irp2, seed):
    """one ciphertext [1][size][k][n] of `size` polynomials (coefficient form), a non-ternary secret key [k][n] (NTT form) and the rows v [k][n] it
    decrypts through: v uniform at every coefficient, c1, c2 and the key all q_i - 1 in the NTT domain, c0_hat = NTT(v) - c1_hat s - c2_hat s^2.
    rp, irp2: the context's tables "root_powers:i" and "inv_root_powers_div_two:i" """
    k = len(q)
    v = uniform_rows(np.random.default_rng(seed), q, (), n)
    ct = np.zeros((1, size, k, n), dtype=np.uint64)
    sk = np.zeros((k, n), dtype=np.uint64)
    for i, qi in enumerate(q):
        top = qi - 1
        hat = ntt_fwd(v[i], rp[i], qi)
        for p in range(1, size):
            hat = [(h - top * pow(top, p, qi)) % qi for h in hat]
            ct[0, p, i] = np.array(ntt_inv([top] * n, irp2[i], qi), dtype=np.uint64)
        ct[0, 0, i] = np.array(ntt_inv(hat, irp2[i], qi), dtype=np.uint64)
        sk[i] = top
    return ct, sk, v
