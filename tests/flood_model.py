"""Noise flooding in Python integers: the definition of include/crcnn_hip.h (crc_flood*).  Its only input is the raw ChaCha20 keystream, taken block by block
through crc_chacha20_block; the sample layout (csrc/chacha.h, CHACHA_DOM_FLOOD), x -> e1, the residues, the products through the context's own transform tables
(mod_switch_model's butterflies), the admission rule, crc_flood_bits and the two budget bounds are all here.  Nothing here is fast.

The two budget bounds.  `bits(v)` is the bit length, Lq = bits(q); the budget of a ciphertext is Lq - bits(max |t w|) - 1 with w the noise polynomial of
c0 + c1 s = Delta m + w and |t w| < q / 2.

Lower bound (budget_lower).  A budget of b bits says |t w| < 2^(Lq - b - 1) <= q 2^-b.  The flood adds w' = e1 - e_pk u + e2 s with |e1| <= 2^B and, under ternary
u and s and errors in [-19, 19], |e_pk u| and |e2 s| at most 19 n each: |w'| <= 2^B + 38 n.  So |t (w + w')| / q < v = 2^-b + t (2^B + 38 n) / q, and the budget
after is at least floor(-log2 v) - 1 (one bit for the floor inside bits()).  The tests allow 2 bits under floor(-log2 v), as mod_switch_model.budget_bound's do.

Upper bound (budget_upper) -- a flood that does not flood is a bug too.  Let W = floor((2^(Lq - b - 1) - 1) / t): the input has |w| <= W.  Where
B >= bits(W) + 8 the old noise is below 2^(B - 8).  e1 is uniform on [-2^B, 2^B): a coefficient has |e1| >= 2^(B - 1) with probability at least 1/2, independently, so
SOME coefficient of a ciphertext has, except with probability 2^-n.  For that coefficient
        |w + w'| >= 2^(B - 1) - W - 38 n = m0          (slack: the whole old noise W < 2^(B - 8), and the 38 n of small terms, both against the flood)
and where the lower bound is at least 1 (|t (w + w')| < q / 2, so the centred value is the integer itself) the budget after is AT MOST
        Lq - bits(t m0) - 1.
It applies when B >= bits(W) + 8 and m0 > 0; budget_upper returns None elsewhere.
"""
import ctypes
from fractions import Fraction
from functools import lru_cache

import numpy as np

import mod_switch_model as mm

DOM_FLOOD = 12
COEFF, NTT = 0, 1
PB = ctypes.POINTER(ctypes.c_uint8)


def seed_key(seed):
    """the 256-bit key of the deterministic entry points (chacha_seed_key): the 64-bit seed in front of a fixed tag"""
    return int(seed).to_bytes(8, "little") + b"crcnn-seeded-determinist"


def raw_blocks(E, key, sid, n):
    """block 0 of every stream (sid, even coefficient s) of one ciphertext: n / 2 blocks of 64 bytes"""
    kb = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(key))
    out = (ctypes.c_uint8 * 64)()
    blocks = []
    for s in range(0, n, 2):
        nonce = (ctypes.c_uint8 * 12).from_buffer_copy(int(sid & 0xffffffff).to_bytes(4, "little") + int(sid >> 32).to_bytes(4, "little")
                                                       + (DOM_FLOOD << 24 | s).to_bytes(4, "little"))
        assert E.L.crc_chacha20_block(ctypes.cast(kb, PB), 0, ctypes.cast(nonce, PB), ctypes.cast(out, PB)) == 0
        blocks.append(bytes(out))
    return blocks


def samples(blocks, B, T):
    """(u, e1, e2) of one ciphertext from its blocks: coefficient s + c owns bytes 32 c .. 32 c + 31 of block s / 2"""
    u, e1, e2 = [], [], []
    for b in blocks:
        for c in range(2):
            h = b[32 * c:32 * c + 32]
            tw = int.from_bytes(h[0:8], "little")
            tv = 0
            for j in range(32):
                f = (tw >> (2 * j)) & 3
                if f != 3:
                    tv = f
                    break
            u.append(-1 if tv == 2 else tv)
            mw = int.from_bytes(h[8:16], "little")
            X = int.from_bytes(h[16:32], "little")
            mag = sum(1 for thr in T if mw >= thr)
            e2.append(-mag if X >> 127 else mag)
            e1.append((X & ((1 << (B + 1)) - 1)) - (1 << B))
    return u, e1, e2


@lru_cache(maxsize=None)
def _tables(E):
    return ([E.table(f"root_powers:{i}") for i in range(E.k)], [E.table(f"inv_root_powers_div_two:{i}") for i in range(E.k)])


_cache = {}


def _blocks_cached(E, key, sid, n):
    k = (key, sid, n, "blocks")
    if k not in _cache:
        _cache[k] = raw_blocks(E, key, sid, n)
    return _cache[k]


def _fwd_cached(E, name, row, rp, qi):
    k = (int(qi), E.n) + name
    if k not in _cache:
        _cache[k] = mm.ntt_fwd([v % qi for v in row], rp, qi)
    return _cache[k]


def flood(E, pk, cts, form, B, key, stream_base=0, T=None):
    """the definition on ciphertexts [count][2][k][n] in `form`: a flooded copy"""
    T = T or E.encrypt_dev_noise_thresholds()
    q = [int(v) for v in E.q]; n = E.n
    rp, irp2 = _tables(E)
    cts = np.asarray(cts, dtype=np.uint64).reshape(-1, 2, E.k, n)
    out = np.zeros_like(cts)
    for m in range(cts.shape[0]):
        blocks = _blocks_cached(E, bytes(key), stream_base + m, n)
        u, e1, e2 = samples(blocks, B, T)
        for i, qi in enumerate(q):
            # (u and e2 do not depend on B: their transforms are computed once per stream and modulus)
            un = _fwd_cached(E, (bytes(key), stream_base + m, i, "u"), u, rp[i], qi)
            for p, e in enumerate((e1, e2)):
                prod = [a * int(b) % qi for a, b in zip(un, pk[p, i])]
                if form == NTT:
                    en = _fwd_cached(E, (bytes(key), stream_base + m, i, "e2"), e, rp[i], qi) if p else mm.ntt_fwd([v % qi for v in e], rp[i], qi)
                    add = [(a + b) % qi for a, b in zip(prod, en)]
                else:
                    add = [(a + b) % qi for a, b in zip(mm.ntt_inv(prod, irp2[i], qi), e)]
                out[m, p, i] = np.array([(int(c) + a) % qi for c, a in zip(cts[m, p, i], add)], dtype=np.uint64)
    return out


def admissible(q, t, n, B):
    return 1 <= B <= 126 and 2 * t * ((1 << B) + 38 * n) < mm.product(q)


def noise_cap(q, t, b):
    """W: the largest |w| of a ciphertext with b bits of budget"""
    m = mm.product(q).bit_length() - b - 1
    return ((1 << m) - 1) // t if m > 0 else 0


def flood_bits(q, t, n, b, lam):
    """lam bits above the bit length of W -- for W > 0 the smallest B with 2^B > 2^lam W -- or None where that B is not admissible"""
    W = noise_cap(q, t, b)
    B = lam + W.bit_length()
    if W:
        assert (1 << B) > (W << lam) >= (1 << (B - 1))
    return B if admissible(q, t, n, B) else None


def budget_lower(b, t, n, q, B):
    v = Fraction(1, 1 << b) + Fraction(t * ((1 << B) + 38 * n), mm.product(q))
    bits = 0
    while v * 2 <= 1:
        v *= 2; bits += 1
    return bits


def budget_upper(b, t, n, q, B):
    W = noise_cap(q, t, b)
    m0 = (1 << (B - 1)) - W - 38 * n
    if B < W.bit_length() + 8 or m0 <= 0 or budget_lower(b, t, n, q, B) < 1:
        return None
    return mm.product(q).bit_length() - (t * m0).bit_length() - 1


def budget_upper_after_switch(b, t, n, q, B, kept):
    """an upper bound on the budget of a flooded ciphertext after a modulus switch to the first `kept` moduli -- a switch that loses the flood is a bug too.
    Where budget_upper applies, some coefficient of the flooded ciphertext has N = |t (c0 + c1 s) mod q| >= t m0.  The switch divides c0 + c1 s by P, the product
    of the dropped moduli, and moves it by less than n + 1 per coefficient (mod_switch_model.budget_bound's argument), so that coefficient has
    N' >= N / P - t (n + 1) under q_to as long as the switched ciphertext still decrypts (its lower bound is at least 1, which the caller asserts): the budget is at
    most bits(q_to) - bits(floor(t m0 / P) - t (n + 1)) - 1.  None where budget_upper does not apply or the flood does not survive the division"""
    if budget_upper(b, t, n, q, B) is None:
        return None
    m0 = (1 << (B - 1)) - noise_cap(q, t, b) - 38 * n
    low = t * m0 // mm.product(q[kept:]) - t * (n + 1)
    return mm.product(q[:kept]).bit_length() - low.bit_length() - 1 if low > 0 else None


def chi_square_cells(ws, B, cells_log2=9):
    """bin floor((w + 2^B) / 2^(B + 1 - cells_log2)) and return (statistic against the uniform law, the counts); every w must fall inside [-2^B, 2^B)"""
    cells = 1 << cells_log2
    counts = [0] * cells
    for w in ws:
        c = (w + (1 << B)) >> (B + 1 - cells_log2)
        assert 0 <= c < cells, w
        counts[c] += 1
    exp = len(ws) / cells
    return sum((c - exp) ** 2 for c in counts) / exp, counts
