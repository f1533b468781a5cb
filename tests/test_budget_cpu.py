"""The device noise-budget path without a GPU: the exported symbols, the argument checks of crc_noise_budget_dev on a host-only context, and the per-coefficient
routine the kernel runs (csrc/budget_bits.h, through crc_budget_bits_host) at every word boundary of its multi-word accumulator and on both sides of the centring
against floor(q/2) -- expected values from Python integers."""
import ctypes

import numpy as np
import pytest

import crcnn_amd as ca
from crcnn_amd import binding

T30 = 1 << 30


def test_symbols_declared_and_exported():
    syms = binding.header_symbols()
    L = binding.load()
    for s in ("crc_noise_budget_dev", "crc_noise_budget_dev_work_bytes", "crc_budget_bits_host"):
        assert s in syms and hasattr(L, s), s


def test_argument_checks_on_host_only_context():
    E = ca.Engine(4096, ca.default_coeff_modulus_128(4096), 1 << 20, device=-1)
    try:
        for form in (ca.COEFF, ca.NTT):
            for size in (2, 3):
                w = [E.noise_budget_dev_work_bytes(c, size, form) for c in (1, 2, 67, 1024)]
                d = [E.decrypt_dev_work_bytes(c, size, form) for c in (1, 2, 67, 1024)]
                assert all(a >= b > 0 for a, b in zip(w, d)), (w, d)
                assert all(w[i] < w[i + 1] for i in range(3)), w
        buf = (ctypes.c_uint64 * 16)()
        ptr = ctypes.addressof(buf)
        call = lambda sk, ct, count, size, form, bits, work: E.L.crc_noise_budget_dev(E.c, sk, ct, count, size, form, bits, None, work, None)
        bad = -1                                                                # CRC_ERR_INVALID_ARGUMENT
        assert call(ptr, ptr, 1, 4, ca.COEFF, ptr, ptr) == bad                 # size 4
        assert call(ptr, ptr, 1, 1, ca.COEFF, ptr, ptr) == bad
        assert call(ptr, ptr, 1, 2, ca.NTTL, ptr, ptr) == bad                  # a limb form
        assert call(ptr, ptr, 1, 2, ca.NTTP, ptr, ptr) == bad
        for hole in range(4):                                                   # a null pointer: key, ciphertexts, result, work
            a = [ptr] * 4; a[hole] = None
            assert call(a[0], a[1], 1, 2, ca.COEFF, a[2], a[3]) == bad, hole
        assert E.L.crc_budget_bits_host(E.c, None, 1, ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int32))) == bad
        assert E.L.crc_budget_bits_host(E.c, ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint64)), 1, None) == bad
    finally:
        E.close()


def _product(q):
    Q = 1
    for p in q:
        Q *= p
    return Q


def _expected(total_bits, Q, target):
    return max(0, total_bits - min(target, Q - target).bit_length() - 1)


@pytest.mark.parametrize("ring, primes", [(8192, 3), (16384, 8)])
def test_boundary_values_of_the_shared_routine(ring, primes):
    """t v mod q = 2^j - 1, 2^j, q - 2^j, q - (2^j - 1) for EVERY j below the bit count of q: every word boundary of the accumulator, both sides of the centring"""
    q = [int(p) for p in ca.default_coeff_modulus_128(ring)[:primes]]
    assert len(q) == primes
    n, Q = 256, _product(q)
    total_bits = Q.bit_length()
    if primes == 3:
        assert total_bits == 164
    tinv = pow(T30, -1, Q)
    E = ca.Engine(n, q, T30, device=-1)
    try:
        cases = []
        for j in range(total_bits):
            for target in ((1 << j) - 1, 1 << j, Q - (1 << j), Q - ((1 << j) - 1)):
                cases.append((j, target % Q))
        V = np.zeros((len(cases), primes, n), dtype=np.uint64)
        for m, (j, target) in enumerate(cases):
            x = target * tinv % Q
            V[m, :, (7 * j) % n] = [x % p for p in q]
        got = E.budget_bits_host(V)
        want = [_expected(total_bits, Q, target) for _, target in cases]
        wrong = [(cases[m][0], m % 4, int(got[m]), want[m]) for m in range(len(cases)) if int(got[m]) != want[m]]
        assert not wrong, wrong[:10]
        assert len(cases) == 4 * total_bits
    finally:
        E.close()


@pytest.mark.parametrize("ring, primes", [(4096, 2), (8192, 3), (16384, 4), (16384, 8)])
def test_zero_and_random_rows(ring, primes):
    q = [int(p) for p in ca.default_coeff_modulus_128(ring)[:primes]]
    n, Q = 256, _product(q)
    total_bits = Q.bit_length()
    E = ca.Engine(n, q, T30, device=-1)
    try:
        assert E.budget_bits_host(np.zeros((primes, n), dtype=np.uint64)) == total_bits - 1
        rng = np.random.RandomState(1234 + primes)
        V = np.stack([np.stack([rng.randint(0, p, size=n, dtype=np.uint64) for p in q]) for _ in range(3)])
        got = E.budget_bits_host(V)
        for m in range(3):
            norm = 0
            for s in range(n):
                x = 0
                for i, p in enumerate(q):                                       # CRT
                    qh = Q // p
                    x += int(V[m, i, s]) * pow(qh, -1, p) % p * qh
                x = x * T30 % Q
                norm = max(norm, min(x, Q - x))
            want = max(0, total_bits - norm.bit_length() - 1)
            assert want in (0, 1) and int(got[m]) == want, (m, int(got[m]), want)
    finally:
        E.close()
