"""The device encryptor of the seeded form (crc_encrypt_sym_seeded_dev[_key], crc_encrypt_f32_seeded_dev[_key]) as far as it can be checked without a GPU: the
symbols resolve, a host-only context gets the status every device entry point returns there and nothing is written, and the refusals that need no device hold.
tests/test_gpu_seeded_encrypt.py pins the kernels to the host twin crc_encrypt_sym_seeded_key, which tests/test_seeded_cpu.py pins to the oracle."""
import ctypes

import numpy as np

import crcnn_amd as ca
from test_encrypt_sym_cpu import _moduli

NEW = ["crc_encrypt_sym_seeded_dev_key", "crc_encrypt_sym_seeded_dev", "crc_encrypt_f32_seeded_dev_work_bytes", "crc_encrypt_f32_seeded_dev_key",
       "crc_encrypt_f32_seeded_dev"]


def test_symbols_resolve_and_the_engine_has_the_wrappers():
    L = ca.binding.load()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in ca.binding.header_symbols(), name
    for m in ("encrypt_sym_seeded_dev", "encrypt_f32_seeded_dev", "encrypt_f32_seeded_dev_work_bytes"):
        assert callable(getattr(ca.Engine, m)), m


def test_work_bytes():
    n = 1024
    E = ca.Engine(n, _moduli(n, 2), 1 << 16, device=-1)
    assert E.L.crc_encrypt_f32_seeded_dev_work_bytes(None, 5) == 0
    for cnt in (0, 1, 784, 100000):
        assert E.encrypt_f32_seeded_dev_work_bytes(cnt) >= cnt * 96 * 8
    E.close()


def test_host_only_context_is_refused_and_nothing_is_written():
    """host memory stands in for the device buffers: a call that is refused must not touch any of them"""
    n = 1024
    q = _moduli(n, 2)
    E = ca.Engine(n, q, 1 << 16, device=-1)
    k, cnt = len(q), 3
    sk, _ = E.keygen(11)
    pl = np.arange(cnt * n, dtype=np.uint64).reshape(cnt, n) % 7
    vals = np.linspace(-1, 1, cnt).astype(np.float32)
    c0 = np.full((cnt, k, n), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    work = np.full(E.encrypt_f32_seeded_dev_work_bytes(cnt), 0x5a, dtype=np.uint8)
    keep = [a.copy() for a in (sk, pl, vals, c0, work)]
    key, pub = E._key(bytes(range(32))), E._key(bytes(range(100, 132)))
    P = lambda a: a.ctypes.data
    L = E.L
    for count in (cnt, 0):
        assert L.crc_encrypt_sym_seeded_dev_key(E.c, P(sk), P(pl), count, key, pub, 5, P(c0), None) < 0
        assert L.crc_encrypt_sym_seeded_dev(E.c, P(sk), P(pl), count, 77, P(c0), None) < 0
        assert L.crc_encrypt_f32_seeded_dev_key(E.c, P(sk), P(vals), count, key, pub, 5, P(c0), P(work), None) < 0
        assert L.crc_encrypt_f32_seeded_dev(E.c, P(sk), P(vals), count, 77, P(c0), P(work), None) < 0
    with np.testing.assert_raises(ca.CrcError):
        E.encrypt_sym_seeded_dev(P(sk), P(pl), cnt, 77, P(c0))
    with np.testing.assert_raises(ca.CrcError):
        E.encrypt_f32_seeded_dev(P(sk), P(vals), cnt, 77, P(c0), P(work), key=bytes(range(32)), public_seed=bytes(range(100, 132)), stream_base=9)
    for a, b in zip((sk, pl, vals, c0, work), keep):
        assert np.array_equal(a, b)
    E.close()


def test_refusals_that_need_no_device():
    """NULL arguments and a public seed byte-equal to the private key: CRC_ERR_INVALID_ARGUMENT before anything else is looked at"""
    n = 1024
    q = _moduli(n, 2)
    E = ca.Engine(n, q, 1 << 16, device=-1)
    k, cnt = len(q), 2
    sk, _ = E.keygen(11)
    pl = np.zeros((cnt, n), dtype=np.uint64); vals = np.zeros(cnt, dtype=np.float32)
    c0 = np.full((cnt, k, n), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    work = np.full(E.encrypt_f32_seeded_dev_work_bytes(cnt), 0x5a, dtype=np.uint8)
    key, pub = E._key(bytes(range(32))), E._key(bytes(range(100, 132)))
    P = lambda a: a.ctypes.data
    L = E.L
    good = [E.c, P(sk), P(pl), cnt, key, pub, 5, P(c0), None]
    for hole in (0, 1, 2, 4, 5, 7):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_sym_seeded_dev_key(*a) == -1, hole
    good = [E.c, P(sk), P(pl), cnt, 77, P(c0), None]
    for hole in (0, 1, 2, 5):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_sym_seeded_dev(*a) == -1, hole
    good = [E.c, P(sk), P(vals), cnt, key, pub, 5, P(c0), P(work), None]
    for hole in (0, 1, 2, 4, 5, 7, 8):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_f32_seeded_dev_key(*a) == -1, hole
    good = [E.c, P(sk), P(vals), cnt, 77, P(c0), P(work), None]
    for hole in (0, 1, 2, 5, 6):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_f32_seeded_dev(*a) == -1, hole
    same = E._key(bytes(range(32)))
    assert L.crc_encrypt_sym_seeded_dev_key(E.c, P(sk), P(pl), cnt, key, same, 5, P(c0), None) == -1
    assert L.crc_encrypt_f32_seeded_dev_key(E.c, P(sk), P(vals), cnt, key, same, 5, P(c0), P(work), None) == -1
    assert (c0 == 0x5a5a5a5a5a5a5a5a).all() and (work == 0x5a).all()
    E.close()
