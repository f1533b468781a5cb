"""The seeded form produced on the device: crc_encrypt_sym_seeded_dev[_key] (seeded_enc_sample_kernel -> the row transform -> seeded_enc_mask_kernel) and
crc_encrypt_f32_seeded_dev[_key] (the compact device encoder in front) against the host twin crc_encrypt_sym_seeded[_key] bit for bit, the round trip through
the device expansion, decryptor and budget, the refusals, and the host classes (encryptImageSeeded(..., on_device = true): seeded_host roundtrip).  The host
twin is pinned to the oracle's decryptor, to the documented keystreams and to the sampling laws by tests/test_seeded_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

from test_encrypt_sym_cpu import IDS, _derived_budget, _plaintexts, param_sets
from test_seeded_cpu import CARRY_BASE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED_HOST = os.path.join(ROOT, "crcnn_amd", "lib", "seeded_host")
KEY, PUB = bytes(range(3, 35)), bytes(range(200, 232))


def _check_encryption(E, sk, d_sk, pl, key=None, pub=None, base=0, seed=0):
    """one call against the host twin; 0xff in the destination first; the plaintexts and the device secret key unchanged"""
    cnt, k, n = pl.shape[0], E.k, E.n
    d_pl = E.upload(pl); d_c0 = E.alloc(cnt * k * n * 8)
    E.L.crc_memset(E.c, E.p(d_c0), 0xff, cnt * k * n * 8, E.stream)
    got_seed, got_base = E.encrypt_sym_seeded_dev(d_sk, d_pl, cnt, seed, d_c0, key=key, public_seed=pub, stream_base=base)
    got = E.download(d_c0, (cnt, k, n))
    want, want_seed, want_base = E.encrypt_sym_seeded(sk, pl, seed, key=key, public_seed=pub, stream_base=base)
    assert (got_seed, got_base) == (want_seed, want_base)
    assert np.array_equal(got, want), (cnt, base, seed, int(np.argmax((got != want).reshape(-1))))
    assert np.array_equal(E.download(d_pl, (cnt, n)), pl)
    assert np.array_equal(E.download(d_sk, sk.shape), sk)
    d_pl.free(); d_c0.free()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_device_encryption_equals_the_host_twin(n, q, t):
    """all six parameter sets: the 40- and 60-bit-modulus rings lack the wave-local transform, so both transform paths run"""
    import crcnn_amd as ca
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    d_sk = E.upload(sk)
    rng = np.random.default_rng(5)
    big = max(24, (8 * 256 * 2048) // n)                     # >= 8 workgroups per CU of a 256-CU device
    for cnt in (1, 24, big):
        pl, _ = _plaintexts(E, n, q, t, max(cnt, 2), rng)
        pl = np.ascontiguousarray(pl[:cnt])
        for base in (77 + cnt, CARRY_BASE, (1 << 64) - 2):   # ... stream ids that carry into the high nonce word, and that wrap around 2^64
            _check_encryption(E, sk, d_sk, pl, key=KEY, pub=PUB, base=base)
        _check_encryption(E, sk, d_sk, pl, seed=1234 + cnt)
    E.close()


@pytest.mark.parametrize("k", [4, 5, 8])
def test_device_encryption_with_two_three_and_four_mask_blocks_per_pair(k):
    """(16384, 4), (16384, 5), (16384, 8): (k + 1) / 2 = 2, 3 and 4 blocks of the public stream per coefficient pair, the last one of k = 5 serving one modulus"""
    import crcnn_amd as ca
    n, t = 16384, 1 << 44
    q = ca.default_coeff_modulus_128(n)[:k]
    assert len(q) == k
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    d_sk = E.upload(sk)
    pl, _ = _plaintexts(E, n, q, t, 3, np.random.default_rng(6))
    _check_encryption(E, sk, d_sk, pl, key=KEY, pub=PUB, base=12)
    _check_encryption(E, sk, d_sk, pl, key=KEY, pub=PUB, base=CARRY_BASE)
    _check_encryption(E, sk, d_sk, pl, seed=99)
    E.close()


def _f32_values(rng):
    """2000 floats in the MNIST-normalised range ((x - 0.1307) / 0.3081 for x in [0, 1]: -0.4242 .. 2.8215) and the edge values: the issue's list, the float32
    edge inputs of test_gpu_ops.test_device_fractional_codec, and the largest float whose integer part the 64 low coefficients hold.  64 balanced ternary digits
    (each 0 or +-1, whatever t >= 3 is) reach (3^64 - 1) / 2 > 2^63, so the encoder's int64 integer part is what limits it: the largest float32 below 2^63"""
    rnd = ((rng.random(2000) - 0.1307) / 0.3081).astype(np.float32)
    issue = [0.0, 1.0, -1.0, 0.5, -0.5, 1 / 3, -1 / 3, 2.8215, -2.8215, 1e-9, -1e-9, 12345.678, -12345.678]
    codec = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 1 / 3, -1 / 3, 1e-9, -1e-9, 12345.678, -98765.4321, 3.0 ** -32, 0.49999997, 1e6 + 0.5, -1e6 - 0.25]
    top = np.nextafter(np.float32(2.0 ** 63), np.float32(0))
    assert float(top) == 2.0 ** 63 - 2.0 ** 39
    return np.concatenate([rnd, np.array(issue + codec, dtype=np.float32), np.array([top, -top], dtype=np.float32)])


@pytest.mark.parametrize("n,k,t", [(2048, 1, 1 << 18), (4096, 2, 1 << 29), (8192, 3, 1 << 42)])
def test_f32_path_equals_host_encode_then_host_encrypt(n, k, t):
    import crcnn_amd as ca
    from test_encrypt_sym_cpu import _moduli
    q = _moduli(n, k)
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    vals = _f32_values(np.random.default_rng(17))
    cnt = vals.size
    pl, _ = E.encode(vals)
    d_sk = E.upload(sk); d_v = E.upload(vals); d_c0 = E.alloc(cnt * k * n * 8); d_w = E.alloc(E.encrypt_f32_seeded_dev_work_bytes(cnt))
    for kw in (dict(), dict(key=KEY, public_seed=PUB, stream_base=CARRY_BASE)):
        E.L.crc_memset(E.c, E.p(d_c0), 0xff, cnt * k * n * 8, E.stream)
        E.encrypt_f32_seeded_dev(d_sk, d_v, cnt, 4321, d_c0, d_w, **kw)
        want, _, _ = E.encrypt_sym_seeded(sk, pl, 4321, **kw)
        assert np.array_equal(E.download(d_c0, (cnt, k, n)), want), kw
    assert np.array_equal(E.download(d_v, (cnt,), dtype=np.float32).view(np.uint32), vals.view(np.uint32))
    # the compact plaintexts left in the work buffer are the words crc_encode_f32_compact gives (the buffer is aligned up to 256 bytes inside)
    import ctypes
    cp = np.zeros((cnt, 96), dtype=np.uint64)
    assert E.L.crc_encode_f32_compact(E.c, vals.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cnt, cp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None) == 0
    off = (-E.p(d_w)) % 256
    assert np.array_equal(E.download(d_w, (off + cnt * 96 * 8,), dtype=np.uint8)[off:].view(np.uint64).reshape(cnt, 96), cp)
    E.close()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_round_trip_on_the_device(n, q, t):
    """crc_encrypt_sym_seeded_dev_key -> crc_seeded_expand_dev in both forms -> crc_decrypt_dev gives the plaintexts; crc_noise_budget_dev at least the derived
    integer bound of test_encrypt_sym_cpu for every ciphertext; another stream base in the expansion is another c1 and nothing decrypts"""
    import crcnn_amd as ca
    k = len(q)
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    rng = np.random.default_rng(5)
    cnt = 24
    pl, max_mc = _plaintexts(E, n, q, t, cnt, rng)
    bound = _derived_budget(q, t, max_mc)
    d_sk = E.upload(sk); d_pl_in = E.upload(pl); d_c0 = E.alloc(cnt * k * n * 8)
    d_ct = E.alloc(cnt * 2 * k * n * 8); d_pl = E.alloc(cnt * n * 8); d_bits = E.alloc(cnt * 4)
    E.encrypt_sym_seeded_dev(d_sk, d_pl_in, cnt, 0, d_c0, key=KEY, public_seed=PUB, stream_base=CARRY_BASE)
    for form in (ca.NTT, ca.COEFF):
        E.seeded_expand_dev(d_c0, cnt, PUB, CARRY_BASE, form, d_ct)
        d_dw = E.alloc(E.decrypt_dev_work_bytes(cnt, 2, form)); d_bw = E.alloc(E.noise_budget_dev_work_bytes(cnt, 2, form))
        E.decrypt_dev(d_sk, d_ct, cnt, d_pl, d_dw, in_form=form)
        assert np.array_equal(E.download(d_pl, (cnt, n)), pl), form
        E.noise_budget_dev(d_sk, d_ct, cnt, d_bits, d_bw, in_form=form)
        bits = E.download(d_bits, (cnt,), dtype=np.int32)
        d_dw.free(); d_bw.free()
        print("device budgets", IDS[param_sets().index((n, q, t))], "form", form, "derived bound", bound, "min", int(bits.min()), "max", int(bits.max()))
        assert int(bits.min()) >= bound, (bits, bound)
    E.seeded_expand_dev(d_c0, cnt, PUB, CARRY_BASE + 1, ca.NTT, d_ct)
    d_dw = E.alloc(E.decrypt_dev_work_bytes(cnt, 2, ca.NTT))
    E.decrypt_dev(d_sk, d_ct, cnt, d_pl, d_dw, in_form=ca.NTT)
    assert not np.array_equal(E.download(d_pl, (cnt, n)), pl)
    d_dw.free()
    E.close()


def test_refusals_write_nothing():
    import crcnn_amd as ca
    from test_encrypt_sym_cpu import _moduli
    n, k, t = 4096, 2, 1 << 29
    E = ca.Engine(n, _moduli(n, k), t, device=0)
    L = E.L
    sk, _ = E.keygen(11)
    d_sk = E.upload(sk)
    cnt = 4
    row, prow = k * n * 8, n * 8
    wb = E.encrypt_f32_seeded_dev_work_bytes(cnt)
    # one buffer: [c0 rows of cnt][plaintexts of cnt][floats + slack][work]
    total = cnt * row + cnt * prow + 256 + wb
    d = E.alloc(total)
    L.crc_memset(E.c, E.p(d), 0x5a, total, E.stream)
    before = E.download(d, (total,), dtype=np.uint8)
    c0 = E.p(d); plp = c0 + cnt * row; vp = plp + cnt * prow; wp = vp + 256
    skp = E.p(d_sk)
    key, pub = E._key(KEY), E._key(PUB)
    # count == 0: CRC_OK, nothing written
    assert L.crc_encrypt_sym_seeded_dev_key(E.c, skp, plp, 0, key, pub, 0, c0, E.stream) == 0
    assert L.crc_encrypt_sym_seeded_dev(E.c, skp, plp, 0, 7, c0, E.stream) == 0
    assert L.crc_encrypt_f32_seeded_dev_key(E.c, skp, vp, 0, key, pub, 0, c0, wp, E.stream) == 0
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, vp, 0, 7, c0, wp, E.stream) == 0
    # key == seed
    assert L.crc_encrypt_sym_seeded_dev_key(E.c, skp, plp, cnt, key, E._key(KEY), 0, c0, E.stream) == -1
    assert L.crc_encrypt_f32_seeded_dev_key(E.c, skp, vp, cnt, key, E._key(KEY), 0, c0, wp, E.stream) == -1
    # each NULL argument
    good = [E.c, skp, plp, cnt, key, pub, 0, c0, E.stream]
    for hole in (0, 1, 2, 4, 5, 7):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_sym_seeded_dev_key(*a) == -1, hole
    good = [E.c, skp, plp, cnt, 7, c0, E.stream]
    for hole in (0, 1, 2, 5):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_sym_seeded_dev(*a) == -1, hole
    good = [E.c, skp, vp, cnt, key, pub, 0, c0, wp, E.stream]
    for hole in (0, 1, 2, 4, 5, 7, 8):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_f32_seeded_dev_key(*a) == -1, hole
    good = [E.c, skp, vp, cnt, 7, c0, wp, E.stream]
    for hole in (0, 1, 2, 5, 6):
        a = list(good); a[hole] = None
        assert L.crc_encrypt_f32_seeded_dev(*a) == -1, hole
    # the plaintexts overlapping the rows: equal, partly from either side, by one 16-byte pair
    for src, dst in ((c0, c0), (c0 + row, c0), (c0 + cnt * row - 16, c0), (c0, c0 + cnt * prow - 16)):
        assert L.crc_encrypt_sym_seeded_dev_key(E.c, skp, src, cnt, key, pub, 0, dst, E.stream) == -1, (src - c0, dst - c0)
        assert L.crc_encrypt_sym_seeded_dev(E.c, skp, src, cnt, 7, dst, E.stream) == -1, (src - c0, dst - c0)
    # the floats, the work buffer or the secret key inside the rows
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, c0 + 64, cnt, 7, c0, wp, E.stream) == -1
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, vp, cnt, 7, c0, c0 + 256, E.stream) == -1
    assert L.crc_encrypt_sym_seeded_dev(E.c, c0, plp, 1, 7, c0, E.stream) == -1
    # the work buffer over the floats
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, wp, cnt, 7, c0, wp, E.stream) == -1
    # misaligned pointers: rows, plaintexts, key (16 bytes), floats (4 bytes)
    assert L.crc_encrypt_sym_seeded_dev(E.c, skp, plp, cnt - 1, 7, c0 + 8, E.stream) == -1
    assert L.crc_encrypt_sym_seeded_dev(E.c, skp, plp + 8, cnt - 1, 7, c0, E.stream) == -1
    assert L.crc_encrypt_sym_seeded_dev(E.c, skp + 8, plp, cnt, 7, c0, E.stream) == -1
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, vp, cnt, 7, c0 + 8, wp, E.stream) == -1
    assert L.crc_encrypt_f32_seeded_dev(E.c, skp, vp + 2, cnt, 7, c0, wp, E.stream) == -1
    E.sync()
    assert np.array_equal(E.download(d, (total,), dtype=np.uint8), before)
    assert np.array_equal(E.download(d_sk, sk.shape), sk)
    # adjacent ranges are fine: the plaintexts right behind the rows
    assert L.crc_encrypt_sym_seeded_dev(E.c, skp, plp, cnt, 7, c0, E.stream) == 0
    E.sync()
    after = E.download(d, (total,), dtype=np.uint8)
    assert np.array_equal(after[cnt * row:], before[cnt * row:]) and not np.array_equal(after[:cnt * row], before[:cnt * row])
    E.close()


def test_f32_path_refuses_a_short_ring():
    """n = 64 <= CRC_PLAIN_COMPACT_WORDS: the compact form does not exist there (as k_encrypt_sym refuses compact input)"""
    import crcnn_amd as ca
    n = 64
    q = ca.default_coeff_modulus_128(2048)       # one prime = 1 mod 4096, hence = 1 mod 128
    E = ca.Engine(n, q, 1 << 10, device=0)
    sk, _ = E.keygen(11)
    d_sk = E.upload(sk)
    cnt = 2
    d_v = E.upload(np.zeros(cnt, dtype=np.float32)); d_c0 = E.alloc(cnt * E.k * n * 8); d_w = E.alloc(E.encrypt_f32_seeded_dev_work_bytes(cnt))
    E.L.crc_memset(E.c, E.p(d_c0), 0x5a, cnt * E.k * n * 8, E.stream)
    assert E.L.crc_encrypt_f32_seeded_dev(E.c, E.p(d_sk), E.p(d_v), cnt, 7, E.p(d_c0), E.p(d_w), E.stream) == -1
    assert E.L.crc_encrypt_f32_seeded_dev_key(E.c, E.p(d_sk), E.p(d_v), cnt, E._key(KEY), E._key(PUB), 0, E.p(d_c0), E.p(d_w), E.stream) == -1
    assert (E.download(d_c0, (cnt * E.k * n,)) == 0x5a5a5a5a5a5a5a5a).all()
    E.close()


@pytest.mark.parametrize("n,t", [(2048, 1 << 18), (4096, 1 << 29)])
def test_cpp_seeded_images_on_the_device(n, t):
    """encryptImageSeeded(..., on_device = true) == the host path byte for byte under a deterministic seed; save -> load -> expandSeeded in both forms ->
    decryptImages gives the floats of encryptImage's ciphertexts; with OS entropy fresh seeds and the same floats"""
    out = subprocess.run([SEEDED_HOST, "roundtrip", str(n), str(t)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "seeded_host ok" in out.stdout, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
