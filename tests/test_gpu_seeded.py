"""Seeded secret-key ciphertexts on the device: crc_seeded_expand_dev (seeded_expand_kernel) against its host twin bit for bit, the round trip through the
device decryptor and budget, the host classes (SeededImages / encryptImageSeeded / expandSeeded), a network on seeded inputs and bench_host's
stream_inputs=seeded.  The host twin is pinned to the oracle's decryptor, to the documented keystream and to the sampling laws by tests/test_seeded_cpu.py."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs
from test_encrypt_sym_cpu import IDS, _derived_budget, _moduli, _plaintexts, param_sets
from test_gpu_host_cpp import DRIVER
from test_seeded_cpu import CARRY_BASE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_expansion(E, cnt, seed, base, rng):
    """both forms against the host twin on random rows below q_i; 0xff in the destination first; the packed source unchanged"""
    import crcnn_amd as ca
    k, n = E.k, E.n
    c0 = np.stack([rng.integers(0, int(E.q[i]), size=(cnt, n), dtype=np.uint64) for i in range(k)], axis=1)
    d_c0 = E.upload(c0); d_ct = E.alloc(cnt * 2 * k * n * 8)
    for form in (ca.NTT, ca.COEFF):
        E.L.crc_memset(E.c, E.p(d_ct), 0xff, cnt * 2 * k * n * 8, E.stream)
        E.seeded_expand_dev(d_c0, cnt, seed, base, form, d_ct)
        got = E.download(d_ct, (cnt, 2, k, n))
        assert np.array_equal(got, E.seeded_expand(c0, seed, base, form)), (cnt, form, base)
        if form == ca.NTT:
            assert np.array_equal(got[:, 0], c0)
    assert np.array_equal(E.download(d_c0, (cnt, k, n)), c0)
    d_c0.free(); d_ct.free()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_device_expansion_equals_the_host_twin(n, q, t):
    import crcnn_amd as ca
    k = len(q)
    E = ca.Engine(n, q, t, device=0)
    rng = np.random.default_rng(5)
    big = max(24, (8 * 256 * 2048) // n)                     # >= 8 workgroups per CU of a 256-CU device
    seed = bytes(range(9, 41))
    for cnt in (1, 24, big):
        _check_expansion(E, cnt, seed, 77 + cnt, rng)
    _check_expansion(E, 8, seed, CARRY_BASE, rng)            # stream ids that carry into the high nonce word
    _check_expansion(E, 5, seed, (1 << 64) - 2, rng)         # ... and wrap around 2^64, as the host's uint64 sum does
    # count 0 writes nothing; overlapping or misaligned ranges and bad forms are refused and write nothing
    cnt = 4
    row = k * n * 8
    d = E.alloc(3 * cnt * row + 64)
    E.L.crc_memset(E.c, E.p(d), 0x5a, 3 * cnt * row + 64, E.stream)
    before = E.download(d, (3 * cnt * row + 64,), dtype=np.uint8)
    key = E._key(seed)
    base = E.p(d)
    assert E.L.crc_seeded_expand_dev(E.c, base, 0, key, 0, ca.NTT, base + cnt * row, E.stream) == 0
    for src, dst in ((base, base), (base + cnt * row, base), (base + 2 * cnt * row - 16, base), (base, base + cnt * row - 16), (base + row, base)):
        assert E.L.crc_seeded_expand_dev(E.c, src, cnt, key, 0, ca.NTT, dst, E.stream) == -1, (src - base, dst - base)
    assert E.L.crc_seeded_expand_dev(E.c, base + 2 * cnt * row + 8, cnt, key, 0, ca.NTT, base, E.stream) == -1          # misaligned source
    for form in (ca.NTTP, ca.NTTL, -1, 7):
        assert E.L.crc_seeded_expand_dev(E.c, base + 2 * cnt * row, cnt, key, 0, form, base, E.stream) == -1
    assert E.L.crc_seeded_expand_dev(E.c, None, cnt, key, 0, ca.NTT, base, E.stream) == -1
    assert E.L.crc_seeded_expand_dev(E.c, base + 2 * cnt * row, cnt, None, 0, ca.NTT, base, E.stream) == -1
    assert E.L.crc_seeded_expand_dev(E.c, base + 2 * cnt * row, cnt, key, 0, ca.NTT, None, E.stream) == -1
    assert np.array_equal(E.download(d, (3 * cnt * row + 64,), dtype=np.uint8), before)
    # adjacent ranges are fine: the source right behind the destination
    assert E.L.crc_seeded_expand_dev(E.c, base + 2 * cnt * row, cnt, key, 0, ca.NTT, base, E.stream) == 0
    E.sync()
    E.close()


@pytest.mark.parametrize("k", [4, 8])
def test_device_expansion_with_two_and_four_blocks_per_pair(k):
    """(16384, 4) and (16384, 8): (k + 1) / 2 = 2 and 4 keystream blocks per coefficient pair"""
    import crcnn_amd as ca
    n = 16384
    q = ca.default_coeff_modulus_128(n)[:k]
    assert len(q) == k
    E = ca.Engine(n, q, 1 << 44, device=0)
    rng = np.random.default_rng(6)
    _check_expansion(E, 3, bytes(range(50, 82)), 12, rng)
    _check_expansion(E, 3, bytes(range(50, 82)), CARRY_BASE, rng)
    E.close()


def test_device_expansion_with_an_odd_number_of_moduli_above_one_block():
    """(16384, 5): the last block serves one modulus only"""
    import crcnn_amd as ca
    n, k = 16384, 5
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, 1 << 44, device=0)
    _check_expansion(E, 3, bytes(range(60, 92)), 3, np.random.default_rng(7))
    E.close()


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_round_trip_through_the_device(n, q, t):
    """encrypt_sym_seeded on the host -> upload -> expand -> crc_decrypt_dev gives the plaintexts; crc_noise_budget_dev at least the derived bound"""
    import crcnn_amd as ca
    k = len(q)
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    rng = np.random.default_rng(5)
    cnt = 24
    pl, max_mc = _plaintexts(E, n, q, t, cnt, rng)
    bound = _derived_budget(q, t, max_mc)
    key, pub = bytes(range(3, 35)), bytes(range(200, 232))
    c0, _, _ = E.encrypt_sym_seeded(sk, pl, 0, key=key, public_seed=pub, stream_base=CARRY_BASE)
    d_sk = E.upload(sk); d_c0 = E.upload(c0); d_ct = E.alloc(cnt * 2 * k * n * 8); d_pl = E.alloc(cnt * n * 8); d_bits = E.alloc(cnt * 4)
    for form in (ca.NTT, ca.COEFF):
        E.seeded_expand_dev(d_c0, cnt, pub, CARRY_BASE, form, d_ct)
        E.decrypt_dev(d_sk, d_ct, cnt, d_pl, E.alloc(E.decrypt_dev_work_bytes(cnt, 2, form)), in_form=form)
        assert np.array_equal(E.download(d_pl, (cnt, n)), pl), form
        E.noise_budget_dev(d_sk, d_ct, cnt, d_bits, E.alloc(E.noise_budget_dev_work_bytes(cnt, 2, form)), in_form=form)
        bits = E.download(d_bits, (cnt,), dtype=np.int32)
        print("device budgets", IDS[param_sets().index((n, q, t))], "form", form, "derived bound", bound, "min", int(bits.min()), "max", int(bits.max()))
        assert int(bits.min()) >= bound, (bits, bound)
    # a wrong seed or base is another c1: nothing decrypts
    E.seeded_expand_dev(d_c0, cnt, pub, CARRY_BASE + 1, ca.NTT, d_ct)
    E.decrypt_dev(d_sk, d_ct, cnt, d_pl, E.alloc(E.decrypt_dev_work_bytes(cnt, 2, ca.NTT)), in_form=ca.NTT)
    assert not np.array_equal(E.download(d_pl, (cnt, n)), pl)
    E.close()


@pytest.mark.parametrize("n,t", [(2048, 1 << 18), (4096, 1 << 29)])
def test_cpp_seeded_images(n, t):
    """encryptImageSeeded -> save -> load -> expandSeeded in both forms: the floats and plaintexts encryptImage's ciphertexts of the same pixels decrypt to"""
    out = subprocess.run([DRIVER, "seeded", str(n), str(t)], capture_output=True, text=True)
    assert out.returncode == 0 and "seeded ok" in out.stdout, out.stderr[-2000:]


def test_cpp_network_on_seeded_inputs():
    """PlainModelTiny at tiny1024's parameters, two images, fused: forward(expandSeeded(encryptImageSeeded(x))) decrypts to the output plaintexts of
    forward(encryptImage(x)) polynomial for polynomial, with at least the public-key run's remaining budget at every output"""
    g = load_net_golden("tiny1024_eng")
    _, _, _, _, img, _ = make_inputs(g)
    d = tempfile.mkdtemp()
    np.array([g["n"], len(g["q"]), g["t"]] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    img = np.asarray(img, dtype=np.float32).reshape(28, 28)
    np.stack([img, img[::-1, ::-1].copy()]).astype(np.float32).tofile(os.path.join(d, "pixels.f32"))
    h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
    out = subprocess.run([DRIVER, "netseeded", g["model"], h5, d], capture_output=True, text=True)
    print(out.stdout.strip())
    assert out.returncode == 0 and "netseeded ok" in out.stdout, (out.stdout[-1500:], out.stderr[-2000:])
    n = g["n"]
    a = np.fromfile(os.path.join(d, "dec_seeded.u64"), dtype=np.uint64).reshape(2, 10, n)
    b = np.fromfile(os.path.join(d, "dec_pk.u64"), dtype=np.uint64).reshape(2, 10, n)
    assert np.array_equal(a, b) and a.any() and not np.array_equal(a[0], a[1])
    shutil.rmtree(d, ignore_errors=True)


def test_bench_host_streams_seeded_inputs():
    """bench.py prepares the small workload's inputs and leaves its bench_host command line; that line with stream_inputs=ciphertext,seeded"""
    keep = tempfile.mkdtemp(prefix="crc_seeded_bench_")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(CRC_BENCH_KEEP=keep, CRC_BENCH_KEEP_CONFIGS="tiny1024")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "tiny1024", "--steps", "1", "--cpu-seconds", "0", "--also", "none", "--full",
                          "--stream-inputs", "both"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    cmd = open(os.path.join(keep, "tiny1024", "cmd_tiny1024.txt")).read().split()
    assert any(c.startswith("plain_inputs=") for c in cmd) and any(c.startswith("stream_inputs=") for c in cmd)
    cmd = [c for c in cmd if not c.startswith(("stream_inputs=", "stream_steps="))] + ["stream_inputs=ciphertext,seeded", "stream_steps=1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    line = json.loads(p.stdout.strip().splitlines()[-1])
    modes = {s["mode"]: s for s in line["streamed"]}
    assert set(modes) == {"ciphertext", "seeded"}
    print({m: (s["images_per_s"], s["bytes_per_image"]) for m, s in modes.items()})
    assert modes["ciphertext"]["outputs_identical_to_resident"] is True and "outputs_decrypt_identical_to_resident" not in modes["ciphertext"]
    assert modes["seeded"]["outputs_decrypt_identical_to_resident"] is True and modes["seeded"]["outputs_identical_to_resident"] is None
    assert 2 * modes["seeded"]["bytes_per_image"] == modes["ciphertext"]["bytes_per_image"]
    assert line["last_timed_launch_identical_to_first"] is True
    # an unknown mode is refused before any work
    bad = subprocess.run([c for c in cmd if not c.startswith("stream_inputs=")] + ["stream_inputs=ciphertext,seed"], capture_output=True, text=True, timeout=900)
    assert bad.returncode != 0 and "stream_inputs=" in bad.stderr
    shutil.rmtree(keep, ignore_errors=True)
