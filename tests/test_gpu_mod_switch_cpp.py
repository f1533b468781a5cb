"""The host classes' makeLevel / modSwitch / LevelTensor (crcnn_amd/host/modswitch_host.cpp): one encrypted 4 x 4 image at (4096, 2 -> 1) decrypts to the same
floats at the level, travels in SEAL's wire format under the level's own parameters, and the exceptions the header promises."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mod_switch_model as mm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]
T = 1 << 20


def test_host_classes_switch_a_response_to_one_prime():
    import crcnn_amd as ca
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "modswitch_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds modswitch_host"
    n = 4096
    slot_t = ca.Engine.slots_prime(n, 20)
    img = np.random.RandomState(5).uniform(-1, 1, size=16).astype(np.float32)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), T] + Q2 + [slot_t], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    img.tofile(os.path.join(d, "image.f32"))
    out = subprocess.run([driver, d], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "modswitch_host ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    equal = {l[1]: int(l[2]) for l in lines if l[0] == "equal"}
    nbytes = {l[1]: int(l[2]) for l in lines if l[0] == "bytes"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    # decryptImages(LevelTensor) is decryptImages of the unswitched tensor, and both are the image
    full = np.fromfile(os.path.join(d, "full.f32"), dtype=np.float32); low = np.fromfile(os.path.join(d, "level.f32"), dtype=np.float32)
    assert np.array_equal(full, low) and np.allclose(full, img, atol=1e-6)
    assert equal == {"budgets_and_min": 1, "budgets_ntt": 1, "decrypt": 1, "load": 1, "slots": 1}
    # the derived bound, from the budget the driver measured at the full modulus
    for a, b, t in (("full", "level", T), ("slots_full", "slots_level", slot_t)):
        bound = mm.budget_bound(budgets[a], t, n, Q2[0])
        assert budgets[b] >= bound - 2 and bound - 2 > 0, (a, budgets, bound)
    # the file: SEAL's ciphertext format under the level's own parameters, 16 ciphertexts of one prime each -- half the two-prime tensor's
    B = ca.Engine(n, Q2[:1], T, device=-1)
    one = B.L.crc_seal_ct_bytes(B.c, 2)
    assert nbytes["level_ct"] == nbytes["expected"] == 16 * one == os.path.getsize(os.path.join(d, "level.ct"))
    assert nbytes["full_ct"] - nbytes["level_ct"] == 16 * 2 * (n + 1) * 8            # (SEAL stores n + 1 words per polynomial and modulus)
    B.close()
    assert throws == {"level_before_parameters": "logic_error", "level_0": "invalid_argument", "level_k": "invalid_argument", "save_ntt": "invalid_argument",
                      "decrypt_ntt": "invalid_argument", "load_full_file_at_level": "invalid_argument", "load_more_than_the_file": "invalid_argument",
                      "load_less_than_the_file": "invalid_argument", "switch_to_no_level": "invalid_argument", "switch_bad_form": "invalid_argument",
                      "slots_without_batching": "invalid_argument", "stale_level_switch": "invalid_argument", "stale_level_decrypt": "invalid_argument",
                      "stale_level_budget": "invalid_argument", "stale_level_load": "invalid_argument", "stale_level_after_del": "invalid_argument"}
