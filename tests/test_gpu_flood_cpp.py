"""The host classes' floodImages / floodBits / sanitizeResponse / Network::flood_bits (crcnn_amd/host/flood_host.cpp): one encrypted 4 x 4 image at
(4096, 3 -> 2) flooded at the full modulus and at the level, sanitizeResponse against flood-then-switch under the deterministic seed, and PlainModelTiny at
(4096, 2, t = 2^20) with and without Network::flood_bits.  Every budget is held against the bounds tests/flood_model.py derives."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import flood_model as fm
import mod_switch_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3 = [0x7fffffff380001, 0x7ffffffef00001, 0x3fffffff000001]
Q2 = [0x7fffffff380001, 0x3fffffff000001]
T = 1 << 20
N = 4096
# The budget of PlainModelTiny's logits that the driver floods by.  It is NOT derived from the network (nothing in the project derives a network's budget from
# its weights yet: DESIGN section 10): it is the smallest figure for which a 40-bit flood is admitted at (4096, 2, t = 2^20)
# (40 + bits(q) - b - bits(t) <= bits(q) - bits(t) - 2), and the test asserts that the measured budget is no smaller, i.e. that the figure is at least a valid
# lower bound.  At these parameters the flood takes all but 2 bits, so the derived LOWER bound on the flooded logits is lo - 2 = 0 and asserts nothing here;
# what binds is the derived upper bound, the equality of the logits, and the lower bounds of the image tests above, which have room (lo - 2 > 0 is asserted there).
NET_BUDGET = 42


def fresh_budget(q, t, n):
    """a fresh public-key encryption, derived: |t (c0 + c1 s) mod q| <= 19 t (2 n + 1) + t^2 (the noise e1 - e_pk u + e2 s, and (q mod t) m from Delta m)"""
    return mm.product(q).bit_length() - (19 * t * (2 * n + 1) + t * t).bit_length() - 1


def run_driver(with_model):
    driver = os.path.join(ROOT, "crcnn_amd", "lib", "flood_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds flood_host"
    b_full = fresh_budget(Q3, T, N)
    b_level = mm.budget_bound(b_full, T, N, mm.product(Q3[:2])) - 1
    d = tempfile.mkdtemp()
    np.array([N, len(Q3), T] + Q3 + [b_full, b_level, NET_BUDGET], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    np.random.RandomState(5).uniform(-1, 1, size=16).astype(np.float32).tofile(os.path.join(d, "image.f32"))
    args = [driver, d] + ([os.path.join(ROOT, "tests", "golden", "models", "PlainModelTiny.h5")] if with_model else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "flood_host ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    get = lambda kind, conv: {l[1]: conv(l[2]) for l in lines if l[0] == kind}
    return get("bits", int), get("budget", int), get("equal", int), get("throws", str), get("digest", int), b_full, b_level


@pytest.fixture(scope="module")
def driver_output():
    return run_driver(True)


def test_flood_images_and_sanitize_response(driver_output):
    bits, budgets, equal, throws, _, b_full, b_level = driver_output
    assert bits["full"] == fm.flood_bits(Q3, T, N, b_full, 40) and bits["level"] == fm.flood_bits(Q3[:2], T, N, b_level, 40)
    assert budgets["full"] >= b_full and budgets["level"] >= b_level                      # the a-priori figures are lower bounds
    for name, q, b, B in (("full", Q3, budgets["full"], bits["full"]), ("level", Q3[:2], budgets["level"], bits["level"])):
        lo, hi = fm.budget_lower(b, T, N, q, B), fm.budget_upper(b, T, N, q, B)
        got = budgets[name + "_flooded"]
        print(f"{name}: budget {b} -> {got} after a flood of {B} bits, derived [{lo} - 2, {hi}]")
        assert hi is not None and lo - 2 <= got <= hi and lo - 2 > 0
        if name == "level":                                                                # the NTT-resident LevelTensor, flooded as it stands: the same bounds
            assert lo - 2 <= budgets["level_flooded_ntt"] <= hi
    # decrypt_level: decryptImages of the flooded coefficient-form LevelTensor (the level's public-key rows and context) gives the floats of before
    for name in ("decrypt_full", "flood_changed_full", "decrypt_level", "decrypt_switched", "flood_changed_level", "flood_changed_level_ntt", "refusals_wrote_nothing",
                 "sanitize_is_flood_then_switch", "sanitize_leaves_its_input"):
        assert equal[name] == 1, name
    for name in ("flood_bits_impossible", "flood_width_0", "flood_width_127", "flood_level_width", "sanitize_no_level"):
        assert throws[name] == "invalid_argument", (name, throws)


def test_a_network_with_flood_bits(driver_output):
    bits, budgets, equal, throws, digests, _, _ = driver_output
    assert budgets["net"] >= NET_BUDGET, "NET_BUDGET is not a lower bound of the logits' budget"
    B = bits["net"]
    assert B == fm.flood_bits(Q2, T, N, NET_BUDGET, 40)
    lo, hi = fm.budget_lower(budgets["net"], T, N, Q2, B), fm.budget_upper(budgets["net"], T, N, Q2, B)
    print(f"PlainModelTiny: budget {budgets['net']} -> {budgets['net_flooded']} after a flood of {B} bits, derived [{lo} - 2, {hi}]")
    assert hi is not None and lo - 2 <= budgets["net_flooded"] <= hi and lo >= 1        # (lo >= 1: the logits still decrypt, which the driver checked)
    assert equal["logits"] == 1 and equal["flood_changed_net"] == 1
    # flood_bits = 0: the output of before, bit for bit, from the same launches
    assert digests["plain"] == digests["plain_again"] and equal["launches"] == 1
    assert throws["net_bad_width"] == "invalid_argument"
