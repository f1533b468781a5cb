"""The host classes' rotateRows / rotateColumns / sumSlots (crcnn_amd/host/galois_host.cpp): a slot-encrypted batch against the integer expectation, and the
reference's exceptions where the reference throws them."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import galois_model as gm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_rotate_and_sum():
    import crcnn_amd as ca
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "galois_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds galois_host"
    n, P = 4096, 3
    t = ca.Engine.slots_prime(n, 20)
    half = (t - 1) // 2
    v = np.random.RandomState(9).randint(-half, half + 1, size=(n, P)).astype(np.int64)       # [image = slot][pixel = ciphertext]
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    v.tofile(os.path.join(d, "values.i64"))
    out = subprocess.run([driver, d], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "galois_host ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    rows = v.T                                                                                 # [ciphertext][slot]
    tot = (rows.astype(object).sum(axis=1) % t + half) % t - half
    want = {"fresh": rows, "rows_0": rows, "rows_1": gm.rotate_rows_slots(rows, 1), "rows_m1": gm.rotate_rows_slots(rows, -1),
            "rows_5": gm.rotate_rows_slots(rows, 5), "rows_last": gm.rotate_rows_slots(rows, n // 2 - 1), "cols": gm.rotate_columns_slots(rows),
            "rows_5_cols_ntt": gm.rotate_columns_slots(gm.rotate_rows_slots(rows, 5)), "rows_3": gm.rotate_rows_slots(rows, 3),
            "sum": np.repeat(np.array([int(x) for x in tot], dtype=np.int64)[:, None], n, axis=1)}
    assert set(budgets) == set(want)
    for name, w in want.items():
        assert budgets[name] >= 1, (name, budgets[name])
        got = np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64).reshape(n, P)
        assert np.array_equal(got.T, w), name
    assert throws == {"no_batching_rows": "logic_error", "no_batching_columns": "logic_error", "no_batching_sum": "logic_error", "no_keys": "invalid_argument",
                      "steps_too_large": "invalid_argument", "steps_too_large_negative": "invalid_argument", "bad_dbc": "invalid_argument",
                      "bad_element": "invalid_argument", "missing_key_rows": "invalid_argument", "missing_key_columns": "invalid_argument",
                      "missing_key_sum": "invalid_argument"}
