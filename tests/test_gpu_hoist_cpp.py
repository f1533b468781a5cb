"""The host classes' rotateRowsMany / matvecSlots (crcnn_amd/host/hoist_host.cpp): hoisted rotations and the diagonal matrix-vector product of slot-encrypted
vectors against the integer expectation, with the reference's exceptions where rotateRows throws them."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import galois_hoisted_model as hm
import galois_model as gm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_rotate_many_and_matvec():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "hoist_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds hoist_host"
    n, P, M, t = 4096, 3, 8, 65537
    half = (t - 1) // 2
    rng = np.random.RandomState(19)
    xs = rng.randint(-half, half + 1, size=(P, M)).astype(np.int64)                           # one vector of M entries per ciphertext
    rows = np.tile(xs, (1, n // M))                                                            # [ciphertext][slot], period M
    W8 = rng.randint(0, t, size=(8, 8)).astype(np.int64); W8[0, 0] = t - 1
    W5 = rng.randint(-half, half + 1, size=(5, 8)).astype(np.int64)                            # (any int64 is taken mod t)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    np.ascontiguousarray(rows.T).tofile(os.path.join(d, "values.i64"))                         # [slot][ciphertext]
    W8.tofile(os.path.join(d, "w8.i64")); W5.tofile(os.path.join(d, "w5.i64"))
    out = subprocess.run([driver, d], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "hoist_host ok" in out.stdout and "empty 0" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}

    def product(W):
        res = []
        for c in range(P):
            y = hm.matvec(W, xs[c], t)
            res.append([(v + half) % t - half for v in y + [0] * (M - len(y))] * (n // M))
        return np.array(res, dtype=np.int64)
    want = {"fresh": rows, "many_0": rows, "many_1": gm.rotate_rows_slots(rows, 1), "many_5": gm.rotate_rows_slots(rows, 5),
            "many_7": gm.rotate_rows_slots(rows, 7), "many_5_ntt": gm.rotate_rows_slots(rows, 5), "rows_1": gm.rotate_rows_slots(rows, 1),
            "rows_5": gm.rotate_rows_slots(rows, 5), "matvec_8x8": product(W8), "matvec_5x8": product(W5), "matvec_8x8_ntt": product(W8),
            "matvec_zero": np.zeros_like(rows)}
    assert set(budgets) == set(want)
    for name, w in want.items():
        if name != "matvec_zero":                                                              # (the sum of no terms is the transparent zero ciphertext)
            assert budgets[name] >= 1, (name, budgets[name])
        got = np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64).reshape(n, P)
        assert np.array_equal(got.T, w), name
    # the hoisted rotation's noise follows the direct rotation's law: within the measure's one bit
    assert budgets["many_1"] >= budgets["rows_1"] - 1 and budgets["many_5"] >= budgets["rows_5"] - 1, budgets
    assert throws == {"no_batching_many": "logic_error", "no_batching_matvec": "logic_error", "no_keys_many": "invalid_argument",
                      "no_keys_matvec": "invalid_argument", "steps_too_large": "invalid_argument", "missing_key_many": "invalid_argument",
                      "bad_M": "invalid_argument", "M_too_large": "invalid_argument", "W_too_large": "invalid_argument",
                      "missing_key_matvec": "invalid_argument", "bad_form": "invalid_argument"}
