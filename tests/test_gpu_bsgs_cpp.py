"""The host classes' matvecSlotsBsgs (crcnn_amd/host/hoist_host.cpp, its bsgs case): 16 x 16 and 11 x 16 matrices on slot-encrypted vectors with the six keys of
crc_bsgs_elements(16, 4, n), against W x mod t computed by the program and again here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import galois_hoisted_model as hm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_matvec_bsgs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "hoist_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds hoist_host"
    n, P, M, B, t = 4096, 2, 16, 4, 65537
    half = (t - 1) // 2
    rng = np.random.RandomState(23)
    xs = rng.randint(-half, half + 1, size=(P, M)).astype(np.int64)
    rows = np.tile(xs, (1, n // M))
    W16 = rng.randint(0, t, size=(16, 16)).astype(np.int64); W16[0, 0] = t - 1
    W11 = rng.randint(-half, half + 1, size=(11, 16)).astype(np.int64)                         # (any int64 is taken mod t)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    np.ascontiguousarray(rows.T).tofile(os.path.join(d, "values.i64"))
    W16.tofile(os.path.join(d, "w16.i64")); W11.tofile(os.path.join(d, "w11.i64"))
    out = subprocess.run([driver, d, "bsgs"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "hoist_host bsgs ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    products = {l[1]: l[2] for l in lines if l[0] == "product"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    keys = [l for l in lines if l[0] == "keys"][0]

    def product(W):
        res = []
        for c in range(P):
            y = hm.matvec(W, xs[c], t)
            res.append([(v + half) % t - half for v in y + [0] * (M - len(y))] * (n // M))
        return np.array(res, dtype=np.int64)
    i = np.arange(M)[:, None]; j = np.arange(M)[None, :]
    dg = (j - i) % M
    Wd = np.where((dg >= B) & (dg % B != 0), 0, W16)
    want = {"bsgs_16x16": product(W16), "bsgs_11x16": product(W11), "bsgs_16x16_ntt": product(W16), "bsgs_16x16_B16": product(Wd), "bsgs_zero": np.zeros_like(rows)}
    assert set(budgets) == set(want) == set(products)
    for name, w in want.items():
        assert products[name] == "equal", name
        if name != "bsgs_zero":
            assert budgets[name] >= 1, (name, budgets[name])
        got = np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64).reshape(n, P)
        assert np.array_equal(got.T, w), name
    kb = int(keys[2]) // 6
    assert keys[1] == "bsgs" and keys[3] == "flat" and int(keys[2]) == 6 * kb and int(keys[4]) == 15 * kb and kb > 0
    assert throws == {"no_batching_bsgs": "logic_error", "no_keys_bsgs": "invalid_argument", "bad_B": "invalid_argument", "B_too_large": "invalid_argument",
                      "bad_M_bsgs": "invalid_argument", "missing_key_bsgs": "invalid_argument", "bad_form_bsgs": "invalid_argument"}
