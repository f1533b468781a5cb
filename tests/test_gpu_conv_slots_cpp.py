"""The host classes' convSlots (crcnn_amd/host/hoist_host.cpp, its conv case): one 12 x 12 image as a channel plane, a 3 x 3 convolution with a folded 2 x 2 sum
pool and a second 3 x 3 convolution at the returned dilation, with the keys of convSlotsElements only, against the integer convolution computed by the program
and again here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conv_slots_model as cm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_conv_slots():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "hoist_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds hoist_host"
    n, t = 4096, 65537
    rng = np.random.RandomState(29)
    img = rng.randint(0, 4, size=(1, 12, 12)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64)
    w2 = rng.randint(-2, 3, size=(3, 2, 3, 3)).astype(np.int64)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    img.tofile(os.path.join(d, "image.i64")); w1.tofile(os.path.join(d, "w1.i64")); w2.tofile(os.path.join(d, "w2.i64"))
    out = subprocess.run([driver, d, "conv"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "hoist_host conv ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    convs = {l[1]: l[2] for l in lines if l[0] == "conv"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    keys = [l for l in lines if l[0] == "keys"][0]
    y1 = cm.conv_direct(img, w1, 2)
    y2 = cm.conv_direct(y1, w2, 1)
    assert y1.shape == (2, 5, 5) and y2.shape == (3, 3, 3) and int(np.abs(y2).max()) < t // 2
    want = {"conv_fresh": img, "conv_1": y1, "conv_2": y2, "conv_2_ntt": y2}
    assert set(budgets) == set(want) == set(convs)
    for name, w in want.items():
        assert convs[name] == "equal", name
        assert budgets[name] >= 1, (name, budgets[name])
        got = np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64).reshape(w.shape)
        assert np.array_equal(got, w.astype(np.int64)), name
    # 16 taps of the pooled first layer and 9 of the second at dilation 2 share the steps 0, 2, 24, 26: 15 + 9 - 4 keys
    assert keys[1] == "conv" and keys[3] == "elements" and int(keys[4]) == 20 and int(keys[2]) % 20 == 0 and int(keys[2]) > 0
    assert throws == {"no_batching_conv": "logic_error", "no_slot_encoding": "logic_error", "no_keys_conv": "invalid_argument", "bad_weights": "invalid_argument",
                      "bad_M_conv": "invalid_argument", "plane_does_not_fit": "invalid_argument", "missing_key_conv": "invalid_argument",
                      "bad_form_conv": "invalid_argument", "not_planes": "invalid_argument", "plane_too_large": "invalid_argument"}
