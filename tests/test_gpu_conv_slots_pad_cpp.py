"""The host classes' convSlots with a bias and a mask (crcnn_amd/host/hoist_host.cpp, its convpad case): one 12 x 12 image encrypted with a margin of one, a
3 x 3 'same' layer (pad 1) with a bias and the mask, then a 3 x 3 layer with pad 1 and stride 2 that reads the margin the mask zeroed, with the keys of
convSlotsElements only, against the integer convolution computed by the program and again here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conv_slots_pad_model as pm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_conv_slots_pad():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "hoist_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds hoist_host"
    n, t = 4096, 65537
    rng = np.random.RandomState(37)
    img = rng.randint(0, 4, size=(1, 12, 12)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64); b1 = np.array([3, -3], dtype=np.int64)
    w2 = rng.randint(-2, 3, size=(3, 2, 3, 3)).astype(np.int64)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    for name, a in (("image", img), ("w1", w1), ("b1", b1), ("w2", w2)):
        a.tofile(os.path.join(d, name + ".i64"))
    out = subprocess.run([driver, d, "convpad"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "hoist_host convpad ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    convs = {l[1]: l[2] for l in lines if l[0] == "conv"}
    clean = {l[1]: l[2] for l in lines if l[0] == "clean"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    keys = [l for l in lines if l[0] == "keys"][0]
    y1 = pm.conv_direct_geom(img, w1, 1, bias=b1)
    y2 = pm.conv_direct_geom(y1, w2, 1, 2)
    assert y1.shape == (2, 12, 12) and y2.shape == (3, 6, 6) and int(np.abs(y2).max()) <= 2052 < t // 2
    want = {"convpad_fresh": img, "convpad_1": y1, "convpad_2": y2, "convpad_2_ntt": y2}
    assert set(convs) == set(want) and set(budgets) == set(want) | {"convpad_1_unmasked"}
    for name, w in want.items():
        assert convs[name] == "equal", name
        assert budgets[name] >= 1, (name, budgets[name])
        got = np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64).reshape(w.shape)
        assert np.array_equal(got, w.astype(np.int64)), name
    assert clean == {"convpad_fresh": "yes", "convpad_1": "yes"}
    assert budgets["convpad_1_unmasked"] > budgets["convpad_1"]        # the mask is a full plaintext row: it costs noise, the bias does not
    # 3 x 3 with pad 1 at pitch 13: the steps +-1, +-12, +-13, +-14; at stride 2 the same taps: 8 keys for both layers
    assert keys[1] == "convpad" and keys[3] == "elements" and int(keys[4]) == 8 and int(keys[2]) % 8 == 0 and int(keys[2]) > 0
    assert throws == {"bad_bias": "invalid_argument", "too_little_margin": "invalid_argument", "pad_without_margin": "invalid_argument",
                      "negative_margin": "invalid_argument", "margin_too_large": "invalid_argument", "bad_stride": "invalid_argument"}
