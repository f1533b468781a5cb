"""The host classes' densePlanes (crcnn_amd/host/hoist_host.cpp, its planes case): one 12 x 12 image as a channel plane through convSlots (3 x 3, folded 2 x 2 sum
pool), densePlanes over the two planes of 5 x 5 pixels to 6 outputs on the input lattice, and densePlanes at Cin = 1 from that vector to 3 outputs, with the keys
of convSlotsElements and densePlanesElements only, against the integer network computed by the program and again here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conv_slots_model as cm
import dense_planes_model as dm

pytestmark = pytest.mark.gpu
Q2 = [0x7fffffff380001, 0x3fffffff000001]


def test_host_classes_dense_planes():
    import crcnn_amd as ca
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "hoist_host")
    assert os.path.exists(driver), "crcnn_amd/host/Makefile builds hoist_host"
    n, t, M = 4096, 65537, 256
    half = t // 2
    rng = np.random.RandomState(31)
    img = rng.randint(0, 3, size=(1, 12, 12)).astype(np.int64)
    w1 = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64)
    w3 = rng.randint(-2, 3, size=(6, 2, 25)).astype(np.int64)
    w4 = rng.randint(-1, 2, size=(3, 1, 6)).astype(np.int64)
    d = tempfile.mkdtemp()
    np.array([n, len(Q2), t] + Q2, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    for name, a in (("image", img), ("w1", w1), ("w3", w3), ("w4", w4)):
        a.tofile(os.path.join(d, name + ".i64"))
    out = subprocess.run([driver, d, "planes"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "hoist_host planes ok" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines()]
    budgets = {l[1]: int(l[2]) for l in lines if l[0] == "budget"}
    same = {l[1]: l[2] for l in lines if l[0] == "planes"}
    throws = {l[1]: l[2] for l in lines if l[0] == "throws"}
    keys = [l for l in lines if l[0] == "keys"][0]
    steps = [l for l in lines if l[0] == "steps"][0]
    y1 = cm.conv_direct(img, w1, 2)
    assert y1.shape == (2, 5, 5)
    centre = lambda v: [(int(x) + half) % t - half for x in v]
    v1 = centre(dm.dense_direct(w3, y1.reshape(2, 25), t))
    v2 = centre(dm.dense_direct(w4, np.array(v1, dtype=object).reshape(1, 6), t))
    out1, out2 = [2 * (12 * a + b) for a in range(2) for b in range(3)], [0, 2, 4]
    want = {"dense_1": (out1, v1), "dense_2": (out2, v2), "dense_2_ntt": (out2, v2)}
    assert set(budgets) == set(want) == set(same)
    for name, (slots, v) in want.items():
        assert budgets[name] >= 1, (name, budgets[name])                # (the parameters first: no budget, no result to compare)
        assert same[name] == "equal", name
        expect = np.zeros(M, dtype=np.int64)
        expect[slots] = v
        assert np.array_equal(np.fromfile(os.path.join(d, name + ".i64"), dtype=np.int64), expect), name
    in1 = [2 * (12 * r + c) for r in range(5) for c in range(5)]
    p1, p2 = ca.binding.dense_planes_plan(n, M, in1, out1), ca.binding.dense_planes_plan(n, M, out1, out2)
    assert [int(steps[i]) for i in (2, 4, 6)] == [16, len(p1.steps), len(p2.steps)]
    conv_elts = set(ca.binding.conv_slots_plan(n, M, 12, 12, 12, 3, 3, 1, 2).elements)
    elts = (conv_elts | set(p1.elements) | set(p2.elements)) - {1}
    H = ca.Engine(n, Q2, t, device=-1)
    assert keys[1] == "planes" and int(keys[6]) == len(elts) and int(keys[2]) == len(elts) * H.L.crc_evk_words(H.c, 16) * 8 and int(keys[4]) >= 2 * int(keys[2])
    H.close()
    assert throws == {"no_batching_planes": "logic_error", "missing_key_planes": "invalid_argument", "bad_weights_planes": "invalid_argument",
                      "bad_M_planes": "invalid_argument", "duplicate_slot": "invalid_argument", "slot_outside_M": "invalid_argument",
                      "wrong_output_count": "invalid_argument", "bad_form_planes": "invalid_argument", "not_planes_dense": "invalid_argument",
                      "no_slots": "invalid_argument"}
