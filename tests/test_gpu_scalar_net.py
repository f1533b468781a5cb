"""Slot-batched networks through the host classes with the scalar limb form (CRC_NTTLS) off and on: crcnn_amd/host/scalar_host.cpp runs PlainModelTiny and
approx_poly.net at the n = 256 golden parameters, five images per ciphertext, unfused and fused, under scalar_mac = 0 and 1.  The decrypted slot integers are the
integer network's, the output ciphertexts are the same bits either way, and with the key on conv2 and the dense layers run the scalar kernel on weights n times
smaller."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import slots_model as sm
from test_gpu_slots import NETS

pytestmark = pytest.mark.gpu


def round_up(v, m):
    return -(-v // m) * m


def steps_of(zd, xf, yf):
    return xf * -(-(yf * round_up(zd, 4)) // 32) if zd < 32 else xf * yf * (round_up(zd, 32) // 32)


@pytest.mark.parametrize("desc,model,golden,in_bits,w_bits", NETS, ids=[n[0] for n in NETS])
def test_scalar_form_through_the_host_classes(desc, model, golden, in_bits, w_bits):
    import crcnn_amd as ca
    from crcnn_amd import netrun
    from netcommon import GOLD, load_net_golden, model_weights
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "crcnn_amd", "lib", "scalar_host")
    g = load_net_golden(golden)
    n, k, S = g["n"], len(g["q"]), 5
    t = ca.Engine.slots_prime(n, 20)
    path = desc if not desc.endswith(".net") else os.path.join(GOLD, "activations", desc)
    layers = netrun.load_description(path)
    zd, xd, yd = layers.input_shape
    images = np.random.RandomState(17).uniform(-1, 1, size=(S, zd, xd, yd)).astype(np.float32)
    d = tempfile.mkdtemp()
    np.array([n, k, t] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    h5 = os.path.join(GOLD, "models", model + ".h5")
    out = subprocess.run([driver, path, h5, d, str(S), str(in_bits), str(w_bits)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "scalar_host ok" in out.stdout
    want, _ = sm.network_forward(list(layers), model_weights(model), images, t, in_bits, w_bits)
    digest, macs = {}, {}
    for line in out.stdout.splitlines():
        f = line.split(" ")
        if f[0] == "run":
            digest[(int(f[1]), int(f[2]))] = f[4]
        elif f[0] == "mac":
            macs.setdefault((int(f[1]), int(f[2])), []).append((tuple(int(v) for v in f[4:12]), int(f[12]), " ".join(f[13:])))
    assert sorted(digest) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for key in (0, 1):
        for fused in (0, 1):
            got = np.fromfile(os.path.join(d, f"slots_{key}_{fused}.i64"), dtype=np.int64).reshape(S, -1)
            assert got.tolist() == want, (key, fused)
    for fused in (0, 1):
        assert digest[(0, fused)] == digest[(1, fused)], f"fused={fused}: the output ciphertexts differ between scalar_mac off and on"
        off, on = macs[(0, fused)], macs[(1, fused)]
        assert len(off) == len(on) >= 3
        scalar_layers = 0
        for (geom, bytes_off, name_off), (geom_on, bytes_on, name_on) in zip(off, on):
            assert geom == geom_on
            zd_, _, _, _, _, xf, yf, nf = geom
            assert "CRC_NTTLS" not in name_off
            if zd_ == 1:                                          # conv1 keeps its own kernel
                assert name_on == name_off and bytes_on == bytes_off
                continue
            scalar_layers += 1
            assert "CRC_NTTLS" in name_on and "mfma_mac2w_kernel" in name_on, (geom, name_on)
            bias = 2 * nf * k * n * 8                             # coefficient- and NTT-form bias rows
            scalar = k * round_up(steps_of(zd_, xf, yf), 2) * 7 * round_up(nf, 64) * 32
            assert bytes_on == scalar + bias, (geom, bytes_on)
            # the row path holds n times the limb container, or one canonical / packed row of k n words per weight
            rows = n * scalar if "CRC_NTTL)" in name_off else nf * zd_ * xf * yf * k * n * 8
            assert bytes_off == rows + bias, (geom, name_off, bytes_off)
        assert scalar_layers >= 3                                     # conv2, fc3, fc4
