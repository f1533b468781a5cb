"""GPU exactness of the hoisted conv + pool pair (crc_plan_hoist_pool, Network::fuse() step 1a) at the shapes PlainModelTiny runs it at, n = 256, k = 2:
  the one-channel matrix-core kernel at 8 x 8 / 2 on 28 x 28 (121 positions: 242 rows, a ragged 16th row tile), as NTT-form rows and as the limb tensor it hands to
  the convolution behind it;
  the limb GEMM at 32 channels, 11 x 11, 5 x 5 / 2, 64 filters (25 reduction steps, an odd image width), on one whole row tile (2 images) and a ragged one (3);
  both against the vector-ALU kernel on the same operands, bit for bit (random canonical residues: the kernels' exact integer arithmetic has no tolerance);
  PlainModelTiny through the C++ classes, fused: the reference's output digest, with the hoisted geometry reported by the fused layers -- and the weight-folded geometry
  and the same digest under CRC_HOIST_POOL=0; ApproxPlainModel keeps the geometry it had."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs, sha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")
N = 256
Q = load_net_golden("tiny256")["q"]


@pytest.fixture(scope="module")
def eng():
    import crcnn_amd as ca
    E = ca.Engine(N, Q, 1 << 20, device=0)
    yield E, ca
    E.close()


def rand_rows(rng, lead):
    out = np.empty(lead + (len(Q), N), dtype=np.uint64)
    for i, q in enumerate(Q):
        out[..., i, :] = rng.integers(0, q, size=lead + (N,), dtype=np.uint64)
    return out


def run_conv(E, ca, d_x, d_w, d_b, geom, B, w_form, out_form=None):
    zd, xd, yd, xs, ys, xf, yf, nf = geom
    out_form = ca.NTT if out_form is None else out_form
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    limb = out_form == ca.NTTLC
    nbytes = E.limb_tensor_bytes(B, nf, xo, yo) if limb else B * nf * xo * yo * 2 * E.k * E.n * 8
    d_y = E.alloc(nbytes)
    E.L.crc_memset(E.c, E.p(d_y), 0 if limb else 0xff, nbytes, E.stream)       # (a limb tensor's padding is nobody's to write; a u64 result left unwritten cannot pass)
    d_work = E.alloc(E.conv2d_forms_work_bytes(B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, w_form, out_form))
    E.conv2d(d_x, d_w, d_b, B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, out_form, d_y, d_work, w_form=w_form)
    E.sync()
    out = E.download(d_y, (nbytes // 8,))
    d_y.free(); d_work.free()
    return out


def test_conv1_8x8_stride2_equals_vector_alu(eng):
    """conv1+pool1 with pool2's window sum folded in: (28, 28, 2, 2, 8, 8, 32) on 2 images"""
    E, ca = eng
    geom, B = (1, 28, 28, 2, 2, 8, 8, 32), 2
    assert E.plan_mac(*geom, B) == ca.NTTL1 and E.limb_conv1_form(*geom) == 1          # 64 taps: the plane-major form
    rng = np.random.default_rng(811)
    d_x, d_w, d_b = E.upload(rand_rows(rng, (B, 28, 28, 2))), E.upload(rand_rows(rng, (32, 8, 8))), E.upload(rand_rows(rng, (32,)))
    want = run_conv(E, ca, d_x, d_w, d_b, geom, B, ca.NTT)
    d_wl = E.alloc(E.limb_conv1_weights_bytes()); E.limb_conv1_pack_weights(d_w, 32, 8, 8, d_wl)
    assert np.array_equal(run_conv(E, ca, d_x, d_wl, d_b, geom, B, ca.NTTL1), want)
    # ... and as the blocked limb tensor [slot][B][7][121][2][32] of the convolution behind: what crc_limb_pack_tensor makes of the vector-ALU result
    nb = E.limb_tensor_bytes(B, 32, 11, 11)
    d_ref = E.alloc(nb); E.L.crc_memset(E.c, E.p(d_ref), 0, nb, E.stream)
    E.limb_pack_tensor(E.upload(want), ca.NTT, B, 32, 11, 11, d_ref)
    assert np.array_equal(run_conv(E, ca, d_x, d_wl, d_b, geom, B, ca.NTTL1, ca.NTTLC), E.download(d_ref, (nb // 8,)))


@pytest.fixture(scope="module")
def conv2_operands(eng):
    E, ca = eng
    rng = np.random.default_rng(812)
    d_x = E.upload(rand_rows(rng, (3, 32, 11, 11, 2)))
    d_w, d_b = E.upload(rand_rows(rng, (64, 32, 5, 5))), E.upload(rand_rows(rng, (64,)))
    d_wl = E.alloc(E.limb_weights_bytes(64, 32, 5, 5)); E.limb_pack_weights(d_w, 64, 32, 5, 5, d_wl)
    return d_x, d_w, d_b, d_wl


@pytest.mark.parametrize("B", [2, 3])
def test_limb_gemm_5x5_stride2_on_11x11_equals_vector_alu(eng, conv2_operands, B):
    """conv2+pool2 hoisted: 32 channels, 11 x 11, 5 x 5 / 2, 64 filters; 2 images are one whole 64-row tile, 3 leave a ragged one"""
    E, ca = eng
    d_x, d_w, d_b, d_wl = conv2_operands
    geom = (32, 11, 11, 2, 2, 5, 5, 64)
    assert E.plan_mac(*geom, B) == ca.NTTL
    want = run_conv(E, ca, d_x, d_w, d_b, geom, B, ca.NTT)             # (the first B of the three images)
    assert np.array_equal(run_conv(E, ca, d_x, d_wl, d_b, geom, B, ca.NTTL), want)


# ---- the networks through the C++ classes ----------------------------------------------------------------------------------------------------------------
def run_netgeom(name, batch, head_chunk, env=None):
    g = load_net_golden(name)
    O, sk, pk, evk, img, x = make_inputs(g)
    d = tempfile.mkdtemp()
    np.array([g["n"], len(g["q"]), g["t"]] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    evk.tofile(os.path.join(d, "evk.u64")); x.tofile(os.path.join(d, "net_in.u64"))
    h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
    out = subprocess.run([DRIVER, "netgeom", g["model"], h5, d, str(batch), str(head_chunk)], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    geom = {l.split()[2]: tuple(int(v) for v in l.split()[3:]) for l in out.stdout.splitlines() if l.startswith("geom ")}
    return g, geom, np.fromfile(os.path.join(d, "out.u64"), dtype=np.uint64).reshape(batch, -1)


HOISTED = {"pool1_features.conv1+pool1": (1, 28, 28, 2, 2, 8, 8, 32), "pool2_features.conv2+pool2": (32, 11, 11, 2, 2, 5, 5, 64)}
FOLDED = {"pool1_features.conv1+pool1": (1, 28, 28, 2, 2, 6, 6, 32), "pool2_features.conv2+pool2": (32, 12, 12, 2, 2, 6, 6, 64)}


@pytest.mark.parametrize("batch,head_chunk", [(2, 0), (16, 3)])
@pytest.mark.parametrize("hoist", [True, False])
def test_tiny256_fused_digest_and_geometry(batch, head_chunk, hoist):
    g, geom, out = run_netgeom("tiny256", batch, head_chunk, env=None if hoist else {"CRC_HOIST_POOL": "0"})
    for name, want in (HOISTED if hoist else FOLDED).items():
        assert geom[name] == want, (name, geom)
    assert geom["classifier.fc3"] == (1024, 1, 1, 1, 1, 1, 1, 512)
    for b in range(batch):
        assert sha(out[b]) == g["out_sha256"], (batch, head_chunk, hoist, b)


def test_approx256_keeps_its_geometry():
    """conv2 has stride 2 and a Square behind it: nothing to hoist"""
    g, geom, out = run_netgeom("approx256", 2, 0)
    assert geom["pool1_features.conv1+pool1"] == (1, 28, 28, 2, 2, 7, 7, 20), geom
    assert geom["pool1_features.norm1+pool2_features.conv2"] == (20, 11, 11, 2, 2, 3, 3, 50), geom
    assert sha(out[0]) == g["out_sha256"] and sha(out[1]) == g["out_sha256"]
