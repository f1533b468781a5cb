"""The hoisted conv + pool pair without a GPU.

crc_plan_hoist_pool on host-only engines: which pairs Network::fuse() / netrun.py hoist (PlainModelTiny's conv2 + pool2 behind the fused conv1 + pool1) and which
they leave to the weight fold.

The algebra on the CPU oracle at n = 256, k = 2: conv, pool, conv, pool in the reference's order against the hoisted pair -- the first convolution with its own
pool and then the second pool's stride-1 window sum folded into its weights, the second convolution with its own window, the pool's stride, the divisor in its
weights and the bias of every window position -- residue for residue.  The folds are done here in Python integers (what k_fold_pool computes on the device)."""
import numpy as np
import pytest

import crcnn_amd as ca
from benchkit import geometry
from benchkit.configs import CONFIGS
from crcnn_amd.netrun import TOPOLOGIES
from netcommon import load_net_golden
from oracle import orc

TINY_UP, TINY_CONV, POOL22 = (1, 28, 28, 2, 2, 6, 6, 32), (32, 12, 12, 1, 1, 5, 5, 64), (2, 2, 2, 2)


def host_engine(cfg_name):
    cfg = CONFIGS[cfg_name]
    return ca.Engine(cfg["n"], ca.default_coeff_modulus_128(cfg["n"])[:cfg["k"]], cfg["t"], device=-1)


def test_plan_hoists_tiny_conv2():
    T = host_engine("tiny4096")
    assert T.plan_hoist_pool(TINY_UP, TINY_CONV, POOL22, 128, matrix_cores=True) is True
    assert T.plan_hoist_pool(TINY_UP, TINY_CONV, POOL22, 128, matrix_cores=False) is True
    assert T.plan_hoist_pool(TINY_UP, TINY_CONV, POOL22, 64, matrix_cores=False) is True        # tiny4096_valu's chunk
    # the weight fold keeps its answer
    assert T.plan_fold_pool(*TINY_CONV, *POOL22) is True
    plan = geometry.fused_plan(T, "PlainModelTiny")
    geo = lambda a: tuple(a[k] for k in ("zd", "xd", "yd", "xs", "ys", "xf", "yf", "nf"))
    assert [pl[1] for pl in plan[:2]] == ["pool1_features.conv1+pool1", "pool2_features.conv2+pool2"]
    assert geo(plan[0][2]) == (1, 28, 28, 2, 2, 8, 8, 32) and plan[0][4] == (32, 11, 11)
    assert geo(plan[1][2]) == (32, 11, 11, 2, 2, 5, 5, 64) and plan[1][3] == (32, 11, 11) and plan[1][4] == (64, 4, 4)
    T.close()


def test_plan_refuses():
    T = host_engine("tiny4096")
    # a stride-2 convolution (30 x 30 -> 13 x 13 in front of it)
    assert T.plan_hoist_pool((1, 30, 30, 2, 2, 6, 6, 32), (32, 13, 13, 2, 2, 5, 5, 64), POOL22, 128) is False
    # the window of the one-channel layer in front would grow to 10 x 10: no matrix-core kernel takes it
    up, conv = (1, 28, 28, 2, 2, 8, 8, 32), (32, 11, 11, 1, 1, 4, 4, 64)
    assert T.plan_mac(*up, 128) == ca.NTTL1 and T.plan_mac(1, 28, 28, 2, 2, 10, 10, 32, 128) != ca.NTTL1
    assert T.plan_fold_pool(*conv, *POOL22) is True
    assert T.plan_hoist_pool(up, conv, POOL22, 128) is False
    # a first-layer conv + pool has nothing in front of it
    assert T.plan_hoist_pool(None, (1, 28, 28, 1, 1, 5, 5, 32), POOL22, 128) is False
    # a stride-1 pool removes no multiply-accumulates
    assert T.plan_hoist_pool(TINY_UP, TINY_CONV, (1, 1, 2, 2), 128) is False
    # the layer in front must produce this layer's input
    assert T.plan_hoist_pool((1, 28, 28, 2, 2, 6, 6, 16), TINY_CONV, POOL22, 128) is False
    T.close()


@pytest.mark.parametrize("cfg_name", ["approx8192", "wopad16384"])
def test_plan_leaves_the_other_models_alone(cfg_name):
    """ApproxPlainModel / PlainModelWoPad: conv1 + pool1 is the first layer, and a Square follows conv2 (stride 2)"""
    E = host_engine(cfg_name)
    topo = TOPOLOGIES[CONFIGS[cfg_name]["model"]]
    geo = lambda a: tuple(a[k] for k in ("zd", "xd", "yd", "xs", "ys", "xf", "yf", "nf"))
    pairs = 0
    for i, (kind, name, a) in enumerate(topo[:-1]):
        if kind == "conv" and topo[i + 1][0] in ("pool", "avgpool"):
            pa = topo[i + 1][2]
            up = geo(topo[i - 1][2]) if i and topo[i - 1][0] == "conv" else None
            for mc in (True, False):
                assert E.plan_hoist_pool(up, geo(a), (pa["xs"], pa["ys"], pa["xf"], pa["yf"]), CONFIGS[cfg_name]["chunk"], matrix_cores=mc) is False
            pairs += 1
    assert pairs == 1
    plan = geometry.fused_plan(E, CONFIGS[cfg_name]["model"])
    assert geo(plan[0][2]) == (1, 28, 28, 2, 2, 7, 7, 20) and geo(plan[1][2]) == (20, 11, 11, 2, 2, 3, 3, 50)
    E.close()


# ---- the algebra ---------------------------------------------------------------------------------------------------------------------------------------------
def mulmod(a, b, q):
    return ((a.astype(object) * b.astype(object)) % q).astype(np.uint64)


def fold_pool(O, w, bias, cxs, cys, pxf, pyf, div):
    """k_fold_pool: w [nf][zd][xf][yf][k][n], bias [nf][k][n] NTT-form rows, div [k][n] or None -> the pooled kernel and bias"""
    nf, zd, xf, yf = w.shape[:4]
    xf2, yf2 = (pxf - 1) * cxs + xf, (pyf - 1) * cys + yf
    out = np.zeros((nf, zd, xf2, yf2) + w.shape[4:], dtype=np.uint64)
    b2 = np.zeros_like(bias)
    for i, q in enumerate(O.q):
        acc = np.zeros((nf, zd, xf2, yf2, O.n), dtype=object)
        for a in range(pxf):
            for b in range(pyf):
                acc[:, :, a * cxs:a * cxs + xf, b * cys:b * cys + yf] += w[..., i, :].astype(object)
        acc %= q
        bb = (bias[:, i].astype(object) * (pxf * pyf)) % q
        if div is not None:
            acc = (acc * div[i].astype(object)) % q
            bb = (bb * div[i].astype(object)) % q
        out[..., i, :] = acc.astype(np.uint64); b2[:, i] = bb.astype(np.uint64)
    return out, b2


def hoist_pool(O, w, bias, pxf, pyf, div):
    """the downstream half (crc_conv2d_hoist_pool): the window stays, w' = div w, b' = div pxf pyf b"""
    out, b2 = w.copy(), np.zeros_like(bias)
    for i, q in enumerate(O.q):
        bb = (bias[:, i].astype(object) * (pxf * pyf)) % q
        if div is not None:
            out[..., i, :] = mulmod(w[..., i, :], np.broadcast_to(div[i], w[..., i, :].shape), q)
            bb = (bb * div[i].astype(object)) % q
        b2[:, i] = bb.astype(np.uint64)
    return out, b2


def bias_rows(O, plains):
    """NTT-form rows of what add_plain adds to poly 0, per filter"""
    out = np.zeros((len(plains), O.k, O.n), dtype=np.uint64)
    for f, p in enumerate(plains):
        d = O.add_plain(O.ct(), p)[0]
        for i in range(O.k):
            out[f, i] = O.ntt_fwd(i, d[i])
    return out


def conv_rows(O, x, w, b_rows, xs, ys):
    """a convolution whose bias is given as NTT-form rows (a folded bias is no plaintext's lift): the oracle's layer with a zero bias, then the rows on poly 0"""
    y = O.conv(x, w, np.zeros((w.shape[0], O.n), dtype=np.uint64), xs, ys)
    for f in range(w.shape[0]):
        for i, q in enumerate(O.q):
            y[f, :, :, 0, i] = (y[f, :, :, 0, i] + O.ntt_inv(i, b_rows[f, i])) % np.uint64(q)
    return y


@pytest.fixture(scope="module")
def setting():
    g = load_net_golden("tiny256")
    O = orc.Oracle(g["n"], g["q"], g["t"])
    assert O.n == 256 and O.k == 2
    sk, pk = O.keygen(31)
    rng = np.random.RandomState(5)
    x = O.encrypt_many(pk, O.encode_many(rng.uniform(-1, 1, size=(1, 16, 16)).astype(np.float32)).reshape(1, 16, 16, O.n), 700)
    enc = lambda a: O.encode_many(np.asarray(a, dtype=np.float32)).reshape(np.shape(a) + (O.n,))
    w1, b1 = enc(rng.normal(0, 0.3, size=(2, 1, 5, 5))), enc(rng.normal(0, 0.1, size=2))
    # the first pair, shared by the cases and left unchanged: 5 x 5 convolution of the 16 x 16 image, 2 x 2 / 2 average pool -> 2 channels of 6 x 6
    div1 = O.encode(0.25)[0]
    t2 = O.pool(O.conv(x, O.plains_to_ntt(w1), b1, 1, 1), 2, 2, 2, 2, div_plain=div1)
    return O, rng, enc, x, O.plains_to_ntt(w1), bias_rows(O, b1), O.plain_to_ntt(div1), t2


@pytest.mark.parametrize("xf,avg", [(5, True), (5, False), (3, True)], ids=["5x5-avg", "5x5-sum", "3x3-avg"])
def test_hoisted_pair_equals_conv_pool_conv_pool(setting, xf, avg):
    O, rng, enc, x, w1n, b1n, div1n, t2 = setting
    w2, b2 = enc(rng.normal(0, 0.3, size=(3, 2, xf, xf))), enc(rng.normal(0, 0.1, size=3))
    div2 = O.encode(0.25)[0] if avg else None
    want = O.pool(O.conv(t2, O.plains_to_ntt(w2), b2, 1, 1), 2, 2, 2, 2, div_plain=div2)
    assert want.shape[:3] == (3, (6 - xf + 1) // 2, (6 - xf + 1) // 2)
    # conv1 + pool1 as one convolution (6 x 6 / 2), then pool2's stride-1 window sum folded into it as well (8 x 8 / 2): S, 5 x 5
    w1f, b1f = fold_pool(O, w1n, b1n, 1, 1, 2, 2, div1n)
    w1s, b1s = fold_pool(O, w1f, b1f, 2, 2, 2, 2, None)
    assert w1s.shape[2:4] == (8, 8)
    S = conv_rows(O, x, w1s, b1s, 2, 2)
    assert S.shape[:3] == (2, 5, 5)
    # the weight-folded pair computes the same tensor: the check of the helpers above
    w2f, b2f = fold_pool(O, O.plains_to_ntt(w2), bias_rows(O, b2), 1, 1, 2, 2, O.plain_to_ntt(div2) if avg else None)
    assert np.array_equal(conv_rows(O, conv_rows(O, x, w1f, b1f, 2, 2), w2f, b2f, 2, 2), want)
    w2h, b2h = hoist_pool(O, O.plains_to_ntt(w2), bias_rows(O, b2), 2, 2, O.plain_to_ntt(div2) if avg else None)
    got = conv_rows(O, S, w2h, b2h, 2, 2)
    assert got.shape == want.shape and np.array_equal(got, want)
