"""GPU exactness of the limb GEMM's epilogue (kernels_mfma.hip): the one-pass centred reduction, the paired digit stores into the staging area and the copy-out to a
dense consumer's limb tensor, at the smallest shapes at which each store path can go wrong, with results ON the centring boundaries.

Shapes (n = 128): 2P = 32 (two images per tile, ragged last tile), 2P = 4 (the smallest paired-store case; filters past nf written as zero), P = 1 dense -> dense
(byte stores, two row tiles, the second with one image), 2P = 18 (does not divide 64: the canonical slot-major result and the conversion kernel).  Every shape runs
on moduli with a fold constant and on a pair of which one has none (its outputs take the canonical sequence), on both kernel variants, and is read back both as the
consumer's limb tensor (CRC_NTTL, over a buffer pre-filled with 0x55) and as canonical residues (CRC_NTT: the slot-major result).

Operands.  "unit": every filter's weights are 1 in one term and 0 elsewhere, x and the bias rows are drawn from {0, 1, (q-1)/2, (q+1)/2, q-1}: an output is
x + b mod q and lands on 0, (q-1)/2, (q+1)/2, q-1 and their neighbours.  "unit_image": the weight of that term is 2^-64 mod q -- its limb-form image (w 2^64 mod q,
what limb_pack_weights digitises) is exactly 1, the smallest diagonals there are -- and x = e 2^64 mod q for e from the same set: the output is e + b again.
"random": uniform residues everywhere.

Reference: the convolution in numpy, exact -- residues split into three 19-bit limbs, the nine limb products as float64 matrix products (each sum below
2^38 T < 2^53), recombined mod q in 64-bit words -- and, for the unit kinds, also the selected x + b directly.  The expected limb tensor is cut from it here
(balanced base-256 digits of the centred representatives, the consumer's [k][n][7][ch / 32][B][2][32] layout).  Nothing expected comes from the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
Q55, Q54 = 0x7fffffff380001, 0x3fffffff000001            # 2^b - f, f < 2^26: fold constant
Q55NF = 0x7fffffbffd0001                                 # 55 bits, 2^55 - q > 2^26: no fold constant
QSETS = {"fold": [Q55, Q54], "q55nofold": [Q55NF, Q55]}
SHAPES = {
    # zd, xd, yd, xs, ys, xf, yf, nf, B
    "2P=32": (32, 6, 6, 1, 1, 3, 3, 64, 3),
    "2P=4": (32, 2, 3, 1, 1, 2, 2, 50, 5),
    "P=1": (70, 1, 1, 1, 1, 1, 1, 10, 33),
    "2P=18": (32, 5, 5, 1, 1, 3, 3, 64, 2),
}
KINDS = ["unit", "unit_image", "random"]


def edge_values(q):
    return np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 1], dtype=np.uint64)


def mod_matmul(A, W, q):
    """(A @ W) mod q, exact: A [S][M][T], W [S][T][F] uint64 residues below q < 2^57, T < 2^15"""
    import torch                                              # (batched float64 products on the CPU: numpy's own take seconds at these sizes)
    mask = np.uint64((1 << 19) - 1)
    al = [torch.from_numpy(np.ascontiguousarray(((A >> np.uint64(19 * i)) & mask).astype(np.float64))) for i in range(3)]
    wl = [torch.from_numpy(np.ascontiguousarray(((W >> np.uint64(19 * i)) & mask).astype(np.float64))) for i in range(3)]
    assert A.shape[-1] < (1 << 15)
    qq = np.uint64(q)
    acc = None
    for lvl in range(4, -1, -1):                              # Horner over the limb weight 2^(19 lvl)
        s = sum(torch.bmm(al[i], wl[lvl - i]) for i in range(3) if 0 <= lvl - i < 3).numpy().astype(np.uint64) % qq
        if acc is None:
            acc = s
        else:
            for sh in (8, 8, 3):                              # acc < 2^55: every shifted value fits the word
                acc = (acc << np.uint64(sh)) % qq
            acc = (acc + s) % qq
    return acc


def make_case(shape, q, kind, seed):
    """x [B][zd][xd][yd][2][k][n], w [nf][zd][xf][yf][k][n], b [nf][k][n] and the exact y [B][nf][P][2][k][n]"""
    zd, xd, yd, xs, ys, xf, yf, nf, B = shape
    k, n = len(q), N
    rng = np.random.default_rng(seed)
    xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
    x = np.empty((B, zd, xd, yd, 2, k, n), dtype=np.uint64)
    w = np.zeros((nf, zd, xf, yf, k, n), dtype=np.uint64)
    b = np.empty((nf, k, n), dtype=np.uint64)
    term = rng.integers(0, zd * xf * yf, size=nf)          # the one non-zero term of every filter (unit kinds)
    tz, tx, ty = np.unravel_index(term, (zd, xf, yf))
    for i, qi in enumerate(q):
        if kind == "random":
            x[..., i, :] = rng.integers(0, qi, size=x.shape[:-2] + (n,), dtype=np.uint64)
            w[..., i, :] = rng.integers(0, qi, size=w.shape[:-2] + (n,), dtype=np.uint64)
            b[:, i] = rng.integers(0, qi, size=(nf, n), dtype=np.uint64)
            continue
        ev = edge_values(qi)
        e = ev[rng.integers(0, len(ev), size=x.shape[:-2] + (n,))]
        if kind == "unit":
            x[..., i, :] = e
            w[np.arange(nf), tz, tx, ty, i, :] = 1
        else:                                                # the weight's limb image is 1; x carries the factor 2^64
            R = (1 << 64) % qi
            x[..., i, :] = np.array([int(v) * R % qi for v in ev], dtype=np.uint64)[np.searchsorted(ev, e)]
            w[np.arange(nf), tz, tx, ty, i, :] = pow(1 << 64, -1, qi)
            assert (pow(1 << 64, -1, qi) << 64) % qi == 1
        b[:, i] = ev[rng.integers(0, len(ev), size=(nf, n))]
    y = np.empty((B, nf, xo * yo, 2, k, n), dtype=np.uint64)
    for i, qi in enumerate(q):
        xi = x[..., i, :]                                     # [B][zd][xd][yd][2][n]
        pat = np.stack([np.stack([xi[:, :, kx:kx + (xo - 1) * xs + 1:xs, ky:ky + (yo - 1) * ys + 1:ys] for ky in range(yf)], axis=2) for kx in range(xf)], axis=2)
        A = pat.transpose(7, 0, 4, 5, 6, 1, 2, 3).reshape(n, B * xo * yo * 2, zd * xf * yf)          # pat [B][zd][xf][yf][xo][yo][2][n]
        W = w[..., i, :].transpose(4, 1, 2, 3, 0).reshape(n, zd * xf * yf, nf)
        r = mod_matmul(A, W, qi).reshape(n, B, xo * yo, 2, nf)
        r[:, :, :, 0, :] = (r[:, :, :, 0, :] + b[:, i].T[:, None, None, :]) % np.uint64(qi)            # the bias rows go to poly 0
        y[:, :, :, :, i, :] = r.transpose(1, 4, 2, 3, 0)
        if kind != "random":                                  # the reference against the selected term itself
            sel = xi[:, tz, :, :, :, :]                       # [B][nf][xd][yd][2][n]
            want = np.empty((B, nf, xo, yo, 2, n), dtype=np.uint64)
            for f in range(nf):
                want[:, f] = sel[:, f, tx[f]:tx[f] + (xo - 1) * xs + 1:xs, ty[f]:ty[f] + (yo - 1) * ys + 1:ys]
            if kind == "unit_image":
                Rinv = pow(1 << 64, -1, qi)
                lut = {int(v) * ((1 << 64) % qi) % qi: int(v) for v in edge_values(qi)}
                assert all(int(v) * Rinv % qi == lut[int(v)] for v in lut)
                keys = np.array(sorted(lut), dtype=np.uint64)
                want = np.array([lut[int(v)] for v in keys], dtype=np.uint64)[np.searchsorted(keys, want)]
            want[..., 0, :] = (want[..., 0, :] + b[:, i][None, :, None, None, :]) % np.uint64(qi)
            assert np.array_equal(y[:, :, :, :, i, :], want.reshape(B, nf, xo * yo, 2, n))
    return x, w, b, y


def limb_tensor_dense(y, q):
    """y [B][C][P][2][k][n] canonical -> the dense consumer's limb tensor [k][n][7][ch / 32][B][2][32] int8 (channel = c P + p, zero padded to a multiple of 32)"""
    B, C, P, _, k, n = y.shape
    qv = np.array(q, dtype=np.int64).reshape(k, 1)
    v = y.astype(np.int64)
    v = np.where(v > (qv >> 1), v - qv, v)
    assert (np.abs(v) <= (qv >> 1)).all()
    ch, chp = C * P, -(-C * P // 32) * 32
    out = np.zeros((7, B, chp, 2, k, n), dtype=np.int8)
    for l in range(7):
        d = ((v + 128) & 255) - 128
        out[l, :, :ch] = d.reshape(B, ch, 2, k, n).astype(np.int8); v = (v - d) >> 8
    assert not v.any()
    return np.ascontiguousarray(out.reshape(7, B, chp // 32, 32, 2, k, n).transpose(5, 6, 0, 2, 1, 4, 3))


_ENGINES, _CASES = {}, {}


@pytest.fixture(scope="module")
def engines():
    yield _ENGINES
    for E in _ENGINES.values():
        E.close()
    _ENGINES.clear(); _CASES.clear()


def case(sname, qname, kind):
    """operands and expected results of a case: computed once, shared by the kernel variants, never written to"""
    key = (sname, qname, kind)
    if key not in _CASES:
        x, w, b, y = make_case(SHAPES[sname], QSETS[qname], kind, seed=sorted(SHAPES).index(sname) * 16 + KINDS.index(kind) * 2 + sorted(QSETS).index(qname))
        if kind != "random":                                  # the boundaries are hit: every centring decision of the epilogue is exercised
            for i, qi in enumerate(QSETS[qname]):
                got = set(np.unique(y[..., i, :]).tolist())
                assert {0, (qi - 1) // 2, (qi + 1) // 2, qi - 1, 1} <= got
        xl = limb_tensor_dense(y, QSETS[qname])
        for a in (x, w, b, y, xl):
            a.setflags(write=False)
        _CASES[key] = (x, w, b, y, xl)
    return _CASES[key]


@pytest.mark.parametrize("variant", [2, 1], ids=["two-workgroups-per-CU", "one-workgroup-per-CU"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qname", list(QSETS))
@pytest.mark.parametrize("sname", list(SHAPES))
def test_limb_epilogue_on_centring_boundaries(engines, request, sname, qname, kind, variant):
    import crcnn_amd as ca
    q = QSETS[qname]
    if qname not in engines:
        engines[qname] = ca.Engine(N, q, 1 << 20, device=0)
    E = engines[qname]
    E.set_tuning("mfma_variant", variant); request.addfinalizer(lambda: E.set_tuning("mfma_variant", 2))
    zd, xd, yd, xs, ys, xf, yf, nf, B = SHAPES[sname]
    x, w, b, y, xl = case(sname, qname, kind)
    P = y.shape[2]
    d_x, d_w, d_b = E.upload(x), E.upload(w), E.upload(b)
    d_wl = E.alloc(E.limb_weights_bytes(nf, zd, xf, yf)); E.limb_pack_weights(d_w, nf, zd, xf, yf, d_wl)
    bufs = [d_x, d_w, d_b, d_wl]
    # the consumer's limb tensor, written by the GEMM kernel itself where 2P divides 64
    nb = E.limb_tensor_bytes(B, nf * P)
    assert nb == xl.nbytes
    d_l = E.alloc(nb); E.L.crc_memset(E.c, E.p(d_l), 0x55, nb, E.stream)
    d_work = E.alloc(E.conv2d_forms_work_bytes(B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL, ca.NTTL))
    E.conv2d(d_x, d_wl, d_b, B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL, d_l, d_work, w_form=ca.NTTL)
    got_l = E.download(d_l, xl.shape, dtype=np.int8)
    bufs += [d_l, d_work]
    # canonical residues: the slot-major result of the same kernel, transposed
    d_y = E.alloc(y.nbytes); E.L.crc_memset(E.c, E.p(d_y), 0x55, y.nbytes, E.stream)
    d_work2 = E.alloc(E.conv2d_forms_work_bytes(B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTTL, ca.NTT))
    E.conv2d(d_x, d_wl, d_b, B, zd, xd, yd, xs, ys, xf, yf, nf, ca.NTT, ca.NTT, d_y, d_work2, w_form=ca.NTTL)
    got_y = E.download(d_y, y.shape)
    for d in bufs + [d_y, d_work2]:
        d.free()
    bad = np.argwhere(got_l != xl)
    assert bad.size == 0, f"limb tensor: {len(bad)} wrong bytes, first at [k, n, plane, block, image, poly, byte] = {bad[0].tolist()}: {got_l[tuple(bad[0])]} for {xl[tuple(bad[0])]}"
    bad = np.argwhere(got_y != y)
    assert bad.size == 0, f"canonical result: {len(bad)} wrong residues, first at [B, f, p, poly, k, n] = {bad[0].tolist()}"
