"""The 64-bit row transform at every kernel, ring size and modulus-width class ntt_launch (crcnn_amd/csrc/kernels.hip) tells apart, bit for bit against the CPU oracle
and against the transform's definition in Python integers.  A class is the set [p, 0x3fffffff000001] (k = 2): the lazy butterflies run only when EVERY modulus of a
launch has 45..57 bits, the inverse butterflies that do not halve only when every modulus is below 2^55, the lazily folded products only from 53 bits on.  Plain
transforms on every ring from 64 to 16384, the fused forms (multiply_plain, both device encryptors, square / multiply with relinearisation, a convolution with bias)
on 1024, 2048, 8192 and 16384.  Which kernel a case reaches is decided by ntt_select (crcnn_amd/csrc/ntt_select.h), whose map from (ring, class, request) to
kernel tests/test_ntt_select_cpu.py checks row by row on the CPU; this test cannot see the choice, only its result -- profiles/ntt_paths_kernels.md records the
instantiations it launched, DESIGN.md has the map as a table.  Nothing is skipped: the engine admits every combination below.

Reference of the public-key device encryptor: crc_encrypt_dev_* has NO bit-exact host twin (include/crcnn_hip.h: "same laws as crc_encrypt, different bits"), so
its NTT-form result (the fused product of the wave-local kernel, FMA 1) is pinned to the oracle's transform of its own coefficient-form result of the same (key,
stream), and both decrypt under the oracle to the plaintext.  The secret-key encryptor is compared with its host twin."""
import numpy as np
import pytest

from bfv_multiply_model import MultiplyModel

pytestmark = pytest.mark.gpu

Q54 = 0x3fffffff000001
CLASSES = {"w44": (0xfffffdf8001, 44), "w45": (0x100000020001, 45), "w52": (0xffffffff58001, 52), "w53": (0x1ffffffff38001, 53), "w55": (0x7fffffffe90001, 55),
           "w56": (0x80000000068001, 56), "w57": (0x1fffffffffc0001, 57), "w58": (0x200000000208001, 58), "w60": (0xffffffffffe8001, 60)}
T = 1 << 20
PLAIN_RINGS = [64, 128, 512, 1024, 2048, 4096, 8192, 16384]
FUSED_RINGS = [1024, 2048, 8192, 16384]
UNSUPPORTED = -4                                             # CRC_ERR_UNSUPPORTED (include/crcnn_hip.h)


def is_prime(p):
    """deterministic Miller-Rabin for p < 3.3 10^24 (the first twelve primes as bases)"""
    if p < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in bases:
        if p % b == 0:
            return p == b
    d, s = p - 1, 0
    while d % 2 == 0:
        d //= 2; s += 1
    for b in bases:
        x = pow(b, d, p)
        if x in (1, p - 1):
            continue
        for _ in range(s - 1):
            x = x * x % p
            if x == p - 1:
                break
        else:
            return False
    return True


def moduli(cls):
    p, bits = CLASSES[cls]
    assert p.bit_length() == bits and is_prime(p) and p % 32768 == 1, hex(p)
    assert Q54.bit_length() == 54 and is_prime(Q54) and Q54 % 32768 == 1
    return [p, Q54]


def brev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2)


def by_definition(row, psi, q, j):
    """out[j] = Sum_s a_s psi^((2 bitrev(j) + 1) s) mod q, Horner from the top coefficient"""
    n = len(row)
    w = pow(int(psi), 2 * brev(j, n.bit_length() - 1) + 1, q)
    acc = 0
    for a in row[::-1]:
        acc = (acc * w + int(a)) % q
    return acc


def rand_rows(rng, q, shape_lead, n):
    """canonical random residues [..lead..][k][n]"""
    return np.stack([rng.integers(0, qi, size=tuple(shape_lead) + (n,), dtype=np.uint64) for qi in q], axis=-2)


def engines(n, cls):
    import crcnn_amd as ca
    from oracle import orc
    q = moduli(cls)
    return ca, q, ca.Engine(n, q, T, device=0), orc.Oracle(n, q, T)


def pairs(rings):
    return [pytest.param(n, c, id=f"n{n}-{c}") for n in rings for c in CLASSES]


# ------------------------------------------------------------------------------------------------------------------------------ (a) plain transforms
@pytest.mark.parametrize("n,cls", pairs(PLAIN_RINGS))
def test_plain_transforms(n, cls):
    """crc_ntt_fwd / crc_ntt_inv on edge and random rows laid out as ciphertexts of size 1, 2 and 3: the oracle's transform (itself checked against the definition
    here), the round trip, and the inverse of NTT-form rows; for w55 at three rings also the transforms over the auxiliary base"""
    ca, q, E, O = engines(n, cls)
    k = len(q)
    for i in range(k):
        assert np.array_equal(E.table(f"root_powers:{i}"), O.table(f"root_powers:{i}")), i
    psi = [int(v) for v in O.table("root")]
    rng = np.random.default_rng(n + CLASSES[cls][1])
    qm1 = (np.array(q, dtype=np.uint64) - np.uint64(1))[:, None]
    polys = np.zeros((11, k, n), dtype=np.uint64)
    polys[1] = qm1                                               # all q - 1
    polys[2, :, 0::2] = qm1                                      # alternating (q - 1, 0)
    for u, s in enumerate((0, 1, n // 2, n - 1)):                # (q - 1) e_s: every output is a power of psi, together they touch every table entry
        polys[3 + u, :, s] = qm1[:, 0]
    polys[7:] = rand_rows(rng, q, (4,), n)
    want = np.stack([O.ct_to_ntt(p[None])[0] for p in polys])    # the one reference, shared by the three layouts below
    want.setflags(write=False)
    # the oracle's transform is the definition (one random row per modulus, in Python integers)
    for i in range(k):
        for j in (0, 1, 2, n // 2, n - 1, 37 % n):
            assert int(want[7, i, j]) == by_definition(polys[7, i], psi[i], q[i], j), (i, j)
    # 11 polynomials as ciphertexts of size 1, 2 and 3: 22, 20 and 18 rows -- never a multiple of 8
    for size, lo, cnt in ((1, 0, 11), (2, 0, 5), (3, 2, 3)):
        x = np.ascontiguousarray(polys[lo:lo + cnt * size].reshape(cnt, size, k, n))
        d = E.upload(x)
        E.ntt_fwd(d, cnt, size)
        assert np.array_equal(E.download(d, x.shape), want[lo:lo + cnt * size].reshape(x.shape)), ("forward", size)
        E.ntt_inv(d, cnt, size)
        assert np.array_equal(E.download(d, x.shape), x), ("round trip", size)
    # the same rows read as NTT-form rows: the all-(q - 1) one is the largest sum an inverse transform can see
    want_inv = np.stack([O.ct_from_ntt(p[None])[0] for p in polys])
    for size, lo, cnt in ((1, 0, 11), (3, 1, 3)):
        x = np.ascontiguousarray(polys[lo:lo + cnt * size].reshape(cnt, size, k, n))
        d = E.upload(x)
        E.ntt_inv(d, cnt, size)
        assert np.array_equal(E.download(d, x.shape), want_inv[lo:lo + cnt * size].reshape(x.shape)), ("inverse", size)
    if cls == "w55" and n in (1024, 4096, 16384):
        bsk_transforms(E, n, rng)
    E.close()


def bsk_transforms(E, n, rng):
    """crc_ntt_fwd_bsk / crc_ntt_inv_bsk on [count][kbsk][n] rows over the auxiliary base (61-bit primes: the strict butterflies and ntt_rows_inv61_kernel): the
    definition with psi = entry n/2 of the base's own table (bit-reversed index of exponent 1), and the round trip"""
    kb = E.kbsk
    bsk = [int(v) for v in E.table("bsk")]
    assert len(bsk) == kb
    psi = []
    for j in range(kb):
        tab = E.table(f"root_powers:{E.k + j}")
        assert len(tab) == n
        psi.append(int(tab[n // 2]))
        assert pow(psi[j], n, bsk[j]) == bsk[j] - 1, j             # psi^n = -1: a primitive 2n-th root
    cnt = 5
    x = rand_rows(rng, bsk, (cnt,), n)
    x[0] = 0
    x[1] = (np.array(bsk, dtype=np.uint64) - np.uint64(1))[:, None]
    d = E.upload(x)
    assert E.L.crc_ntt_fwd_bsk(E.c, E.p(d), cnt, E.stream) == 0
    got = E.download(d, x.shape)
    assert not got[0].any()
    for c in (1, 4):
        for j in range(kb):
            for o in (0, 1, 2, n // 2, n - 1, 37 % n):
                assert int(got[c, j, o]) == by_definition(x[c, j], psi[j], bsk[j], o), (c, j, o)
    assert E.L.crc_ntt_inv_bsk(E.c, E.p(d), cnt, E.stream) == 0
    assert np.array_equal(E.download(d, x.shape), x)


# ------------------------------------------------------------------------------------------------------------------------------ (b) fused forms
CNT = 5                                                          # 10 (ciphertext, modulus) pairs: one full XCD group of eight and a partial one


def operand_arrays(E, O, q, n, pk, rng):
    """five 'ciphertexts' in both forms: two fresh encryptions, and three full-range ones GIVEN in NTT form -- rows all q - 1, all 1, random.  The last three are
    not valid encryptions; square and multiply are exact integer arithmetic either way, and the oracle gets the same rows through ct_from_ntt"""
    k = len(q)
    pl = rng.integers(0, T, size=(2, n), dtype=np.uint64)
    fresh = O.encrypt_many(pk, pl, 700)
    full = np.zeros((3, 2, k, n), dtype=np.uint64)
    full[0] = (np.array(q, dtype=np.uint64) - np.uint64(1))[None, :, None]
    full[1] = 1
    full[2] = rand_rows(rng, q, (2,), n)
    coeff = np.concatenate([fresh, np.stack([O.ct_from_ntt(c) for c in full])])
    ntt = np.concatenate([np.stack([O.ct_to_ntt(c) for c in fresh]), full])
    return np.ascontiguousarray(coeff), np.ascontiguousarray(ntt)


@pytest.mark.parametrize("n,cls", pairs(FUSED_RINGS))
def test_fused_forms(n, cls):
    """every entry point that hands the row transform a prologue, a fused product or an addend, five ciphertexts each, bit for bit against the oracle (the
    ciphertext product of two different operands: against the Python-integer model)"""
    ca, q, E, O = engines(n, cls)
    k = len(q)
    rng = np.random.default_rng(7 * n + CLASSES[cls][1])
    sk, pk = O.keygen(21)
    evk = O.gen_evk(22, sk)
    nb = CNT * 2 * k * n * 8
    xc, xn = operand_arrays(E, O, q, n, pk, rng)

    # multiply_plain, one plaintext per group of two ciphertexts (FMA 2 in the wave-local kernel, transform + product elsewhere)
    pl = rng.integers(0, T, size=(3, n), dtype=np.uint64)
    pl[1, 1:] = 0; pl[1, 0] = T - 1
    d_w = E.alloc(3 * k * n * 8); E.plain_to_ntt(E.upload(pl), 3, d_w)
    d = E.upload(xc); E.multiply_plain(d, d_w, CNT, 2)
    want = np.stack([O.multiply_plain(xc[i], pl[i // 2]) for i in range(CNT)])
    assert np.array_equal(E.download(d, xc.shape), want), "multiply_plain"

    # the device encryptors, both result forms (FMA 1 and FMA 3 in the wave-local kernel; crc_ntt_fwd, k_ntt_ct_poly0 and a product pass elsewhere)
    key = bytes(range(3, 35))
    msgs = rng.integers(0, T, size=(CNT, n), dtype=np.uint64)
    msgs[0] = 0; msgs[1] = T - 1
    d_pl, d_ct = E.upload(msgs), E.alloc(nb)
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    d_ew = E.alloc(max(E.encrypt_dev_work_bytes(CNT), E.encrypt_sym_dev_work_bytes(CNT)))
    got = {}
    for form in (ca.COEFF, ca.NTT):
        E.L.crc_memset(E.c, E.p(d_ct), 0xff, nb, E.stream)
        E.encrypt_dev_key_forms(d_pk, d_pl, CNT, key, 1 << 33, form, d_ct, d_ew)
        got[form] = E.download(d_ct, xc.shape)
    assert np.array_equal(np.stack([O.decrypt(sk, c) for c in got[ca.COEFF]]), msgs), "encrypt_dev: the oracle's decryption"
    assert np.array_equal(got[ca.NTT], np.stack([O.ct_to_ntt(c) for c in got[ca.COEFF]])), "encrypt_dev: NTT form"
    for form in (ca.COEFF, ca.NTT):
        E.L.crc_memset(E.c, E.p(d_ct), 0xff, nb, E.stream)
        E.encrypt_sym_dev_key_forms(d_sk, d_pl, CNT, key, 1 << 34, form, d_ct, d_ew)
        got[form] = E.download(d_ct, xc.shape)
        assert np.array_equal(got[form], E.encrypt_sym(sk, msgs, 0, out_form=form, key=key, stream_base=1 << 34)), ("encrypt_sym_dev: the host twin", form)
    assert np.array_equal(np.stack([O.decrypt(sk, c) for c in got[ca.COEFF]]), msgs), "encrypt_sym_dev: the oracle's decryption"
    assert np.array_equal(got[ca.NTT], np.stack([O.ct_to_ntt(c) for c in got[ca.COEFF]])), "encrypt_sym_dev: NTT form"

    # square + relinearisation, the four form combinations (prologues 3, 4, 5 and 6 of the row transform, k_ntt_ct_head_add, k_ntt_ct_addct)
    sq = O.square_layer(xc, evk, threads=4)
    sq_ntt = np.stack([O.ct_to_ntt(c) for c in sq])
    d_evk = E.upload(evk)
    d_xc, d_xn, d_y = E.upload(xc), E.upload(xn), E.alloc(nb)
    d_work = E.alloc(max(E.square_relin_work_bytes(CNT), E.multiply_relin_work_bytes(CNT)))
    for fin in (ca.COEFF, ca.NTT):
        for fout in (ca.COEFF, ca.NTT):
            E.L.crc_memset(E.c, E.p(d_y), 0xff, nb, E.stream)
            E.square_relin(d_xn if fin == ca.NTT else d_xc, CNT, d_evk, d_y, d_work, in_form=fin, out_form=fout)
            assert np.array_equal(E.download(d_y, xc.shape), sq_ntt if fout == ca.NTT else sq), ("square_relin", fin, fout)
    # ... and under keys of 32-bit digits: log2(n D 2^dbc q) is then past what the key switch over fp64 primes admits at every ring and class here, so the digits
    # go through the 64-bit row transform that cuts them out of the source word as it loads the row (prologue 3), which 16-bit digits reach for w60 only
    evk32 = O.gen_evk(23, sk, dbc=32)
    sq32 = O.square_layer(xc, evk32, dbc=32, threads=4)
    sq32_ntt = np.stack([O.ct_to_ntt(c) for c in sq32])
    d_evk32, d_work32 = E.upload(evk32), E.alloc(E.square_relin_work_bytes(CNT, 32))
    for f in (ca.COEFF, ca.NTT):
        E.L.crc_memset(E.c, E.p(d_y), 0xff, nb, E.stream)
        E.square_relin(d_xn if f == ca.NTT else d_xc, CNT, d_evk32, d_y, d_work32, dbc=32, in_form=f, out_form=f)
        assert np.array_equal(E.download(d_y, xc.shape), sq32_ntt if f == ca.NTT else sq32), ("square_relin, 32-bit digits", f)
    assert np.array_equal(E.download(d_xc, xc.shape), xc) and np.array_equal(E.download(d_xn, xc.shape), xn)

    # multiply + relinearisation of two such arrays: pair 0 (a fresh encryption x the full-range random rows) against the Python-integer model of Evaluator::multiply
    # and the oracle's relinearisation, pairs 1..4 (y_i = x_i) against the oracle's square
    yc, yn = xc.copy(), xn.copy()
    yc[0], yn[0] = xc[4], xn[4]
    mul = sq.copy()
    mul[0] = O.relinearize(MultiplyModel(O).multiply(xc[0], yc[0]), evk)
    mul_ntt = sq_ntt.copy(); mul_ntt[0] = O.ct_to_ntt(mul[0])
    d_yc, d_yn = E.upload(yc), E.upload(yn)
    for f in (ca.COEFF, ca.NTT):
        E.L.crc_memset(E.c, E.p(d_y), 0xff, nb, E.stream)
        E.multiply_relin(d_xn if f == ca.NTT else d_xc, d_yn if f == ca.NTT else d_yc, CNT, d_evk, d_y, d_work, in_form=f, out_form=f)
        assert np.array_equal(E.download(d_y, xc.shape), mul_ntt if f == ca.NTT else mul), ("multiply_relin", f)

    # a tiny convolution with bias, coefficient form in and out: the inverse transform's addend epilogue with add_group = P, add_mod = nf
    B, zd, xd, yd, xf, yf, nf = 2, 1, 3, 3, 2, 2, 3
    img = rng.integers(0, T, size=(B, zd, xd, yd, n), dtype=np.uint64)
    x = np.ascontiguousarray(E.encrypt(pk, img, 900))
    w = rng.normal(0, 0.4, size=(nf, zd, xf, yf)).astype(np.float32); b = rng.normal(0, 0.2, size=nf).astype(np.float32)
    wp, bp = O.encode_many(w), O.encode_many(b)
    d_cw = E.alloc(len(wp) * k * n * 8); d_cb = E.alloc(nf * k * n * 8)
    E.plain_to_ntt(E.upload(wp), len(wp), d_cw); E.plain_to_delta(E.upload(bp), nf, ca.COEFF, d_cb)
    d_cy = E.alloc(B * nf * 2 * 2 * 2 * k * n * 8)
    E.L.crc_memset(E.c, E.p(d_cy), 0xff, B * nf * 2 * 2 * 2 * k * n * 8, E.stream)
    E.conv2d(E.upload(x), d_cw, d_cb, B, zd, xd, yd, 1, 1, xf, yf, nf, ca.COEFF, ca.COEFF, d_cy, E.alloc(E.conv2d_work_bytes(B, zd, xd, yd, 1, 1, xf, yf, nf, ca.COEFF)))
    w_ntt = O.plains_to_ntt(wp.reshape(nf, zd, xf, yf, n))
    want = np.stack([O.conv(x[i], w_ntt, bp, 1, 1) for i in range(B)])
    assert np.array_equal(E.download(d_cy, want.shape), want), "conv2d"
    E.close()


# ------------------------------------------------------------------------------------------------------------------------------ n = 32768
def test_ring_32768_is_reported_unsupported():
    """a row of n = 32768 does not fit one workgroup's LDS image: crc_ntt_fwd / crc_ntt_inv answer CRC_ERR_UNSUPPORTED before anything reaches the runtime (no HIP
    error recorded), the buffer is untouched, and a transform on a context created afterwards is exact"""
    import crcnn_amd as ca
    from oracle import orc
    q = moduli("w55")
    assert all((p - 1) % 65536 == 0 for p in q)
    E = ca.Engine(32768, q, T, device=0)
    x = rand_rows(np.random.default_rng(1), q, (1, 2), 32768)
    d = E.upload(x)
    for name, fn in (("crc_ntt_fwd", E.L.crc_ntt_fwd), ("crc_ntt_inv", E.L.crc_ntt_inv)):
        assert fn(E.c, E.p(d), 1, 2, E.stream) == UNSUPPORTED, name
        assert E.L.crc_last_hip_error() == 0, name
    with pytest.raises(ca.binding.CrcError) as e:
        E.ntt_fwd(d, 1)
    assert e.value.status == UNSUPPORTED
    assert np.array_equal(E.download(d, x.shape), x)
    E.close()
    n = 4096
    E = ca.Engine(n, q, T, device=0); O = orc.Oracle(n, q, T)
    x = rand_rows(np.random.default_rng(2), q, (3, 2), n)
    d = E.upload(x); E.ntt_fwd(d, 3)
    assert np.array_equal(E.download(d, x.shape), np.stack([O.ct_to_ntt(c) for c in x]))
    E.ntt_inv(d, 3)
    assert np.array_equal(E.download(d, x.shape), x)
    E.close()
