"""Encryption under the secret key on the device (crc_encrypt_sym_dev*_forms), the refresh that uses it (crc_refresh_sym_dev*) and the host classes' opt-in
(Network::reenc_symmetric, encryptImageSymmetric).  The device is pinned to the host twin bit for bit -- and the host twin to the oracle's decryptor and to the
sampling laws by tests/test_encrypt_sym_cpu.py; the refresh and the published configurations are checked against the oracle and the reference's goldens."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, sha
from test_encrypt_sym_cpu import IDS, _derived_budget, _moduli, param_sets
from test_gpu_host_cpp import DRIVER, PUBLISHED, _run_refresh_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,q,t", param_sets(), ids=IDS)
def test_device_encryptor_sym_equals_the_host_twin(n, q, t):
    """same seed / key and stream base, both result forms, dense plaintexts: the device's ciphertexts are the host twin's, bit for bit -- on rings with the
    wave-local transform (the product joins the transform's last loop) and without it (n = 1024, n = 256, 40- and 60-bit moduli: a pass of its own)"""
    import crcnn_amd as ca
    k = len(q)
    E = ca.Engine(n, q, t, device=0)
    sk, _ = E.keygen(11)
    rng = np.random.default_rng(5)
    big = max(24, (8 * 256 * 2048) // n)                     # >= 8 sampling workgroups (and 8 k row transforms) per CU of a 256-CU device
    d_sk = E.upload(sk)
    key = bytes(range(7, 39))
    for cnt in (1, 24, big):
        pl = rng.integers(0, t, size=(cnt, n), dtype=np.uint64)
        pl[0] = 0
        if cnt > 1: pl[1] = t - 1
        d_pl = E.upload(pl); d_ct = E.alloc(cnt * 2 * k * n * 8); d_w = E.alloc(E.encrypt_sym_dev_work_bytes(cnt))
        for form in (ca.NTT, ca.COEFF):
            E.L.crc_memset(E.c, E.p(d_ct), 0xff, cnt * 2 * k * n * 8, E.stream)
            E.encrypt_sym_dev_forms(d_sk, d_pl, cnt, 77 + cnt, form, d_ct, d_w)
            assert np.array_equal(E.download(d_ct, (cnt, 2, k, n)), E.encrypt_sym(sk, pl, 77 + cnt, out_form=form)), (cnt, form)
            E.encrypt_sym_dev_key_forms(d_sk, d_pl, cnt, key, 1 << 33, form, d_ct, d_w)
            assert np.array_equal(E.download(d_ct, (cnt, 2, k, n)), E.encrypt_sym(sk, pl, 0, out_form=form, key=key, stream_base=1 << 33)), (cnt, form, "key")
        assert np.array_equal(E.download(d_pl, (cnt, n)), pl)              # the plaintexts are not modified
    # the transform's tuning switch off: the two-pass form on a ring that has the wave-local kernel gives the same bits
    if n in (2048, 4096, 8192):
        pl = rng.integers(0, t, size=(24, n), dtype=np.uint64)
        d_pl = E.upload(pl); d_ct = E.alloc(24 * 2 * k * n * 8); d_w = E.alloc(E.encrypt_sym_dev_work_bytes(24))
        E.set_tuning("ntt_wave", 0)
        E.encrypt_sym_dev_forms(d_sk, d_pl, 24, 5, ca.NTT, d_ct, d_w)
        E.set_tuning("ntt_wave", -1)
        assert np.array_equal(E.download(d_ct, (24, 2, k, n)), E.encrypt_sym(sk, pl, 5, out_form=ca.NTT))
    E.close()


@pytest.mark.parametrize("n,k,t", [(4096, 2, 1 << 29), (2048, 1, 1 << 18), (8192, 3, 1 << 42)])
def test_device_refresh_sym(n, k, t):
    """crc_refresh_sym_dev on the mid-network inputs of test_device_refresh: the floats of crc_refresh_dev bit for bit, every output decrypts under the ORACLE to
    encode(float), the four form combinations give identical ciphertexts, in place, other seeds give other ciphertexts of the same plaintexts, and the budget
    is at least the derived bound (|m_c| <= 1 for encoder-made plaintexts) and at least the public-key refresh's"""
    import crcnn_amd as ca
    from oracle import orc
    q = _moduli(n, k)
    E = ca.Engine(n, q, t, device=0)
    O = orc.Oracle(n, q, t)
    sk, pk = E.keygen(31)
    rng = np.random.default_rng(9)
    cnt = 40
    vals = (rng.standard_normal(cnt) * 3).astype(np.float32)
    pl, _ = E.encode(vals)
    ct = E.encrypt(pk, pl, 5)
    w, _ = E.encode(np.float32([0.37]))
    d_ct = E.upload(ct); d_w = E.alloc(E.k * n * 8); E.plain_to_ntt(E.upload(w), 1, d_w)
    E.ntt_fwd(d_ct, cnt); E.multiply_plain_ntt(d_ct, d_w, cnt, cnt)
    E.ntt_inv(d_ct, cnt)
    ct = E.download(d_ct, (cnt, 2, k, n))
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    # the public-key refresh on the same input: its floats and its budgets
    d_in = E.upload(ct); d_out = E.alloc(cnt * 2 * k * n * 8); d_v = E.alloc(cnt * 4)
    E.refresh_dev(d_sk, d_pk, d_in, cnt, 123, d_out, E.alloc(E.refresh_dev_work_bytes(cnt, ca.COEFF)), d_values=d_v)
    pk_vals = E.download(d_v, (cnt,), dtype=np.float32)
    pk_out = E.download(d_out, (cnt, 2, k, n))
    want_plain, _ = E.encode(pk_vals)
    c = want_plain.astype(object); c = np.where(c > t // 2, t - c, c)
    assert int(c.max()) <= 1
    bound = _derived_budget(q, t, 1)
    outs = {}
    for in_form in (ca.COEFF, ca.NTT):
        d_in = E.upload(ct)
        if in_form == ca.NTT: E.ntt_fwd(d_in, cnt)
        for out_form in (ca.COEFF, ca.NTT):
            d_out = E.alloc(cnt * 2 * k * n * 8); d_v = E.alloc(cnt * 4)
            d_work = E.alloc(E.refresh_sym_dev_work_bytes(cnt, in_form))
            E.refresh_sym_dev(d_sk, d_in, cnt, 123, d_out, d_work, in_form=in_form, out_form=out_form, d_values=d_v)
            got_vals = E.download(d_v, (cnt,), dtype=np.float32)
            assert np.array_equal(got_vals.view(np.uint32), pk_vals.view(np.uint32))
            if out_form == ca.NTT: E.ntt_inv(d_out, cnt)
            r = E.download(d_out, (cnt, 2, k, n))
            assert np.array_equal(np.stack([O.decrypt(sk, r[i]) for i in range(cnt)]), want_plain)
            outs[(in_form, out_form)] = r
    r = outs[(ca.COEFF, ca.COEFF)]
    assert all(np.array_equal(v, r) for v in outs.values())
    # ... and they are what the host twin makes of the same plaintexts under the same seed
    assert np.array_equal(r, E.encrypt_sym(sk, want_plain, 123))
    b_sym = [O.noise_budget(sk, r[i]) for i in range(cnt)]; b_pk = [O.noise_budget(sk, pk_out[i]) for i in range(cnt)]
    print("refresh budgets", (n, k), "derived bound", bound, "symmetric", min(b_sym), max(b_sym), "public-key", min(b_pk), max(b_pk))
    assert min(b_sym) >= bound and all(s >= p for s, p in zip(b_sym, b_pk)), (bound, b_sym, b_pk)
    d_in = E.upload(ct); d_work = E.alloc(E.refresh_sym_dev_work_bytes(cnt, ca.COEFF))
    E.refresh_sym_dev(d_sk, d_in, cnt, 124, d_in, d_work)                  # in place, another seed, no values wanted
    r2 = E.download(d_in, (cnt, 2, k, n))
    assert not np.array_equal(r2[:, 1], r[:, 1])
    assert np.array_equal(np.stack([O.decrypt(sk, r2[i]) for i in range(cnt)]), want_plain)
    d_in = E.upload(ct); E.ntt_fwd(d_in, cnt)
    E.refresh_sym_dev(d_sk, d_in, cnt, 124, d_in, E.alloc(E.refresh_sym_dev_work_bytes(cnt, ca.NTT)), in_form=ca.NTT, out_form=ca.NTT)     # in place, NTT-resident
    E.ntt_inv(d_in, cnt)
    assert np.array_equal(E.download(d_in, (cnt, 2, k, n)), r2)
    key = E.random_key()
    E.refresh_sym_dev(d_sk, E.upload(ct), cnt, 0, d_in, d_work, key=key, stream_base=77)
    r3 = E.download(d_in, (cnt, 2, k, n))
    assert np.array_equal(np.stack([O.decrypt(sk, r3[i]) for i in range(cnt)]), want_plain)
    assert np.array_equal(r3, E.encrypt_sym(sk, want_plain, 0, key=key, stream_base=77))
    E.close()


@pytest.mark.parametrize("name", PUBLISHED)
@pytest.mark.parametrize("case", ["unfused", "fused-batch", "fused-chunked"])
def test_cpp_published_configurations_with_symmetric_refresh(name, case):
    """test_cpp_published_configurations_with_refresh with Network::reenc_symmetric (`netr ... sym`), against the REFERENCE's goldens: the floats the client
    sees at the refresh bit for bit, the decrypted outputs polynomial for polynomial, and at least the reference's remaining budget less the existing test's
    margin of 2 (the lower side only: less noise than the reference is the point).  Without the argument the driver runs as before."""
    import shutil
    batch, fuse, chunk = {"unfused": (1, False, 0), "fused-batch": (5, True, 0), "fused-chunked": (5, True, 2)}[case]
    g, d = _run_refresh_config(name, batch, fuse, chunk)                    # no argument: the public-key refresh, as today
    bud_pk = np.fromfile(os.path.join(d, "budget.u64"), dtype=np.uint64).reshape(batch, 10)
    assert int(bud_pk.min()) >= min(g["budget"]) - 2 and int(bud_pk.max()) <= max(g["budget"]) + 2, (bud_pk, g["budget"])
    h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
    out = subprocess.run([DRIVER, "netr", g["model"], h5, d, str(batch), str(g["layer_before_reenc"]), "1" if fuse else "0", str(chunk), "sym"],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "netr ok" in out.stdout, out.stderr[-2000:]
    n = g["n"]
    want_fl = np.array(g["reenc_floats_bits"], dtype=np.uint32)
    fl = np.fromfile(os.path.join(d, "reenc_floats.f32"), dtype=np.uint32).reshape(batch, -1)
    assert all(np.array_equal(fl[b], want_fl) for b in range(batch))
    want_dec = np.load(os.path.join(GOLD, f"net_{name}_dec.npz"))["dec"]
    dec = np.fromfile(os.path.join(d, "dec.u64"), dtype=np.uint64).reshape(batch, 10, n)
    assert sha(want_dec) == g["dec_sha256"]
    assert all(np.array_equal(dec[b], want_dec) for b in range(batch))
    bud = np.fromfile(os.path.join(d, "budget.u64"), dtype=np.uint64).reshape(batch, 10)
    print("budgets", name, case, "symmetric", int(bud.min()), int(bud.max()), "public-key", int(bud_pk.min()), int(bud_pk.max()), "reference", g["budget"])
    assert int(bud.min()) >= min(g["budget"]) - 2, (bud, g["budget"])
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("n,t", [(2048, 1 << 18), (4096, 1 << 29)])
def test_cpp_encrypt_image_symmetric(n, t):
    """encryptImageSymmetric on a batch, both result forms: the plaintexts and floats encryptImage's ciphertexts decrypt to, image by image"""
    out = subprocess.run([DRIVER, "encsym", str(n), str(t)], capture_output=True, text=True)
    assert out.returncode == 0 and "encsym ok" in out.stdout, out.stderr[-2000:]


def test_cpp_budget_checking_forward_with_symmetric_refresh():
    """Network::reenc_symmetric in the budget-checking forward (max_num_of_reencryptions >= 0): three Square layers exhaust the budget, the forward refreshes under
    the secret key alone (the public key is taken away: a public-key refresh would throw), and gives the public-key mode's values with no more refreshes"""
    out = subprocess.run([DRIVER, "budgetsym"], capture_output=True, text=True)
    assert out.returncode == 0 and "budgetsym ok" in out.stdout, out.stderr[-2000:]
    print(out.stderr.strip().splitlines()[-1])
