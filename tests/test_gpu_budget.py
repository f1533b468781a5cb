"""The device noise-budget path (crc_noise_budget_dev, kernels_budget.hip) on the GPU: against the numbers SEAL 2.3.1 itself reported (tests/golden/ops_*.npz),
against the CPU oracle at the bench ring sizes -- fresh encryptions, a squared and relinearised ciphertext, and ciphertexts constructed so that t v mod q sits
at and next to every 64-bit word boundary of the kernel's accumulator, on both sides of the centring --, and through the C++ host classes (budget_host)."""
import glob
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_HOST = os.path.join(ROOT, "crcnn_amd", "lib", "budget_host")
SETS = sorted(glob.glob(os.path.join(GOLD, "ops_*.npz")))


def device_budgets(E, d_sk, cts, form, with_min=True):
    """budgets of cts [count][size][k][n] (coefficient form on the host; transformed on the device first for form = NTT) and the {min, index} pair"""
    import crcnn_amd as ca
    cts = np.ascontiguousarray(cts)
    count, size = cts.shape[0], cts.shape[1]
    d_ct = E.upload(cts)
    if form == ca.NTT:
        E.ntt_fwd(d_ct, count, size)
    d_bits = E.alloc(4 * count); d_min = E.alloc(8)
    d_work = E.alloc(E.noise_budget_dev_work_bytes(count, size, form))
    E.noise_budget_dev(d_sk, d_ct, count, d_bits, d_work, size=size, in_form=form, d_min=d_min if with_min else None)
    bits = E.download(d_bits, (count,), dtype=np.int32)
    pair = E.download(d_min, (2,), dtype=np.int32) if with_min else None
    return [int(b) for b in bits], pair


def check_min(bits, pair):
    assert int(pair[0]) == min(bits) and int(pair[1]) == bits.index(min(bits)), (bits, pair)


def test_six_golden_sets_present():
    assert len(SETS) == 6, SETS


@pytest.mark.parametrize("path", SETS, ids=[os.path.basename(p)[:-4] for p in SETS])
def test_budgets_are_seals_own(path):
    import crcnn_amd as ca
    from oracle import orc
    g = dict(np.load(path))
    q = [int(v) for v in g["q"]]
    E = ca.Engine(int(g["n"]), q, int(g["t"]), device=0)
    try:
        O = orc.Oracle(int(g["n"]), q, int(g["t"]))
        d_sk = E.upload(g["sk"])
        for form in (ca.COEFF, ca.NTT):
            bits, pair = device_budgets(E, d_sk, g["ct_in"], form)
            assert bits == [int(b) for b in g["ref_budget_in"]], (form, bits)
            check_min(bits, pair)
            bits, pair = device_budgets(E, d_sk, g["ref_relin"], form)
            assert bits == [int(b) for b in g["ref_budget_relin"]], (form, bits)
            check_min(bits, pair)
            # size 3: SEAL's own squared ciphertexts, expected value from the oracle
            bits, pair = device_budgets(E, d_sk, g["ref_sq"], form)
            assert bits == [O.noise_budget(g["sk"], c) for c in g["ref_sq"]], (form, bits)
            check_min(bits, pair)
        # no d_min asked for, and an empty call
        bits, _ = device_budgets(E, d_sk, g["ct_in"], ca.COEFF, with_min=False)
        assert bits == [int(b) for b in g["ref_budget_in"]]
        d = E.alloc(64)
        E.noise_budget_dev(d_sk, d, 0, d, d, d_min=d)
    finally:
        E.close()


def boundary_ciphertexts(q, t, n):
    """c1 = 0, c0 = target t^-1 mod q at coefficient (7 j) mod n: t v mod q = target, for j at and next to every multiple of 64 below the bit count of q"""
    Q = 1
    for p in q:
        Q *= p
    total_bits, tinv = Q.bit_length(), pow(t, -1, Q)
    js = sorted({j for m in range(0, total_bits + 64, 64) for j in (m - 1, m, m + 1) if 0 <= j < total_bits})
    cts, want = [], []
    for j in js:
        for target in ((1 << j) - 1, 1 << j, Q - (1 << j), Q - ((1 << j) - 1)):
            target %= Q
            x = target * tinv % Q
            ct = np.zeros((2, len(q), n), dtype=np.uint64)
            ct[0, :, (7 * j) % n] = [x % p for p in q]
            cts.append(ct)
            want.append(max(0, total_bits - min(target, Q - target).bit_length() - 1))
    return cts, want


@pytest.mark.parametrize("n, k, t", [(4096, 2, 1 << 32), (8192, 3, 1 << 42), (16384, 4, 1 << 44), (16384, 8, 1 << 44)])
def test_budgets_match_oracle_at_bench_ring_sizes(n, k, t):
    """67 ciphertexts (131 with all eight primes, where the boundary cases alone are 80): not a multiple of the wave, of the workgroup or of any tile.  The
    constructed ones come first and last, so the minimum (budget 0 at t v = q/2 + ...) is not at index 0"""
    import crcnn_amd as ca
    from oracle import orc
    q = [int(p) for p in ca.default_coeff_modulus_128(n)[:k]]
    O = orc.Oracle(n, q, t)
    sk, pk = O.keygen(31 + k)
    evk = O.gen_evk(32 + k, sk)
    bcts, bwant = boundary_ciphertexts(q, t, n)
    count = 67 if len(bcts) + 2 <= 67 else 131
    assert len(bcts) + 2 <= count
    rng = np.random.RandomState(5 + k)
    fresh = O.encrypt_many(pk, O.encode_many(rng.uniform(-2, 2, size=count - len(bcts) - 1)), 900)
    squared = O.relinearize(O.square(fresh[0]), evk)
    half = len(bcts) // 2
    cts = np.ascontiguousarray(np.stack(list(fresh[:1]) + bcts[:half] + [squared] + list(fresh[1:]) + bcts[half:]))
    assert cts.shape[0] == count
    want = [O.noise_budget(sk, c) for c in cts]
    # the oracle agrees with the big-integer value of every constructed case
    assert want[1:1 + half] == bwant[:half] and want[count - (len(bcts) - half):] == bwant[half:]
    E = ca.Engine(n, q, t, device=0)
    try:
        d_sk = E.upload(sk)
        for form in (ca.COEFF, ca.NTT):
            bits, pair = device_budgets(E, d_sk, cts, form)
            wrong = [(i, bits[i], want[i]) for i in range(count) if bits[i] != want[i]]
            assert not wrong, (form, wrong[:10])
            check_min(bits, pair)
            assert int(pair[1]) != 0
        # the routine the CPU tests run is the kernel's: same answers from the host entry point on v = c0
        assert [int(b) for b in E.budget_bits_host(np.stack(bcts)[:, 0])] == bwant
    finally:
        E.close()


def _net_names():
    from test_gpu_nets import NAMES
    return NAMES


@pytest.mark.parametrize("name", _net_names())
def test_network_output_budgets_match_reference(name):
    """all ten output ciphertexts of image 0 against the budgets the compiled reference recorded, for every network golden tests/test_gpu_nets.py runs (that file
    checks three of the ten, with the oracle, at n >= 1024)"""
    import crcnn_amd as ca
    from test_gpu_nets import run_net
    g, O, sk, out, _ = run_net(name, resident=True, batch=2)
    E = ca.Engine(g["n"], g["q"], g["t"], device=0)
    try:
        d_sk = E.upload(sk)
        for form in (ca.COEFF, ca.NTT):
            bits, pair = device_budgets(E, d_sk, out[0].reshape(10, 2, E.k, E.n), form)
            assert bits == g["budget"], (name, form, bits)
            check_min(bits, pair)
    finally:
        E.close()


def test_argument_checks_on_the_device():
    """on a device context a valid call returns CRC_OK, so each refusal below is the entry point's own check (they return before anything is launched)"""
    import crcnn_amd as ca
    n, k = 1024, 2
    E = ca.Engine(n, [0x7fffffff380001, 0x3fffffff000001], 1 << 20, device=0)
    try:
        sk, pk = E.keygen(3)
        cts = np.ascontiguousarray(E.encrypt(pk, E.encode(np.array([0.5, -1.25], dtype=np.float32))[0], 9).reshape(2, 2, k, n))
        d_sk, d_ct, d_bits = E.upload(sk), E.upload(cts), E.alloc(8)
        d_work = E.alloc(E.noise_budget_dev_work_bytes(2, 3, ca.COEFF))
        call = lambda sk_, ct_, size, form, bits_, work_: E.L.crc_noise_budget_dev(E.c, E.p(sk_), E.p(ct_), 2, size, form, E.p(bits_), None, E.p(work_), E.stream)
        assert call(d_sk, d_ct, 2, ca.COEFF, d_bits, d_work) == 0
        E.sync()
        bad = -1                                                                # CRC_ERR_INVALID_ARGUMENT
        for size in (1, 4):
            assert call(d_sk, d_ct, size, ca.COEFF, d_bits, d_work) == bad, size
        for form in (ca.NTTP, ca.NTTL, ca.NTTL1, ca.NTTLC, 6, -1):
            assert call(d_sk, d_ct, 2, form, d_bits, d_work) == bad, form
        for hole in range(4):                                                   # a null pointer: key, ciphertexts, result, work
            a = [d_sk, d_ct, d_bits, d_work]; a[hole] = None
            assert call(a[0], a[1], 2, ca.COEFF, a[2], a[3]) == bad, hole
        for size, form in ((4, ca.COEFF), (2, ca.NTTL)):
            assert E.noise_budget_dev_work_bytes(2, size, form) == 0
        assert [int(b) for b in E.download(d_bits, (2,), dtype=np.int32)] == [E.noise_budget(sk, c) for c in cts]
    finally:
        E.close()


def run_budget_host(t, batch=16, n=4096, k=2, seed=77, model="PlainModelTiny"):
    d = tempfile.mkdtemp()
    h5 = os.path.join(GOLD, "models", model + ".h5")
    out = subprocess.run([BUDGET_HOST, h5, str(n), str(k), str(t), str(batch), str(seed), d], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.load(open(os.path.join(d, f"budget_{model}_n{n}_k{k}_b{batch}.json")))


def check_profile(r, layers, batch):
    L = len(r["layers"])
    assert L == layers and len(r["layer_budget_min"]) == L and len(r["layer_budget_first"]) == L
    assert int(np.prod(r["output_shape"])) == 10 * batch and len(r["output_budgets"]) == 10 * batch
    assert all(b >= 0 for b in r["layer_budget_min"] + r["layer_budget_first"])            # coefficient form between the layers: everything measured
    # ciphertext 0 of every layer: the host routine's number
    assert r["layer_budget_first"] == r["layer_budget_host_first"], r
    assert all(m <= f for m, f in zip(r["layer_budget_min"], r["layer_budget_first"])), r
    # the whole-tensor calls agree with each other and with the last layer's profile
    assert r["output_min"] == min(r["output_budgets"]) == r["layer_budget_min"][-1]
    assert r["output_min_index"] == r["output_budgets"].index(r["output_min"])
    assert r["output_budgets"][0] == r["layer_budget_first"][-1]
    # the NTT-resident forward: the same output bits, the same numbers wherever a tensor was in a ciphertext form
    assert r["resident_output_identical"] is True
    for a, b in ((r["layer_budget_resident_min"], r["layer_budget_min"]), (r["layer_budget_resident_first"], r["layer_budget_first"])):
        assert len(a) == L and all(x == -1 or x == y for x, y in zip(a, b)), (a, b)
    assert r["layer_budget_resident_min"][-1] == r["layer_budget_min"][-1]


def test_budget_host_profiles_a_batch():
    """PlainModelTiny at (4096, 2, t = 2^32), 16 images: one minimum and one first budget per layer, 160 output budgets"""
    check_profile(run_budget_host(1 << 32), layers=6, batch=16)


def test_budget_profile_falls_across_the_square_layer():
    """PlainModelTiny has no Square layer; ApproxPlainModel (conv, pool, batch norm, conv, Square, pool, batch norm, fc, fc) at (4096, 2, t = 2^29), 4 images: the same checks, and the
    first ciphertext's budget does not rise across the Square layer"""
    r = run_budget_host(1 << 29, batch=4, model="ApproxPlainModel")
    check_profile(r, layers=len(r["layers"]), batch=4)
    squares = [i for i, nm in enumerate(r["layers"]) if nm.startswith("act")]
    assert len(squares) == 1 and squares[0] > 0, r["layers"]
    for i in squares:
        assert r["layer_budget_first"][i] <= r["layer_budget_first"][i - 1], r["layer_budget_first"]
        assert r["layer_budget_min"][i] <= r["layer_budget_min"][i - 1], r["layer_budget_min"]


def test_budget_scope_and_the_ciphertext_scope_0_cannot_see():
    """ample budget (t = 2^20): the budget-checking forward gives the same bits in both scopes and refreshes nothing; an exhausted ciphertext at index 5 is found by
    minNoiseBudget while noiseBudget(t) -- ciphertext 0 -- is unchanged"""
    r = run_budget_host(1 << 20)
    s = r["scope"]
    assert s["refreshed_values"] == [0, 0], s
    assert s["identical"] is True and s["same_as_plain_forward"] is True, s
    assert s["exhausted_index"] == 5 and s["min"] == 0 and s["where"] == 5, s
    assert s["noise_budget_before"] == s["noise_budget_after"] == r["output_budgets"][0] > 5, s
    # noiseBudgets / minNoiseBudget refuse the packed and limb forms
    assert r["packed_forms_rejected"] is True
    # PlainModulusSearch::whole_batch_budget: one candidate with each scope; with ample budget neither runs out, and they agree
    st = r["search_status"]
    assert st["first_ciphertext"] == st["whole_batch"] and st["whole_batch"] != 1, st
