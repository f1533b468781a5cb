"""Noise flooding on the host: crc_flood (the host twin, any context) against tests/flood_model.py bit for bit at the word boundaries of the flood width, the
flooded ciphertext's plaintext and budget against the two derived bounds, crc_flood_bits / crc_flood_budget_bound against the model, the refusals, the law of
e1, and the kernels' own text on the CPU under sanitizers against that twin.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import flood_model as fm
import mod_switch_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
COEFF, NTT = 0, 1
T = 65537
FILL = 0xabababababababab
WIDTHS = (1, 31, 32, 63, 64, 65)            # and the largest admissible: the word boundaries of x are where a reduction goes wrong


def engine(n, k, t=T):
    import crcnn_amd as ca
    q = (ca.default_coeff_modulus_128(n) + [p for p in ca.default_coeff_modulus_128(8192) if p not in ca.default_coeff_modulus_128(n)])[:k] if n >= 2048 \
        else ca.default_coeff_modulus_128(8192)[:k]
    return ca.Engine(n, q, t, device=-1), [int(v) for v in q]


def largest_bits(E):
    return max(B for B in range(1, 127) if E.flood_supported(B))


def tensor(q, n, count, seed):
    rng = np.random.RandomState(seed)
    x = np.stack([(rng.randint(0, 1 << 62, size=(count, 2, n), dtype=np.int64) % qi).astype(np.uint64) for qi in q], axis=2)
    x[0] = 0
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("n,k", [(256, 2), (2048, 1), (4096, 2)], ids=["n256_k2", "n2048_k1", "n4096_k2"])
def test_host_twin_equals_the_model(n, k):
    """every width of WIDTHS that the parameters admit (one 54-bit modulus admits none above 35: those are refused, which is asserted) and the largest"""
    E, q = engine(n, k)
    _, pk = E.keygen(3)
    top = largest_bits(E)
    assert fm.admissible(q, T, n, top) and not fm.admissible(q, T, n, top + 1)
    x = tensor(q, n, 3, n + k)
    ran = 0
    for B in WIDTHS + (top,):
        assert E.flood_supported(B) == fm.admissible(q, T, n, B)
        if not E.flood_supported(B):
            continue
        for form in (COEFF, NTT):
            got = E.flood(pk, x, B, form=form, seed=40 + B)
            assert np.array_equal(got, fm.flood(E, pk, x, form, B, fm.seed_key(40 + B))), (n, k, B, form)
            ran += 1
    assert ran >= 8
    # the key form names its streams stream_base + m, across the 32-bit boundary of the first nonce word
    key = bytes(range(32)); base = (1 << 32) - 1
    got = E.flood(pk, x, top, form=NTT, key=key, stream_base=base)
    assert np.array_equal(got, fm.flood(E, pk, x, NTT, top, key, stream_base=base))
    E.close()


@pytest.mark.parametrize("n,k", [(256, 2), (4096, 2)], ids=["n256_k2", "n4096_k2"])
def test_flooded_ciphertexts_decrypt_with_a_budget_inside_both_bounds(n, k):
    E, q = engine(n, k)
    sk, pk = E.keygen(21)
    rng = np.random.RandomState(n)
    plains = rng.randint(0, T, size=(3, n)).astype(np.uint64)
    cts = E.encrypt(pk, plains, 77)
    b_in = min(E.noise_budget(sk, c) for c in cts)
    top = largest_bits(E)
    uppers = 0
    for B in (1, 40, 64, top - 1, top):
        out = E.flood(pk, cts, B, seed=5 + B)
        assert np.array_equal(E.decrypt(sk, out), plains), B
        lo, hi = fm.budget_lower(b_in, T, n, q, B), fm.budget_upper(b_in, T, n, q, B)
        assert lo == E.flood_budget_bound(b_in, B)
        for i in range(3):
            b = E.noise_budget(sk, out[i])
            print(f"n={n} B={B}: budget {b_in} -> {b}, derived [{lo} - 2, {hi}]")
            assert b >= lo - 2, (B, b, lo)
            if hi is not None:
                assert b <= hi, (B, b, hi); uppers += 1
    assert uppers >= 9                                                # the upper bound applied at every width far above the fresh noise
    E.close()


def test_a_flood_survives_a_modulus_switch_inside_both_bounds():
    """(4096, 3 -> 2), a flood of 100 bits: divided by the dropped prime it is still far above the switch's rounding term, so the budget after the switch has a
    derived upper bound as well as a lower one (flood_model.budget_upper_after_switch) -- a switch that loses the flood would show"""
    n, B = 4096, 100
    E, q = engine(n, 3)
    L = E.level(2)
    sk, pk = E.keygen(21)
    plains = np.random.RandomState(3).randint(0, T, size=(2, n)).astype(np.uint64)
    cts = E.encrypt(pk, plains, 78)
    b_in = min(E.noise_budget(sk, c) for c in cts)
    low = E.mod_switch(L, E.flood(pk, cts, B, seed=6))
    skL = np.ascontiguousarray(sk[:2])
    assert np.array_equal(L.decrypt(skL, low), plains)
    lo = mm.budget_bound(fm.budget_lower(b_in, T, n, q, B) - 1, T, n, mm.product(q[:2]))
    hi = fm.budget_upper_after_switch(b_in, T, n, q, B, 2)
    for c in low:
        b = L.noise_budget(skL, c)
        print(f"budget {b_in} -> flood of {B} bits -> switch 3 -> 2: {b}, derived [{lo} - 2, {hi}]")
        assert hi is not None and 0 < lo - 2 <= b <= hi
    E.close(); L.close()


def test_flood_bits_and_budget_bound_equal_the_model():
    for n, k, t in ((256, 2, T), (2048, 1, T), (4096, 2, T), (4096, 2, 1 << 20), (8192, 3, 12289 * 4 + 1)):
        E, q = engine(n, k, t)
        Lq = mm.product(q).bit_length()
        assert not E.flood_supported(0) and not E.flood_supported(127) and not E.flood_supported(-3)
        for b in list(range(0, Lq + 1, 7)) + [Lq]:
            for lam in (0, 1, 20, 40, 64, 100, 126):
                want = fm.flood_bits(q, t, n, b, lam)
                got = E.L.crc_flood_bits(E.c, b, lam)
                assert got == (want if want is not None else INVALID), (n, k, t, b, lam, got, want)
                if want is not None:
                    # the smallest: one bit less no longer covers the cap by lam bits (or is not a width at all)
                    W = fm.noise_cap(q, t, b)
                    assert want == lam + W.bit_length() and (W == 0 or (1 << (want - 1)) <= (W << lam))
            for B in (1, 17, 40, 64, 65, 90, 126):
                got = E.L.crc_flood_budget_bound(E.c, b, B)
                assert got == (fm.budget_lower(b, t, n, q, B) if fm.admissible(q, t, n, B) else INVALID), (n, k, t, b, B)
        assert E.L.crc_flood_bits(E.c, -1, 40) == INVALID and E.L.crc_flood_bits(E.c, Lq + 1, 40) == INVALID and E.L.crc_flood_bits(E.c, 10, -1) == INVALID
        assert E.L.crc_flood_budget_bound(E.c, -1, 10) == INVALID and E.L.crc_flood_bits(None, 10, 10) == INVALID
        E.close()


def test_refusals_leave_the_buffer_untouched():
    import crcnn_amd as ca
    n = 256
    E, q = engine(n, 2)
    _, pk = E.keygen(3)
    x = np.full((3, 2, 2, n), FILL, dtype=np.uint64)
    PU = ca.binding.PU
    px, pp = x.ctypes.data_as(PU), pk.ctypes.data_as(PU)
    top = largest_bits(E)
    for B in (0, 127, top + 1, -1):                                   # B = 0, B = 127, a B past t (2^B + 38 n) < q / 2
        for form in (COEFF, NTT):
            assert E.L.crc_flood(E.c, pp, px, 3, form, B, 1) == INVALID, (B, form)
    for form in (2, 3, 4, 5, 6, -1):                                  # the packed and limb forms
        assert E.L.crc_flood(E.c, pp, px, 3, form, 40, 1) == UNSUPPORTED and E.flood_dev_work_bytes(3, form) == 0
    assert E.L.crc_flood(None, pp, px, 3, COEFF, 40, 1) == INVALID and E.L.crc_flood(E.c, None, px, 3, COEFF, 40, 1) == INVALID
    assert E.L.crc_flood(E.c, pp, None, 3, COEFF, 40, 1) == INVALID and E.L.crc_flood_key(E.c, pp, px, 3, COEFF, 40, None, 0) == INVALID
    assert E.L.crc_flood(E.c, px, px, 3, COEFF, 40, 1) == INVALID     # the key inside the tensor
    assert E.L.crc_flood_dev(E.c, None, None, 3, COEFF, 40, 1, None, None) == INVALID          # a host-only context has no device entry points
    assert E.L.crc_flood(E.c, pp, px, 0, COEFF, 40, 1) == 0           # count = 0 is OK
    assert E.L.crc_flood(E.c, None, None, 0, 5, 0, 1) == 0 and E.L.crc_flood(None, pp, px, 0, COEFF, 40, 1) == INVALID     # ... whatever else is passed, on a context
    assert (x == np.uint64(FILL)).all()
    assert E.flood_dev_work_bytes(5, COEFF) == E.flood_dev_work_bytes(5, NTT) == 256 + 5 * 3 * 2 * n * 8
    E.close()


def test_two_stream_bases_differ_in_every_ciphertext():
    E, q = engine(256, 2)
    _, pk = E.keygen(3)
    x = tensor(q, 256, 4, 9)
    key = bytes(range(32))
    a = E.flood(pk, x, 50, key=key, stream_base=0); b = E.flood(pk, x, 50, key=key, stream_base=4); c = E.flood(pk, x, 50, key=key, stream_base=1)
    for m in range(4):
        assert not np.array_equal(a[m], b[m]) and not np.array_equal(a[m, 1], b[m, 1]) and not np.array_equal(a[m], x[m])
    # overlapping ranges of stream ids reuse streams: ciphertext m + 1 at base 0 has the flood of ciphertext m at base 1 (why a server advances by count)
    for m in range(3):
        for i, qi in enumerate(q):
            da = (a[m + 1, :, i].astype(object) - x[m + 1, :, i].astype(object)) % qi
            dc = (c[m, :, i].astype(object) - x[m, :, i].astype(object)) % qi
            assert (da == dc).all()
    E.close()


CHI2_511_Q999 = 615.5149            # the 0.999 quantile of the chi-square law with 511 degrees of freedom


def test_the_law_of_e1():
    """w = e1 - e_pk u + e2 s recovered with the secret key from the twin's flood of all-zero ciphertexts (16 x 4096 = 2^16 coefficients), binned into 512 cells of
    [-2^B, 2^B): the chi-square statistic is below the 0.999 quantile.  B = 64, so the 38 n < 2^18 of small terms moves a coefficient across a cell edge a
    2^18 / 2^55 share of the time.  The seed is fixed, so this is one deterministic outcome: seed 2024 is one for which the MODEL's e1 (straight from the
    keystream, no ciphertext involved) passes, which the test asserts first"""
    n, count, B, seed = 4096, 16, 64, 2024
    E, q = engine(n, 2)
    sk, pk = E.keygen(21)
    Tn = E.encrypt_dev_noise_thresholds()
    e1_all = []
    for m in range(count):
        e1_all += fm.samples(fm.raw_blocks(E, fm.seed_key(seed), m, n), B, Tn)[1]
    stat_model, _ = fm.chi_square_cells(e1_all, B)
    print(f"chi-square of the model's e1: {stat_model:.1f}")
    assert stat_model < CHI2_511_Q999
    out = E.flood(pk, np.zeros((count, 2, 2, n), dtype=np.uint64), B, form=NTT, seed=seed)
    irp2 = [E.table(f"inv_root_powers_div_two:{i}") for i in range(2)]
    Q = mm.product(q)
    ws = []
    for m in range(count):
        rows = []
        for i, qi in enumerate(q):
            v = [(int(a) + int(b) * int(s)) % qi for a, b, s in zip(out[m, 0, i], out[m, 1, i], sk[i])]       # c0 + c1 s, pointwise in NTT form
            rows.append(mm.ntt_inv(v, irp2[i], qi))
        for s in range(n):
            w = mm.crt_compose([rows[0][s], rows[1][s]], q)
            ws.append(w - Q if w > Q // 2 else w)
    stat, counts = fm.chi_square_cells(ws, B)
    print(f"chi-square of the recovered w: {stat:.1f}; cells {min(counts)} .. {max(counts)} of {len(ws) // 512} expected")
    assert stat < CHI2_511_Q999
    assert max(abs(w - e) for w, e in zip(ws, e1_all)) <= 38 * n     # and w is the model's e1 up to the small terms
    E.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/flood_kernel_check.cpp: the bodies of the flood's kernels (csrc/flood_device.h) on the CPU, one thread per workgroup over each launch's whole
    grid, with the address and undefined-behaviour sanitizers, equal the host twin bit for bit in both forms on buffers of exactly the stated sizes -- every pass
    structure of the row transform (n = 64 .. 16384), lazy and strict butterflies, the folding and the generic 128-bit reduction, widths on both sides of the
    word boundaries.  A stand-alone program: nothing sanitised is loaded into Python"""
    import tempfile
    import crcnn_amd as ca
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "flood_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "flood_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    d = {n: ca.default_coeff_modulus_128(n) for n in (4096, 8192, 16384)}
    small = [0xffffe80001, 0xffffc40001, 0xffffffffffc0001]           # two 40-bit primes (generic Barrett) and a 60-bit one (strict butterflies)
    cases = [(64, 3, 1, small), (64, 3, 63, small), (128, 2, 64, small), (256, 3, 65, small), (256, 3, 120, small), (256, 3, 31, d[8192][:2]), (512, 2, 32, d[8192][:1]),
             (1024, 3, 90, d[8192][:2]), (2048, 3, 35, d[8192][:1]), (4096, 3, 90, d[4096]), (8192, 2, 126, d[8192][:3]), (16384, 2, 126, d[16384][:4])]
    for n, count, B, q in cases:
        out = subprocess.run([exe, str(n), str(count), str(B), str(1000 + n + B)] + [str(v) for v in q], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, count, B, q, out.stdout, out.stderr[-1500:])
        assert ("lazy=1" in out.stdout) == all(v < (1 << 57) for v in q)


def test_network_flood_bits_is_off_by_default_and_refused_widths_throw_before_any_launch():
    """what a CPU test can see of `Network::flood_bits = 0 leaves the launch sequence as it is`: the member defaults to 0 (forward() tests it before it calls
    floodImages), and floodImages refuses a tensor without a buffer before it touches the device.  tests/test_gpu_flood_cpp.py holds the output digests and the
    launch counts of a forward with flood_bits = 0 against the same network's before a flooded forward"""
    import tempfile
    d = tempfile.mkdtemp()
    src = os.path.join(d, "default.cpp")
    open(src, "w").write('#include "crcnn_host.h"\n#include <stdexcept>\n'
                         'int main() { Network net; if (net.flood_bits != 0) return 1; ciphertext3D none;\n'
                         '  try { floodImages(none, 40); } catch (const std::invalid_argument &) { return 0; } return 2; }\n')
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(d, "default")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "crcnn_amd", "host"), src, "-o", exe, "-L", lib, "-lcrcnn_host", "-lcrcnn_hip",
                           "-Wl,-rpath," + lib])
    assert subprocess.run([exe]).returncode == 0
