"""Modulus switching on the host: the prefix context's tables, crc_mod_switch (the host twin, any contexts) against tests/mod_switch_model.py for every form
pair and both sizes, the refusals, decryption and noise budget across levels, and the kernels' own text on the CPU under sanitizers against that twin.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mod_switch_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
COEFF, NTT = 0, 1
# n = 256: the moduli of the ops_n256_* goldens -- two 40-bit primes and the 60-bit one (strict butterflies, p far above and far below q_i), and the 55/54-bit set
SMALL = [0xffffe80001, 0xffffc40001, 0xffffffffffc0001]
SMALL_R = [0xffffffffffc0001, 0xffffe80001, 0xffffc40001]
K3 = [0x7fffffff380001, 0x7ffffffef00001, 0x3fffffff000001]
T = 65537


def engines(n, q, kept, t=T):
    import crcnn_amd as ca
    A = ca.Engine(n, q, t, device=-1)
    return A, A.level(kept)


def edge_cts(q, n, count, size, seed):
    """random canonical residues; ciphertext 0: polynomial 0 all zero, polynomial 1 every residue q_i - 1 (composes to q - 1, which rounds to q_to = 0); ciphertext 1,
    polynomial 0: the last residue runs over {0, h, h + 1, p - 1 - h, p - 1}"""
    rng = np.random.RandomState(seed)
    k = len(q)
    x = np.zeros((count, size, k, n), dtype=np.uint64)
    for i, qi in enumerate(q):
        x[:, :, i, :] = (rng.randint(0, 1 << 62, size=(count, size, n), dtype=np.int64) % qi).astype(np.uint64)
    x[0, 0] = 0
    for i, qi in enumerate(q):
        x[0, 1, i, :] = qi - 1
    if count > 1:
        p = q[-1]; h = p >> 1
        x[1, 0, k - 1, :] = np.array([[0, h, h + 1, p - 1 - h, p - 1][s % 5] for s in range(n)], dtype=np.uint64)
    return x


def model_switch(A, B, x, in_form, out_form):
    """the model with the model's own transforms (on the contexts' tables) around it"""
    q = [int(v) for v in A.q]; kept = B.k
    rp = [A.table(f"root_powers:{i}") for i in range(A.k)]
    irp2 = [A.table(f"inv_root_powers_div_two:{i}") for i in range(A.k)]
    out = np.zeros(x.shape[:2] + (kept, A.n), dtype=np.uint64)
    for c in range(x.shape[0]):
        for p in range(x.shape[1]):
            rows = [[int(v) for v in x[c, p, i]] for i in range(A.k)]
            if in_form == NTT:
                rows = [mm.ntt_inv(rows[i], irp2[i], q[i]) for i in range(A.k)]
            got = mm.switch_rows(rows, q, kept)
            assert got == mm.switch_rows_residues(rows, q, kept) == mm.switch_rows_correction(rows, q, kept)
            if out_form == NTT:
                got = [mm.ntt_fwd(got[i], rp[i], q[i]) for i in range(kept)]
            out[c, p] = np.array(got, dtype=np.uint64)
    return out


def test_the_models_two_forms_agree_on_a_toy_ring():
    q = [97, 193, 257, 113]
    for kept in (1, 2, 3):
        rows = [[(7 * s + 3 * i) % q[i] for s in range(8)] for i in range(4)]
        rows[3][:5] = [0, 56, 57, 112 - 56, 112]
        for i in range(4):
            rows[i][7] = q[i] - 1
        a = mm.switch_rows(rows, q, kept)
        assert a == mm.switch_rows_residues(rows, q, kept) == mm.switch_rows_correction(rows, q, kept)
        assert [a[i][7] for i in range(kept)] == [0] * kept            # q - 1 rounds to q_to = 0
    # every integer of a small modulus: the residue forms are the iterated rounded division
    q = [17, 13, 11]
    Q = 17 * 13 * 11
    rows = [[c % qi for c in range(Q)] for qi in q]
    for kept in (1, 2):
        assert mm.switch_rows(rows, q, kept) == mm.switch_rows_residues(rows, q, kept) == mm.switch_rows_correction(rows, q, kept)


def test_a_prefix_context_has_the_full_contexts_tables():
    for n, q in ((256, SMALL), (256, K3), (1024, K3)):
        for kept in range(1, len(q)):
            A, B = engines(n, q, kept)
            assert A.mod_switch_supported(B) and not B.mod_switch_supported(A) and not A.mod_switch_supported(A)
            assert np.array_equal(B.table("root"), A.table("root")[:kept]) and np.array_equal(B.table("q"), A.table("q")[:kept])
            for i in range(kept):
                assert np.array_equal(B.table(f"root_powers:{i}"), A.table(f"root_powers:{i}"))
                assert np.array_equal(B.table(f"inv_root_powers_div_two:{i}"), A.table(f"inv_root_powers_div_two:{i}"))
            A.close(); B.close()


@pytest.mark.parametrize("q,kept", [(SMALL, 2), (SMALL, 1), (SMALL_R, 1), (K3, 2), (K3, 1), (SMALL[:2], 1)],
                         ids=["small_3to2", "small_3to1", "small_reversed_3to1", "k3_3to2", "k3_3to1", "small_2to1"])
def test_host_twin_equals_the_model(q, kept):
    n = 64
    A, B = engines(n, q, kept)
    for size in (2, 3):
        x = edge_cts(q, n, 2, size, 5 * size + kept)
        for in_form in (COEFF, NTT):
            for out_form in (COEFF, NTT):
                got = A.mod_switch(B, x, size=size, in_form=in_form, out_form=out_form)
                assert got.shape == (2, size, kept, n)
                assert np.array_equal(got, model_switch(A, B, x, in_form, out_form)), (q, kept, size, in_form, out_form)
        assert not A.mod_switch(B, x, size=size)[0, :2].any()          # zero stays zero, q - 1 rounds to q_to = 0
    A.close(); B.close()


def test_refusals_leave_the_output_untouched():
    import crcnn_amd as ca
    n = 64
    A, B = engines(n, K3, 2)
    x = edge_cts(K3, n, 2, 3, 1)
    out = np.full((2, 3, 2, n), 0xabababababababab, dtype=np.uint64)
    PU = ca.binding.PU
    px, po = x.ctypes.data_as(PU), out.ctypes.data_as(PU)
    call = A.L.crc_mod_switch
    others = {
        "not a prefix (other moduli)": ca.Engine(n, [K3[0], K3[2]], T, device=-1),
        "not a prefix (same order, another first modulus)": ca.Engine(n, K3[1:], T, device=-1),
        "not proper (all moduli)": ca.Engine(n, K3, T, device=-1),
        "another n": ca.Engine(2 * n, K3[:2], T, device=-1),
        "another t": ca.Engine(n, K3[:2], 1 << 16, device=-1),
    }
    for what, C in others.items():
        assert not A.mod_switch_supported(C), what
        assert call(A.c, C.c, px, COEFF, 2, 2, po, COEFF) == INVALID, what
        assert A.mod_switch_work_bytes(C, 2) == 0, what
        C.close()
    assert call(B.c, A.c, px, COEFF, 2, 2, po, COEFF) == INVALID                                  # the longer context is not a prefix of the shorter
    assert call(None, B.c, px, COEFF, 2, 2, po, COEFF) == INVALID and call(A.c, None, px, COEFF, 2, 2, po, COEFF) == INVALID
    assert call(A.c, B.c, None, COEFF, 2, 2, po, COEFF) == INVALID and call(A.c, B.c, px, COEFF, 2, 2, None, COEFF) == INVALID
    for size in (0, 1, 4, -1):
        assert call(A.c, B.c, px, COEFF, 1, size, po, COEFF) == INVALID and A.mod_switch_work_bytes(B, 1, size=size) == 0
    for form in (2, 3, 4, 5, 6, -1):                                                               # the packed and limb forms
        assert call(A.c, B.c, px, form, 2, 2, po, COEFF) == INVALID and call(A.c, B.c, px, COEFF, 2, 2, po, form) == INVALID
        assert A.mod_switch_work_bytes(B, 2, in_form=form) == 0 and A.mod_switch_work_bytes(B, 2, out_form=form) == 0
    assert (out == np.uint64(0xabababababababab)).all()
    # an output that overlaps the input: in place at the front, and shifted into its middle
    keep = x.copy()
    flat = x.reshape(-1)
    assert call(A.c, B.c, px, COEFF, 2, 3, px, COEFF) == INVALID
    mid = ctypes.cast(ctypes.addressof(px.contents) + 8 * (flat.size - 5), PU)
    assert call(A.c, B.c, px, COEFF, 2, 3, mid, COEFF) == INVALID
    assert np.array_equal(x, keep)
    # what is allowed: count = 0 writes nothing, and the work-bytes query answers for every admitted pair
    assert call(A.c, B.c, px, COEFF, 0, 2, po, COEFF) == 0 and (out == np.uint64(0xabababababababab)).all()
    for size in (2, 3):
        for fi in (COEFF, NTT):
            for fo in (COEFF, NTT):
                assert A.mod_switch_work_bytes(B, 5, size=size, in_form=fi, out_form=fo) >= 256
    rows = 5 * 2 * n * 8
    assert A.mod_switch_work_bytes(B, 5, in_form=NTT, out_form=NTT) - 256 == rows * (A.k - B.k)       # the dropped rows only
    assert A.mod_switch_work_bytes(B, 5, in_form=NTT, out_form=COEFF) - 256 == rows * A.k
    assert A.mod_switch_work_bytes(B, 5, in_form=COEFF, out_form=NTT) == 256 == A.mod_switch_work_bytes(B, 5)
    with pytest.raises(ValueError):
        A.level(0)
    with pytest.raises(ValueError):
        A.level(3)
    with pytest.raises(ca.binding.CrcError):
        B.mod_switch(A, np.zeros((1, 2, 2, n), dtype=np.uint64))
    A.close(); B.close()


@pytest.mark.parametrize("n,q,kept", [(256, SMALL, 2), (256, SMALL, 1), (256, K3, 1), (1024, K3, 2)], ids=["small_3to2", "small_3to1", "k3_3to1", "n1024_3to2"])
def test_decryption_and_budget_across_levels(n, q, kept):
    """a ciphertext of A, switched, decrypts to the same plaintext under the prefix rows of the secret key, with at least the derived budget (less 2 bits)"""
    A, B = engines(n, q, kept)
    sk, pk = A.keygen(21)
    rng = np.random.RandomState(n + kept)
    plains = rng.randint(0, T, size=(3, n)).astype(np.uint64)
    cts = A.encrypt(pk, plains, 77)
    assert np.array_equal(A.decrypt(sk, cts), plains)
    low = A.mod_switch(B, cts)
    skB = np.ascontiguousarray(sk[:kept])
    assert np.array_equal(B.decrypt(skB, low), plains)
    qB = mm.product(q[:kept])
    for i in range(3):
        bA = A.noise_budget(sk, cts[i]); bB = B.noise_budget(skB, low[i])
        bound = mm.budget_bound(bA, T, n, qB)
        print(f"n={n} {len(q)}->{kept}: budget {bA} -> {bB}, derived bound {bound}")
        assert bB >= bound - 2 and bound - 2 > 0
    # the prefix rows of the public key encrypt under B for the same secret key
    fresh = B.encrypt(np.ascontiguousarray(pk[:, :kept]), plains, 78)
    assert np.array_equal(B.decrypt(skB, fresh), plains)
    A.close(); B.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/mod_switch_kernel_check.cpp: the bodies of the three kernels (csrc/modswitch_device.h) on the CPU, one thread per workgroup over each launch's
    whole grid, with the address and undefined-behaviour sanitizers, equal the host twin bit for bit for all four form pairs on buffers of exactly the stated
    sizes -- every pass structure of the row transform (n = 64 .. 16384), lazy and strict butterflies, one to three drops"""
    import tempfile
    import crcnn_amd as ca
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "mod_switch_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mod_switch_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    d = {n: ca.default_coeff_modulus_128(n) for n in (4096, 8192, 16384)}
    q5 = list(dict.fromkeys(d[8192] + d[16384]))[:5]
    strict = [ca.Engine.slots_prime(512, b) for b in (60, 59, 58, 61 - 4)]
    cases = [(64, 2, SMALL), (64, 1, SMALL), (128, 1, SMALL_R), (256, 2, K3), (256, 1, K3), (256, 1, SMALL[:2]), (512, 1, strict), (512, 3, strict),
             (1024, 2, K3), (2048, 1, K3), (4096, 1, d[4096]), (4096, 2, K3), (8192, 3, q5), (16384, 3, d[16384][:4])]
    for n, kept, q in cases:
        out = subprocess.run([exe, str(n), str(kept), "4"] + [str(v) for v in q], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, kept, q, out.stdout, out.stderr[-1500:])
        assert ("lazy=1" in out.stdout) == all(v < (1 << 57) for v in q)
