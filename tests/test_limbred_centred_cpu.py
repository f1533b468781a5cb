"""CPU check of the one-pass centred reduction of the limb GEMM's epilogue (crcnn_amd/csrc/limbred.h diag_reduce_w_centred) against the sequence it replaces and
against 128-bit arithmetic."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_centred_reduction_against_sequence_and_int128():
    """tests/cpp/limbred_centred_check.cpp: for every modulus of default_coeff_modulus_128(n), n = 2048 .. 16384, with a fold constant (all eight) and the bias
    tables of T = 32, 800, 1024, 1152 and 17 984 terms, diag_reduce_w_centred equals the centred representative of addmod(diag_reduce_w(D), bias) and of
    (U 2^-64 + bias) mod q in unsigned __int128 arithmetic: random diagonals within the tables' ranges, every diagonal at its largest and smallest admissible value,
    inputs whose result is exactly 0, (q - 1) / 2 and -(q - 1) / 2, biases 0, 1, (q - 1) / 2, (q + 1) / 2, q - 1, with and without HAS_BIAS"""
    exe = os.path.join(tempfile.mkdtemp(), "limbred_centred_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "limbred_centred_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    assert int(out.split()[1]) >= 200_000
