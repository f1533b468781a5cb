"""CPU check of the seven-diagonal, one-fold reduction of the pixel-major one-channel kernel (crcnn_amd/csrc/limbred.h) against 128-bit arithmetic."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seven_diagonal_reduction_against_int128():
    """tests/cpp/limbred7_check.cpp: for every modulus conv1_fold7_ok accepts among default_coeff_modulus_128(n), n = 2048 .. 16384 (all eight), the kernel's
    arithmetic replayed on the CPU -- image digits x digits of centred(w 256^l mod q) into seven int32 diagonals, pack, one fold, bias, centring -- equals
    sum x w + bias mod q in 128-bit arithmetic: random, edge and extreme-digit operands at 1, 36, 40 and 64 taps, and worst-case diagonals at 64 taps (U > 0,
    U >> b within 20 bits, the folded value below 2q); conv1_fold7_ok refuses f >= 2^26 and moduli outside 53..55 bits"""
    exe = os.path.join(tempfile.mkdtemp(), "limbred7_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "limbred7_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    assert int(out.split()[1]) > 200_000
