"""The 64-bit row transform without a GPU: the device text of crcnn_amd/csrc/ntt_device.h (reduce_small, shoup_lazy4, the lazy and strict butterflies, ntt_row_passes
with and without the fused gap-1 stage, inv_stages_unscaled with the kernels' constants) run by tests/cpp/ntt_rows_check.cpp on one emulated thread against unsigned
__int128 arithmetic and a textbook transform, over every modulus-width class ntt_launch tells apart.  The program stands alone (own tables from a root found by
search, no project library) and is built with the address and undefined-behaviour sanitizers; nothing sanitized is loaded into Python."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(tempfile.mkdtemp(), "ntt_rows_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ntt_rows_check.cpp"), "-o", path])
    return path


def test_primitives_rows_and_unscaled_stages(exe):
    """eight lazy-class primes (45, 45, 52, 53, 54, 55, 56, 57 bits): reduce_small over the multiples of q, the limit and 2 10^6 random values, shoup_lazy4 over the
    top of the word, w = q - 1 and 2 10^6 random pairs (its [3q, 4q) range reached for every prime), whole rows at n = 64, 128, 256, 8192, 16384 with FUSE1 off and
    on; the strict rows over the 44-, 58- and 60-bit primes; inv_stages_unscaled<3> / <4> at operands of 16 q - 1 for q = 0x7fffffffe90001"""
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok", r.stdout
    f = dict(zip(last[1::2], last[2::2]))
    # 11 primes x 5 rings x (FUSE1 off, on) x 3 rows x (forward, inverse, forward back)
    assert int(f["primes"]) == 8 and int(f["strict"]) == 3 and int(f["transforms"]) == 11 * 5 * 2 * 3 * 3, r.stdout
    # local passes: 2 rings x 3 gaps x 3 blocks x 64 trials x 12 butterflies; cross stages: 64 x 12 (n = 8192) + 64 x 32 (n = 16384)
    assert int(f["unscaled_butterflies"]) == 2 * 3 * 3 * 64 * 12 + 64 * 12 + 64 * 32, r.stdout
    assert int(f["min_max_k"]) == 3, r.stdout
    bits = [int(l.split("bits=")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("lazy ")]
    assert bits == [45, 45, 52, 53, 54, 55, 56, 57], bits


@pytest.mark.parametrize("q,ring", [(0x7fffffffff18001, 8192), (0xffffffffffe8001, 64)], ids=["59-bit", "60-bit"])
def test_the_check_sees_a_modulus_too_wide_for_the_lazy_butterflies(exe, q, ring):
    """the same lazy checks over ONE prime beyond the admitted range must report a mismatch: the forward transform lets values grow to (1 + 4 log2 n) q, which
    passes 2^64 at 60 bits from n = 64 on and at 59 bits from n = 8192 on.  (A 58-bit prime does NOT fail: 57 q < 2^64 still holds below 2^58 -- the dispatcher's
    limit of 57 bits keeps the sums below 2^63, one bit more than the arithmetic needs -- and the program passes over 0x200000000208001 as a lazy modulus.)"""
    assert q.bit_length() in (59, 60) and q % 32768 == 1
    r = subprocess.run([exe, "lazy", hex(q)], capture_output=True, text=True)
    assert r.returncode == 1 and f"FAILED forward rows q={q:x} n={ring} " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
