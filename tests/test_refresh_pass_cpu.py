"""The pass length of the client-side refreshes (crcnn_amd/host/refresh_pass.h) without a GPU: tests/cpp/refresh_pass_check.cpp holds refresh_pass_len against the
two computations the four refresh drivers had, at item sizes around the 4 GiB / 1024 threshold, and walks a model of the driver's loop.  The program is built with
the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_length_and_walk():
    exe = os.path.join(tempfile.mkdtemp(), "refresh_pass_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "refresh_pass_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    words = out.split()
    # 6 item sizes (0, which the drivers guard, among them), 6 item counts, 3 ciphertexts per item; the walks of 10^7 items take millions of passes
    assert int(words[1]) == 6 * 6 * 3 and int(words[3]) > 10_000_000, out
