"""The boxed forward transform without a GPU: the index helpers of crcnn_amd/csrc/nttbox.h, which ntt_rows_wave_kernel<.., BOX = true> and its launcher run on,
walked by tests/cpp/ntt_box_index_check.cpp over every shape of tests/test_gpu_ntt_box.py and PlainModelTiny's 28 x 28 image with the 2 x 2 box for 1, 2, 3 and
128 images, both block orders -- every output row exactly once, padding blocks answered "return", every term's source row inside the input and equal to the
naive formula, the grouped order walking whole planes per XCD.  The program is built with the address and undefined-behaviour sanitizers.  (That the window sum
itself stays inside sum_reduce16's bound -- 9 (q - 1) for the eight default moduli -- is tests/cpp/box_sum_check.cpp's.)"""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(tempfile.mkdtemp(), "ntt_box_index_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ntt_box_index_check.cpp"), "-o", path])
    return path


def test_every_shape_and_order(exe):
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    words = out.split()
    shapes, rows, terms, padding = int(words[1]), int(words[3]), int(words[5]), int(words[7])
    # 7 boxes x 3 moduli counts + 4 image counts, in two orders
    assert shapes == 2 * (7 * 3 + 4), out
    # PlainModelTiny's share alone: (1 + 2 + 3 + 128) images x 26 x 26 pixels x 2 polys x 2 moduli, four terms each, per order
    tiny = 134 * 676 * 4
    assert rows > 2 * tiny and terms > 2 * 4 * tiny, out
    # the grouped order pads every launch whose plane count is no multiple of 8 (3 images: 6, 12, 18 planes), the plain order none
    assert padding > 0, out
