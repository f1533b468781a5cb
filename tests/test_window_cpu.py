"""The window geometry of crcnn_amd/csrc/window.h without a GPU: tests/cpp/window_check.cpp walks every one-axis shape with an image of 1..16, a stride of 1..4 and a
window of 1..17 the way the reference walks it, each beside a different shape on the other axis, and compares Window::ok, xo, yo, P, the folded window of every
admitted sum pool, the window on the box sums of every box of at most 9 terms and pool_geom with what the walk found.  The program is built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(tempfile.mkdtemp(), "window_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "window_check.cpp"), "-o", path])
    return path


def test_every_window_fold_and_box(exe):
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    words = out.split()
    windows, valid, folds, boxes, indices = (int(words[i]) for i in (1, 3, 5, 7, 9))
    # 16 x 4 x 17 one-axis shapes, each once on either axis, and the valid ones twice more among themselves; of 12 pools and 23 boxes per valid window a good part
    # fits a 16-pixel image
    assert windows > 1088 and valid > 500 and folds > 2 * valid and boxes > 4 * valid and indices > 1_000_000, out
