"""The staged box of the pixel-major image pack without a GPU: the index helpers of crcnn_amd/csrc/boxstage.h, which limb_pack_box_kernel_px runs on, walked by
tests/cpp/box_stage_check.cpp over every input image up to 32 x 32, strides 1-3 and boxes of at most 9 terms -- global reads inside the image, LDS words inside
the allocation, every output pixel's terms the box's terms, every output pixel exactly once.  The program is built with the address and undefined-behaviour
sanitizers."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(tempfile.mkdtemp(), "box_stage_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "box_stage_check.cpp"), "-o", path])
    return path


def test_every_shape_and_walk(exe):
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    words = out.split()
    shapes, direct, pixels = int(words[1]), int(words[3]), int(words[5])
    # 32 x 32 images x 9 stride pairs x 22 boxes, less the boxes that leave no pixel; tall boxes at stride 2-3 on wide images do not fit the LDS and are read directly
    assert shapes > 100_000 and 0 < direct < shapes // 10 and pixels > 10_000_000, out


@pytest.mark.parametrize("yd,bxf,xs,ydo,path", [(28, 2, 2, 26, "staged"), (32, 2, 2, 30, "staged"), (21, 3, 2, 17, "staged"), (32, 9, 3, 32, "direct")],
                         ids=["tiny", "widest", "halo-past-group", "9x1-stride-3"])
def test_which_body(exe, yd, bxf, xs, ydo, path):
    out = subprocess.check_output([exe, "path", str(yd), str(bxf), str(xs), str(ydo)], text=True).split()
    assert out[0] == path and (int(out[1]) <= 160 * 1024) == (path == "staged"), out
    if (yd, bxf) == (28, 2):
        assert int(out[1]) == 6 * 28 * 32 * 8 + 32 * (4 * 208 + 16)              # PlainModelTiny: 42 KiB of ring, 26.5 KiB of digit staging
