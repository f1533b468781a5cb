"""The row table and the staging layout of the one-channel matrix-core convolution without a GPU: the helpers of crcnn_amd/csrc/conv1_rowtab.h, which
mfma_conv1_kernel_px fills its table with and both kernels stage their limb result by, walked by tests/cpp/conv1_rowtab_check.cpp over the shapes of
tests/test_gpu_conv1_staging_layout.py and a sweep of small geometries -- every entry equal to the expressions the kernel computed per tile before, every window
inside the image, every staged dword inside the staging area, distinct, and where the consumer's limb tensor has it.  The program is built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_table_every_shape():
    exe = os.path.join(tempfile.mkdtemp(), "conv1_rowtab_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "conv1_rowtab_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    shapes, entries, dwords = (int(v) for v in out.split()[1::2])
    assert shapes > 5_000 and entries > 1_000_000 and dwords > 10_000_000, out
