"""The plan of Network::forward (crcnn_amd/host): which form every layer hands its tensor over in, which multiply-accumulate kernel a conv / dense layer
runs on and how often every layer is launched.  tests/test_gpu_host_cpp.py checks the output ciphertexts bit for bit, but a boundary that falls back from a limb
hand-over to packed rows, or a layer that falls back to the vector-ALU kernel, produces the same ciphertexts, only slower: `test_host plan` prints the table and
the tables below pin it.  They were recorded from the commit in front of the one that split Network::forward into plan / timing / range runner / chunk loop
(that commit's host library with only the `plan` subcommand added to the driver), not from the code they check."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from netcommon import GOLD, load_net_golden, make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "crcnn_amd", "lib", "test_host")


def run_plan(name, batch, fuse, head_chunk, matrix_cores, refresh):
    """the lines `test_host plan` prints.  refresh: place the refresh where the golden's reference run had it (with the client's keys in the directory, as
    test_gpu_host_cpp._run_refresh_config writes them); otherwise none"""
    g = load_net_golden(name)
    O, sk, pk, evk, img, x = make_inputs(g)
    d = tempfile.mkdtemp()
    try:
        np.array([g["n"], len(g["q"]), g["t"]] + g["q"], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
        evk.tofile(os.path.join(d, "evk.u64")); x.tofile(os.path.join(d, "net_in.u64"))
        if refresh:
            sk.tofile(os.path.join(d, "sk.u64")); pk.tofile(os.path.join(d, "pk.u64"))
        h5 = os.path.join(GOLD, "models", g["model"] + ".h5")
        out = subprocess.run([DRIVER, "plan", g["model"], h5, d, str(batch), "1" if fuse else "0", str(head_chunk), "1" if matrix_cores else "0",
                              str(g["layer_before_reenc"] if refresh else -1)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.split("\n") if l.startswith(("plan ", "refresh "))]
    finally:
        shutil.rmtree(d, ignore_errors=True)


# out_form: 0 CRC_COEFF, 1 CRC_NTT, 2 CRC_NTTP (packed rows), 3 CRC_NTTL (a dense layer's limb tensor), 5 CRC_NTTLC (a convolution's limb tensor)
# case: (golden, batch, fuse, head_chunk, matrix_cores, refresh), then "refresh <layer>" and per layer "plan <i> <name> <out_form> <kernel> <launches>"
PLANS = {
    "tiny256-fused-b16": (('tiny256', 16, True, 0, True, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 1
plan 1 pool2_features.conv2+pool2 3 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 2 classifier.fc3 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 3 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "approx256-fused-b16": (('approx256', 16, True, 0, True, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 1
plan 1 pool1_features.norm1+pool2_features.conv2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 2 act1+pool2 1 - 1
plan 3 pool2_features.norm2+classifier.fc3 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 4 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "wopad256-fused-b16": (('wopad256', 16, True, 0, True, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 1
plan 1 pool1_features.norm1+pool2_features.conv2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 2 act1+pool2 1 - 1
plan 3 pool2_features.norm2+classifier.fc3 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 4 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "wopad256-fused-b16-chunk3": (('wopad256', 16, True, 3, True, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 6
plan 1 pool1_features.norm1+pool2_features.conv2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 6
plan 2 act1+pool2 1 - 6
plan 3 pool2_features.norm2+classifier.fc3 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 4 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "tiny256-fused-b16-chunk3": (('tiny256', 16, True, 3, True, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 6
plan 1 pool2_features.conv2+pool2 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 6
plan 2 classifier.fc3 2 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 3 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "wopad256-fused-b3-valu": (('wopad256', 3, True, 0, False, False), """
refresh -1
plan 0 pool1_features.conv1+pool1 2 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 1 pool1_features.norm1+pool2_features.conv2 1 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 2 act1+pool2 1 - 1
plan 3 pool2_features.norm2+classifier.fc3 2 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 4 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "tiny256-unfused-b1": (('tiny256', 1, False, 0, True, False), """
refresh -1
plan 0 pool1_features.conv1 1 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 1 pool1 1 - 1
plan 2 pool2_features.conv2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 3 pool2 1 - 1
plan 4 classifier.fc3 2 mac_stream_kernel (weight stream: one image, two rows per weight; v_mad_u64_u32, CRC_NTTP) 1
plan 5 classifier.fc4 0 mac_stream_kernel (weight stream: one image, two rows per weight; v_mad_u64_u32, CRC_NTTP) 1
"""),
    "tiny2048r-fused-b5-refresh": (('tiny2048r', 5, True, 0, True, True), """
refresh 2
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 1
plan 1 pool2_features.conv2+pool2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 1
plan 2 classifier.fc3 2 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 3 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
    "tiny2048r-fused-b5-chunk2-refresh": (('tiny2048r', 5, True, 2, True, True), """
refresh 2
plan 0 pool1_features.conv1+pool1 5 mfma_conv1_kernel (one-channel convolution on the matrix cores, CRC_NTTL1) 3
plan 1 pool2_features.conv2+pool2 1 mfma_mac2w_kernel (int8 limb GEMM, CRC_NTTL) 3
plan 2 classifier.fc3 2 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
plan 3 classifier.fc4 0 mac3_kernel (v_mad_u64_u32, CRC_NTTP) 1
"""),
}


@pytest.mark.parametrize("case", sorted(PLANS))
def test_cpp_forward_plan_is_the_recorded_one(case):
    args, want = PLANS[case]
    got = run_plan(*args)
    print("\n".join(got))
    assert got == want.strip().split("\n"), case
