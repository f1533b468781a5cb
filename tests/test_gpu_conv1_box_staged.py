"""GPU exactness of the STAGED box of the one-channel convolution's image pack (kernels_mfma1.hip limb_pack_box_kernel_px: every input residue loaded once into a
ring in LDS, the window sums taken from there), n = 256, k = 2, the moduli and the operand classes of test_gpu_conv1_box.py.

The reference of every case is the unboxed path on a host-summed image: the box sums of the canonical residues mod q in numpy, then crc_conv2d_forms (NTTL1) on
that xdo x ydo image -- limb_pack_rows1_kernel_px<false> and the same convolution, neither of which the staged box touches.  Bit for bit, as NTT rows and as the
limb tensor (NTTLC).  Where the enlarged window is at most 8 x 8 the same map with the box folded into the weights, on the vector-ALU kernel, is compared too.
Every case first asserts limb_conv1_box_supported and form 2 (Boxed.__init__).

Shapes, the smallest that exercise what staging adds: a halo longer than a row group with an odd summed width and a ragged last group of one row (3 x 3 box at
stride 2 on 21 x 21); nine terms at stride 1 with every residue q - 1 and at the centring boundaries; summed widths 15, 16 and 17 around the two 16-column halves
of a row under 1 x 2 and 2 x 2 boxes, with summed heights 5 (one full group and one ragged row), 3 and 4 (below and at one group) and 6; the widest image (32 x
32, 2 x 2 box: 30 x 30 sums, the largest ring that PlainModelTiny's kind of layer asks for); 28-bit packed and coefficient-form input; three images in
one-image passes; and the one box family whose ring does not fit the LDS (9 x 1 at stride 3 on a 32-wide image), which keeps the direct-read body: the case asks
tests/cpp/box_stage_check.cpp -- the launcher's own predicate, boxstage.h box_staged -- which body its shape takes, and does so for a staged shape as well."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_gpu_conv1_box import BOUNDARY, Q, eng, make  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = ((1, 21, 21, 2, 2, 3, 3, 8), (3, 3))
NINE = ((1, 14, 14, 1, 1, 3, 3, 32), (3, 3))
WIDEST = ((1, 32, 32, 2, 2, 6, 6, 32), (2, 2))
DIRECT = ((1, 32, 32, 3, 1, 3, 2, 8), (9, 1))


def summed_shape(base, box):
    zd, xd, yd, xs, ys, xf, yf, nf = base
    return xd - (box[0] - 1) * xs, yd - (box[1] - 1) * ys


def host_box_sum(L):
    """the window sums of the canonical residues mod q: at most 9 terms below 2^55, exact in uint64"""
    zd, xd, yd, xs, ys, xf, yf, nf = L.base
    xdo, ydo = summed_shape(L.base, L.box)
    acc = np.zeros((L.B, xdo, ydo) + L.x.shape[3:], dtype=np.uint64)
    for a in range(L.box[0]):
        for b in range(L.box[1]):
            acc += L.x[:, a * xs:a * xs + xdo, b * ys:b * ys + ydo]
    for i, q in enumerate(Q):
        acc[..., i, :] %= np.uint64(q)
    return np.ascontiguousarray(acc)


def unboxed(L, fout=None):
    """the base layer on the host-summed image: the pack without a box, the same convolution, the bias of the fold"""
    E, ca = L.E, L.ca
    fout = ca.NTT if fout is None else fout
    zd, xd, yd, xs, ys, xf, yf, nf = L.base
    xdo, ydo = summed_shape(L.base, L.box)
    small = (zd, xdo, ydo, xs, ys, xf, yf, nf)
    assert E.limb_conv1_supported(*small) and E.limb_conv1_form(*small) == 2
    d_xs = E.upload(host_box_sum(L))
    d_y, nbytes = L._out(fout)
    d_work = E.alloc(E.conv2d_forms_work_bytes(L.B, *small, ca.NTT, ca.NTTL1, fout))
    E.conv2d(d_xs, L.d_wl, L.d_bbig, L.B, *small, ca.NTT, fout, d_y, d_work, w_form=ca.NTTL1)
    E.sync()
    out = E.download(d_y, (nbytes // 8,))
    d_y.free(); d_work.free(); d_xs.free()
    return out


def check(L, vector_alu=True):
    E, ca = L.E, L.ca
    want = unboxed(L)
    assert want.size == L.rows * E.n
    assert np.array_equal(L.boxed(), want), (L.base, L.box)
    assert np.array_equal(L.boxed(fout=ca.NTTLC), unboxed(L, ca.NTTLC)), (L.base, L.box)
    if vector_alu:
        assert max(L.big[5], L.big[6]) <= 8
        assert np.array_equal(L.enlarged(ca.NTT), want), (L.base, L.box)
    return want


@pytest.fixture(scope="module")
def which_body():
    exe = os.path.join(tempfile.mkdtemp(), "box_stage_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "box_stage_check.cpp"), "-o", exe])

    def ask(base, box):
        xdo, ydo = summed_shape(base, box)
        return subprocess.check_output([exe, "path", str(base[2]), str(box[0]), str(base[3]), str(ydo)], text=True).split()[0]
    return ask


@pytest.fixture(scope="module")
def halo(eng):
    """3 x 3 box at stride 2: a halo of 4 rows, longer than a row group; 17 x 17 sums (an odd width, 4 full row groups and a ragged one of one row), 8 x 8 outputs"""
    E, ca = eng
    L = make(E, ca, *HALO, 2, 911)
    assert summed_shape(*HALO) == (17, 17) and (L.xo, L.yo) == (8, 8)
    return L, check(L)


def test_halo_longer_than_a_row_group(halo, which_body):
    assert which_body(*HALO) == "staged"


@pytest.mark.parametrize("kind", ["all-q-1", "centring"])
def test_nine_terms_at_stride_one(eng, kind):
    E, ca = eng
    L = make(E, ca, *NINE, 2, 912, BOUNDARY[kind])
    assert summed_shape(*NINE) == (12, 12)
    check(L)


@pytest.mark.parametrize("xd,yd,box", [(6, 16, (2, 2)), (4, 17, (2, 2)), (6, 18, (2, 2)), (4, 16, (1, 2)), (6, 17, (1, 2)), (5, 18, (1, 2))],
                         ids=["5x15-2x2", "3x16-2x2", "5x17-2x2", "4x15-1x2", "6x16-1x2", "5x17-1x2"])
def test_widths_around_the_column_halves(eng, xd, yd, box):
    """3 x 3 / 1 base window; summed widths 15, 16, 17; summed heights 5 (a full group and a ragged row), 3 (below a group), 4 and 6"""
    E, ca = eng
    L = make(E, ca, (1, xd, yd, 1, 1, 3, 3, 8), box, 2, 913 + xd + yd)
    check(L)


def test_widest_image(eng, which_body):
    E, ca = eng
    L = make(E, ca, *WIDEST, 2, 914)
    assert summed_shape(*WIDEST) == (30, 30) and (L.xo, L.yo) == (13, 13) and which_body(*WIDEST) == "staged"
    check(L)


def test_packed_and_coefficient_inputs(eng, halo):
    E, ca = eng
    L, want = halo
    zd, xd, yd = L.base[:3]
    d_xp = E.upload(L.x); E.pack28(d_xp, L.B * xd * yd * 2 * E.k)
    assert np.array_equal(L.boxed(fin=ca.NTTP, d_x=d_xp), want), "28-bit packed input"
    d_xc = E.upload(L.x); E.ntt_inv(d_xc, L.B * xd * yd)
    assert np.array_equal(L.boxed(fin=ca.COEFF, d_x=d_xc), want), "coefficient-form input"
    assert np.array_equal(L.boxed(fin=ca.COEFF, fout=ca.NTTLC, d_x=d_xc), unboxed(L, ca.NTTLC)), "coefficient-form input, limb tensor"


def test_three_images_in_one_image_passes(eng, request):
    E, ca = eng
    request.addfinalizer(lambda: E.set_tuning("conv1_pass_bytes", 0))
    L = make(E, ca, *HALO, 3, 915)
    want, want_limb = unboxed(L), unboxed(L, ca.NTTLC)
    whole = E.conv2d_box_forms_work_bytes(3, *L.base, *L.box, ca.NTT, ca.NTTL1, ca.NTT)
    E.set_tuning("conv1_pass_bytes", whole * 2 // 5)
    assert E.conv2d_box_forms_work_bytes(3, *L.base, *L.box, ca.NTT, ca.NTTL1, ca.NTT) < whole * 3 // 5
    assert np.array_equal(L.boxed(), want)
    assert np.array_equal(L.boxed(fout=ca.NTTLC), want_limb)


def test_ring_past_the_lds_is_read_directly(eng, which_body):
    """9 x 1 at stride 3 on 32 x 32: 28 ring rows x 32 columns x 256 bytes = 224 KiB, more than a CU has: limb_pack_rows1_kernel_px<true>, the same bytes
    (a 3 x 2 base window: a stride above the window is no shape the library takes)"""
    E, ca = eng
    assert which_body(*DIRECT) == "direct"
    L = make(E, ca, *DIRECT, 2, 916)
    assert summed_shape(*DIRECT) == (8, 32) and (L.xo, L.yo) == (2, 31)
    check(L, vector_alu=False)
