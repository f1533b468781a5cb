"""The scalar limb form (CRC_NTTLS) on host-only contexts: the size functions against the layout's formulas, crc_plan_mac_scalar's decisions for the layers of the
three CrCNN topologies, and argument refusals.  (The kernels are tests/test_gpu_scalar_mac.py's.)"""
import pytest

import crcnn_amd as ca

INVALID, UNSUPPORTED = -1, -4


def set_key(E, name, value):
    """(Engine.set_tuning synchronises a stream, which a host-only context has not)"""
    return E.L.crc_ctx_set_tuning(E.c, name.encode(), value)


def round_up(v, m):
    return -(-v // m) * m


def steps_of(zd, xf, yf):
    """32-term reduction steps: flat form below 32 channels (a window row's (ky, channel) run in 32-byte pieces, channels rounded up to 4), else 32-channel blocks"""
    if zd < 32:
        return xf * -(-(yf * round_up(zd, 4)) // 32)
    return xf * yf * (round_up(zd, 32) // 32)


@pytest.fixture(scope="module")
def ctxs():
    T = ca.Engine(4096, ca.default_coeff_modulus_128(4096), 1 << 32, device=-1)
    A = ca.Engine(8192, ca.default_coeff_modulus_128(8192)[:3], 1 << 42, device=-1)
    W8 = ca.Engine(16384, ca.default_coeff_modulus_128(16384), 1 << 44, device=-1)
    yield T, A, W8
    for E in (T, A, W8):
        E.close()


def test_size_functions(ctxs):
    """[k][steps rounded up to even][7][filters rounded up to 64][32] bytes: crc_limb_weights_bytes / n"""
    for E in ctxs:
        for nf, zd, xf, yf in ((64, 32, 6, 6), (50, 20, 3, 3), (33, 40, 3, 3), (10, 70, 1, 1), (512, 1024, 1, 1), (500, 800, 1, 1), (1, 1, 1, 1)):
            want = E.k * round_up(steps_of(zd, xf, yf), 2) * 7 * round_up(nf, 64) * 32
            assert E.scalar_weights_bytes(nf, zd, xf, yf) == want
            assert E.limb_weights_bytes(nf, zd, xf, yf) == want * E.n
    T = ctxs[0]
    assert T.scalar_weights_bytes(0, 32, 1, 1) == 0 and T.scalar_weights_bytes(10, 0, 1, 1) == 0 and T.scalar_weights_bytes(10, 32, 0, 1) == 0
    assert T.L.crc_scalar_weights_bytes(None, 10, 32, 1, 1) == 0
    # the dense tensor and the work space are CRC_NTTL's: same bytes, other row order
    for in_form in (ca.NTT, ca.NTTP, ca.COEFF, ca.NTTLS):
        assert T.conv2d_forms_work_bytes(3, 1000, 1, 1, 1, 1, 1, 1, 33, in_form, ca.NTTLS, ca.NTT) == \
            T.conv2d_forms_work_bytes(3, 1000, 1, 1, 1, 1, 1, 1, 33, ca.NTTL if in_form == ca.NTTLS else in_form, ca.NTTL, ca.NTT)
    assert T.conv2d_forms_work_bytes(2, 40, 7, 7, 1, 1, 3, 3, 33, ca.NTTL, ca.NTTLS, ca.NTTLS) == T.conv2d_forms_work_bytes(2, 40, 7, 7, 1, 1, 3, 3, 33, ca.NTTL, ca.NTTL, ca.NTTL)


def test_plan_mac_scalar(ctxs):
    """the scalar form for conv2 / fc3 / fc4 of the three models on one ciphertext tensor per launch (where crc_plan_mac's rows guard sends the dense layers to the
    vector ALU), CRC_NTTL1 kept for conv1; with the key scalar_mac off crc_plan_mac's answers"""
    T, A, W8 = ctxs
    conv1 = {T: (1, 28, 28, 2, 2, 6, 6, 32), A: (1, 28, 28, 2, 2, 7, 7, 20), W8: (1, 28, 28, 2, 2, 7, 7, 20)}
    macs = {T: [(32, 12, 12, 2, 2, 6, 6, 64), (1024, 1, 1, 1, 1, 1, 1, 512), (512, 1, 1, 1, 1, 1, 1, 10)],
            A: [(20, 11, 11, 2, 2, 3, 3, 50), (800, 1, 1, 1, 1, 1, 1, 500), (500, 1, 1, 1, 1, 1, 1, 10)],
            W8: [(20, 11, 11, 2, 2, 3, 3, 50), (800, 1, 1, 1, 1, 1, 1, 500), (500, 1, 1, 1, 1, 1, 1, 10)]}
    for E in ctxs:
        assert E.plan_mac_scalar(*macs[E][1], 1) == ca.NTTLS                  # the key's default: on (profiles/scalar_mac.md)
        assert set_key(E, "scalar_mac", 0) == 0
        for B in (0, 1, 5):
            for g in macs[E] + [conv1[E]]:
                assert E.plan_mac_scalar(*g, B) == E.plan_mac(*g, B)
        assert set_key(E, "scalar_mac", 1) == 0
        try:
            for B in (0, 1, 5):
                for g in macs[E]:
                    assert E.scalar_supported(max(B, 1), *g)
                    assert E.plan_mac_scalar(*g, B) == ca.NTTLS, (E.n, g, B)
                assert E.plan_mac_scalar(*conv1[E], B) == ca.NTTL1
            assert E.plan_mac(1024, 1, 1, 1, 1, 1, 1, 512, 1) == ca.NTTP          # crc_plan_mac itself does not change
            # a two-channel layer is a GEMM already; one channel that is no conv1 shape keeps crc_plan_mac's answer
            assert E.plan_mac_scalar(2, 1, 1, 1, 1, 1, 1, 10, 1) == ca.NTTLS
            assert E.plan_mac_scalar(1, 40, 40, 2, 2, 6, 6, 32, 1) == E.plan_mac(1, 40, 40, 2, 2, 6, 6, 32, 1)
            # past the term limit and past the offset limit: crc_plan_mac's answer
            assert E.plan_mac_scalar(18001, 1, 1, 1, 1, 1, 1, 3, 1) == E.plan_mac(18001, 1, 1, 1, 1, 1, 1, 3, 1) != ca.NTTLS
            assert E.plan_mac_scalar(1000, 1, 1, 1, 1, 1, 1, 33, 1 << 20) != ca.NTTLS
        finally:
            assert set_key(E, "scalar_mac", 1) == 0
    # moduli above 55 bits keep their kernels
    G = ca.Engine(128, [0xffffffffffc0001], 1 << 20, device=-1)
    assert not G.scalar_supported(1, 70, 1, 1, 1, 1, 1, 1, 10)
    assert G.plan_mac_scalar(70, 1, 1, 1, 1, 1, 1, 10, 1) == ca.NTT
    G.close()


def test_argument_refusals(ctxs):
    T = ctxs[0]
    good = (1, 70, 1, 1, 1, 1, 1, 1, 10)
    assert T.scalar_supported(*good)
    for bad in ((0,) + good[1:], (1, 0) + good[2:], good[:8] + (0,), (1, 70, 1, 1, 0, 1, 1, 1, 10), (1, 70, 2, 2, 1, 1, 3, 3, 10)):
        assert not T.scalar_supported(*bad)
    assert T.L.crc_scalar_supported(None, *good) == 0
    import ctypes
    wf = ctypes.c_int(0)
    assert T.L.crc_plan_mac_scalar(None, 70, 1, 1, 1, 1, 1, 1, 10, 1, ctypes.byref(wf)) == INVALID
    assert T.L.crc_plan_mac_scalar(T.c, 70, 1, 1, 1, 1, 1, 1, 10, 1, None) == INVALID
    assert T.L.crc_plan_mac_scalar(T.c, 0, 1, 1, 1, 1, 1, 1, 10, 1, ctypes.byref(wf)) == INVALID
    assert T.L.crc_plan_mac_scalar(T.c, 70, 2, 2, 1, 1, 3, 3, 10, 1, ctypes.byref(wf)) == INVALID
    # a host-only context launches nothing: the pack and the forms call refuse it, and a refusal of the arguments is not a finding about the rows
    const = ctypes.c_int(0)
    assert T.L.crc_scalar_pack_weights(T.c, 16, T.n, 10, 70, 1, 1, 16, ctypes.byref(const), None) == INVALID and const.value == 1
    assert T.L.crc_conv2d_forms(T.c, 16, 16, ca.NTTLS, None, 1, 70, 1, 1, 1, 1, 1, 1, 10, ca.NTT, ca.NTT, 16, 16, None) == INVALID
    assert set_key(T, "scalar_macs", 1) == -6            # CRC_ERR_NOT_FOUND: no such key
