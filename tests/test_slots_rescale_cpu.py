"""The slot-wise rescale on the host: crc_slots_rescale (the host twin, any context) against tests/slots_rescale_model.py, the kernel's own text on the CPU under
sanitizers against that twin, and the `rescale NAME BITS` line through the description parsers and the scale ledger (`test_host slots_describe`).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import slots_model as sm
import slots_rescale_model as rm

Q1 = [0x3fffffff000001]
BIG = 0x7fffffff380001
PARAMETERS, INVALID = -2, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = os.path.join(ROOT, "tests", "golden", "slots")


def engine(n, t):
    import crcnn_amd as ca
    return ca.Engine(n, Q1, t, device=-1)


def strict_prime(n=256):
    import crcnn_amd as ca
    return ca.Engine.slots_prime(n, 60)


def divisors(t):
    return [1, 2, 3, 6, 1 << 10, t - 1, t + 2, 1 << 62]


def edge_values(t, D, n, seed):
    """n centred slot values: the extremes, 0, every tie +-D/2 and +-3D/2 that fits, neighbours of multiples of D, random values"""
    half = (t - 1) // 2
    v = [half, -half, 0, 1, -1]
    for m in (1, 3):
        if D % 2 == 0 and m * (D // 2) <= half:
            v += [m * (D // 2), -m * (D // 2), m * (D // 2) - 1, -m * (D // 2) - 1, -m * (D // 2) + 1]
    for m in (1, 2):
        if m * D <= half:
            v += [m * D, -m * D, m * D - 1, -m * D + 1]
    v = [x for x in v if -half <= x <= half]
    rng = np.random.RandomState(seed)
    v += [int(rng.randint(0, 1 << 62)) % t - half for _ in range(n - len(v))]
    return v[:n]


@pytest.mark.parametrize("n,t", [(64, 257), (256, 7681), (256, BIG), (256, None)], ids=["n64_t257", "n256_t7681", "n256_t55bit", "n256_t60bit"])
def test_host_twin_equals_the_model(n, t):
    """every divisor of the issue's list; a row of chosen slot values (composed by the model's own interpolation), the same row with words >= t, a random row"""
    t = t or strict_prime()
    E = engine(n, t)
    rng = np.random.RandomState(n + 3)
    for D in divisors(t):
        v = edge_values(t, D, n, D % 1000 + n)
        p = sm.compose(v, n, t)
        big = [c + t if (i % 3 == 0 and c + t < (1 << 64)) else c for i, c in enumerate(p)]        # words >= t are taken mod t
        rnd = [int(rng.randint(0, 1 << 62)) for _ in range(n)]
        rows = np.array([p, big, rnd], dtype=np.uint64)
        got = E.slots_rescale(rows, D)
        want_v = [rm.rescale_value(x, D) for x in v]
        assert got.max() < t
        assert [int(c) for c in got[0]] == sm.compose(want_v, n, t), (n, t, D, "composed row")
        assert np.array_equal(got[1], got[0]), (n, t, D, "words >= t")
        assert [int(c) for c in got[2]] == rm.rescale(rnd, n, t, D), (n, t, D, "random row")
        # the slots themselves: decompose gives the rescaled integers
        assert [int(x) for x in E.slots_decompose(got[:1], n, n, 1)] == want_v
        if D == 1:
            assert [int(c) for c in got[2]] == [c % t for c in rnd]
    zero = E.slots_rescale(np.zeros((1, n), dtype=np.uint64), 3)
    assert not zero.any()
    E.close()


def test_refusals():
    import crcnn_amd as ca
    n = 256
    pl = np.ones((1, n), dtype=np.uint64); out = np.zeros((1, n), dtype=np.uint64)
    pp, po = pl.ctypes.data_as(ca.binding.PU), out.ctypes.data_as(ca.binding.PU)
    G = engine(n, 7681)
    assert G.L.crc_slots_rescale(G.c, pp, 1, 3, po) == 0
    assert G.L.crc_slots_rescale(G.c, pp, 1, 0, po) == INVALID
    assert G.L.crc_slots_rescale(G.c, pp, 1, (1 << 62) + 1, po) == INVALID and G.L.crc_slots_rescale(G.c, pp, 1, 1 << 62, po) == 0
    assert G.L.crc_slots_rescale(G.c, None, 1, 3, po) == INVALID and G.L.crc_slots_rescale(G.c, pp, 1, 3, None) == INVALID
    assert G.L.crc_slots_rescale(G.c, pp, 0, 3, po) == 0
    with pytest.raises(ca.binding.CrcError):
        G.slots_rescale(pl, 0)
    G.close()
    E = engine(n, 1 << 20)                                     # no slots: CRC_ERR_PARAMETERS first, whatever else is wrong
    assert E.L.crc_slots_rescale(E.c, pp, 1, 3, po) == PARAMETERS and E.L.crc_slots_rescale(E.c, pp, 1, 0, po) == PARAMETERS
    E.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/slots_rescale_kernel_check.cpp: the body of slots_rescale_kernel (csrc/slots_device.h) on the CPU, one thread per workgroup, with the address and
    undefined-behaviour sanitizers, equals the host twin bit for bit, out of place and in place on buffers of exactly count * n words -- every pass structure of
    the row transform (n = 64 .. 16384; the gap-1 stage fused at 128, 1024 and 8192, a pass of its own or absent elsewhere), a 13-, 30-, 55- and 60-bit t -- and the
    reciprocal quotient equals unsigned __int128 division over edge magnitudes"""
    import tempfile
    import crcnn_amd as ca
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "slots_rescale_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "slots_rescale_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    p30 = {n: ca.Engine.slots_prime(n, 30) for n in (256, 2048, 4096, 8192)}
    strict = strict_prime()
    cases = [(64, 257, 3), (64, 257, 1), (128, 257, 2), (256, 7681, 6), (256, p30[256], 1 << 10), (256, BIG, 1 << 39), (256, BIG, BIG - 1), (256, strict, 3),
             (256, strict, 1 << 62), (256, strict, strict + 2), (512, 12289, 5), (1024, 12289, 2), (1024, 12289, 1), (2048, p30[2048], 1 << 7),
             (4096, p30[4096], 3), (8192, p30[8192], 6), (8192, p30[8192], 1), (8192, ca.Engine.slots_prime(8192, 60), 1 << 39),
             (16384, ca.Engine.slots_prime(16384, 50), 1 << 7)]
    for n, t, D in cases:
        out = subprocess.run([exe, str(n), str(t), str(D)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, t, D, out.stdout, out.stderr[-1500:])
        assert ("fused=1" in out.stdout) == (n in (128, 1024, 8192))              # log2 n = 3 m + 1


# ---- descriptions ------------------------------------------------------------------------------------------------------------------------------------------
def _driver():
    return os.path.join(ROOT, "crcnn_amd", "lib", "test_host")


def _describe(path, in_bits, w_bits):
    return subprocess.run([_driver(), "slots_describe", str(path), str(in_bits), str(w_bits)], capture_output=True, text=True)


def _ledger_rows(out):
    rows = [l.split() for l in out.stdout.splitlines()]
    return rows[:-1], rows[-1]


@pytest.mark.parametrize("name", ["approx_poly_rescale_act1", "approx_poly_rescale_pool2", "tiny_rescale"])
def test_slots_describe_prints_the_models_ledger(name):
    from crcnn_amd import netrun
    path = os.path.join(SLOTS, name + ".net")
    layers = netrun.load_description(path)
    out = _describe(path, 4, 5)
    assert out.returncode == 0, out.stderr
    rows, last = _ledger_rows(out)
    want = rm.ledger(list(layers), 4, 5)
    assert [(r[2], r[3]) for r in rows] == [(k, nm) for k, nm, _ in layers]
    assert [float(r[4]) for r in rows] + [float(last[1])] == [float(s) for s in want] and last[0] == "slot_scale"
    if name == "approx_poly_rescale_act1":
        at = [k for k, _, _ in layers].index("rescale")
        assert float(rows[at][4]) == 2.0 ** 47 and float(rows[at + 1][4]) == 2.0 ** 8 and float(last[1]) == 2.0 ** 25


def test_approx_poly_without_the_line_is_still_refused(tmp_path):
    text = open(os.path.join(SLOTS, "approx_poly_rescale_act1.net")).read()
    assert "rescale r 8\n" in text
    p = tmp_path / "plain.net"
    p.write_text(text.replace("rescale r 8\n", ""))
    out = _describe(p, 4, 5)
    assert out.returncode != 0 and "line " in out.stderr and "scale" in out.stderr
    gold = os.path.join(ROOT, "tests", "golden", "activations", "approx_poly.net")
    assert _describe(gold, 4, 5).returncode != 0


SMALL = "input 1 6 6\nconv c stride 1 1 filter 3 3 filters 2\navgpool p stride 1 1 window 3 3\n%sfc f 3\n"


@pytest.mark.parametrize("line,ok,what", [
    ("rescale r 8\n", True, ""),                  # sigma = 2^4 2^5 9 = 4608 = 2^9 9: 2^8 divides it, D = 18
    ("rescale r 9\n", True, ""),
    ("rescale r 0\n", True, ""),
    ("rescale r 10\n", False, "line 4:"),         # 2^10 does not divide 4608
    ("rescale r 13\n", False, "line 4:"),         # 2^13 > sigma
    ("rescale r 31\n", False, "line 4:"),         # BITS outside 0..30
    ("rescale r -1\n", False, "line 4:"),
    ("rescale r\n", False, "line 4:"),            # BITS missing
    ("rescale 8\n", False, "line 4:"),            # the name is missing: `8` is taken as the name, the bit count is missing
    ("rescale\n", False, "line 4:"),
    ("rescale r 8 9\n", False, "line 4:"),
    ("rescale r 8 threads 2\n", False, "line 4:"),
])
def test_rescale_lines_admitted_and_refused(tmp_path, line, ok, what):
    from crcnn_amd import netrun
    p = tmp_path / "d.net"
    p.write_text(SMALL % line)
    out = _describe(p, 4, 5)
    if ok:
        assert out.returncode == 0, out.stderr
        layers = netrun.parse_description(SMALL % line)
        rows, last = _ledger_rows(out)
        want = rm.ledger(list(layers), 4, 5)
        assert [float(r[4]) for r in rows] + [float(last[1])] == [float(s) for s in want]
        return
    assert out.returncode != 0 and what in out.stderr, out.stderr
    # the Python parser refuses what is wrong with the line itself; the ledger (bits against sigma) is the C++ builder's and the model's
    bits = line.split()[2:3]
    ledger_only = len(line.split()) == 3 and bits[0].isdigit() and int(bits[0]) <= 30
    if ledger_only:
        with pytest.raises(ValueError):
            rm.ledger(list(netrun.parse_description(SMALL % line)), 4, 5)
    else:
        with pytest.raises(ValueError, match="line 4:"):
            netrun.parse_description(SMALL % line)


def test_canonical_text_agrees_between_the_hosts():
    """`test_host describe` (NetworkDescription::str) and netrun.format_description print the same canonical text, comments and `threads 1` gone"""
    from crcnn_amd import netrun
    for name in ("approx_poly_rescale_act1", "approx_poly_rescale_pool2", "tiny_rescale"):
        path = os.path.join(SLOTS, name + ".net")
        out = subprocess.run([_driver(), "describe", path], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        d = netrun.load_description(path)
        assert out.stdout == netrun.format_description(d)
        assert "rescale r" in out.stdout
        again = netrun.parse_description(out.stdout)
        assert list(again) == list(d) and netrun.format_description(again) == out.stdout
    # shapes pass through a rescale line
    d = netrun.parse_description(SMALL % "rescale r 8\n")
    assert [k for k, _, _ in d] == ["conv", "avgpool", "rescale", "fc"] and d[2][2] == {"bits": 8} and d[3][2]["in_dim"] == 2 * 2 * 2


def test_netrun_refuses_to_run_a_rescale():
    import crcnn_amd as ca
    from crcnn_amd import netrun
    E = ca.Engine(256, Q1, 7681, device=-1)
    w = {"c.weight": np.zeros(18, np.float32), "c.bias": np.zeros(2, np.float32), "f.weight": np.zeros(24, np.float32), "f.bias": np.zeros(3, np.float32)}
    text = SMALL % "rescale r 8\n"
    assert [k for k, _, _ in netrun.parse_description(text)].count("rescale") == 1          # the parser takes the line: what refuses it is the driver
    with pytest.raises(ValueError, match="no slot mode"):
        netrun.Network(E, text, weights=w)
    E.close()


def test_a_refresh_under_slot_encoding_is_still_refused(tmp_path):
    text = "input 1 6 6\nconv c stride 1 1 filter 3 3 filters 2\nsquare act\nrefresh\nrescale r 4\nfc f 3\n"
    p = tmp_path / "refresh.net"
    p.write_text(text)
    out = _describe(p, 4, 5)
    assert out.returncode != 0 and "line 4: refresh is not available with slot encoding" in out.stderr
    p.write_text(text.replace("refresh\n", ""))
    assert _describe(p, 4, 5).returncode == 0
