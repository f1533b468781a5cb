"""The client-side activation of slot-batched networks on the host: crc_slots_act (the host twin, any context) against tests/slots_act_model.py, the kernel's own
text on the CPU under sanitizers against that twin, and the `client_relu` / `client_maxpool` lines through both description parsers and the scale ledger.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import slots_act_model as am
import slots_model as sm
import slots_rescale_model as rm

Q1 = [0x3fffffff000001]
PARAMETERS, INVALID = -2, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = os.path.join(ROOT, "tests", "golden", "slots")
XD, YD = 5, 4
# (xd, yd, xs, ys, xf, yf): 1 x 1, 2 x 2 / 2 (the fifth row of the image lies in no window), 3 x 3 / 1 (overlapping), 2 x 3 / (1, 2)
WINDOWS = [(XD, YD, 1, 1, 1, 1), (XD, YD, 2, 2, 2, 2), (XD, YD, 1, 1, 3, 3), (XD, YD, 1, 2, 2, 3)]


def engine(n, t):
    import crcnn_amd as ca
    return ca.Engine(n, Q1, t, device=-1)


def primes(n):
    import crcnn_amd as ca
    return [ca.Engine.slots_prime(n, 30), 257, ca.Engine.slots_prime(n, 60)]


def caps(t):
    half = (t - 1) // 2
    return [0, 1, min(50, half // 2), half]


def slot_values(n, t, D, seed):
    """centred slot values [planes][XD][YD][n].  Every edge value e -- the extremes +-(t - 1)/2, 0, +-1, the ties +-D/2 and +-3D/2, the values that land on every cap
    and on cap +- 1 behind the division -- sits in one row of a slot whose other rows hold random values <= e, so e is the maximum of every window that holds
    its row.  The last three slots: a negative value in every row (every window's maximum is negative), 0 in every row, -(t - 1)/2 in every row"""
    half = (t - 1) // 2
    edge = [half, -half, 0, 1, -1]
    for m in (1, 3):
        if D % 2 == 0 and m * (D // 2) <= half:
            edge += [m * (D // 2), -m * (D // 2), m * (D // 2) - 1, -m * (D // 2) - 1]
    for c in caps(t)[1:]:
        edge += [(c + d) * D for d in (-1, 0, 1) if (c + d) * D <= half]
        edge += [c * D + D // 2 - 1, c * D + D // 2, c * D - (D + 1) // 2, c * D - (D + 1) // 2 - 1]       # the rounding boundaries around the cap
    edge = [e for e in dict.fromkeys(edge) if -half <= e <= half]
    free = n - 3
    planes = (len(edge) + free - 1) // free
    rng = np.random.RandomState(seed)
    rnd = lambda lo, hi: lo + int(rng.randint(0, 1 << 62)) % (hi - lo + 1)
    v = [[[[rnd(-half, half) for _ in range(n)] for _ in range(YD)] for _ in range(XD)] for _ in range(planes)]
    for k, e in enumerate(edge):
        pl, s = divmod(k, free)
        for r in range(XD * YD):
            v[pl][r // YD][r % YD][s] = e if r == (3 * k) % (XD * YD) else rnd(-half, e)
    for pl in range(planes):
        for i in range(XD):
            for j in range(YD):
                v[pl][i][j][n - 3] = rnd(-half, -1)
                v[pl][i][j][n - 2] = 0
                v[pl][i][j][n - 1] = -half
    return v, planes


@pytest.mark.parametrize("n", [16, 32, 64, 128])
def test_host_twin_equals_the_model(n):
    """Every t, divisor, window, relu and cap of the issue's lists.  The rows are composed once per (t, D) by the model's own interpolation.  The full comparison
    -- the twin's rows against the model's rows, word for word -- runs for one (D, relu, cap) per window; every other combination is compared slot by slot through
    crc_slots_decompose with the rows canonical (below t): decompose is a bijection on canonical rows (tests/test_slots_cpu.py holds it against the same model),
    so equal slots are equal rows, at a fraction of the O(n^2) interpolations.
    n = 16 and n = 32: the library has no ring below 64 (crc_ctx_create answers CRC_ERR_PARAMETERS, as it always has), so no host twin exists there; at these
    sizes the model is held against itself (both orders of maximum and division, act_rows against act_slots) and the refusal is asserted.  n = 64 (log2 n = 6, no
    gap-1 pass of its own) and n = 128 (log2 n = 7, the gap-1 stage fused) are the two structures"""
    if n < 64:
        import crcnn_amd as ca
        for t in primes(n):
            with pytest.raises(ca.binding.CrcError):
                engine(n, t)
            for D in [d for d in (1, 3, 1 << 7, 1 << 39) if d <= (t - 1) // 2]:
                v, planes = slot_values(n, t, D, n + D % 1000)
                rows = [sm.compose(v[pl][i][j], n, t) for pl in range(planes) for i in range(XD) for j in range(YD)]
                for wi, w in enumerate(WINDOWS):
                    relu, cap = wi % 2, caps(t)[wi]
                    want = am.act_slots(v, planes, w, D, relu, cap)
                    assert am.act_slots(v, planes, w, D, relu, cap, divide_first=True) == want
                    if D == 3:
                        assert am.act_rows(rows, planes, w, n, t, D, relu, cap) == [sm.compose(cell, n, t) for plane in want for row in plane for cell in row]
        return
    for t in primes(n):
        E = engine(n, t)
        half = (t - 1) // 2
        Ds = [d for d in (1, 3, 1 << 7, 1 << 39) if d <= half]
        for D in Ds:
            v, planes = slot_values(n, t, D, n + D % 1000)
            rows = np.array([sm.compose(v[pl][i][j], n, t) for pl in range(planes) for i in range(XD) for j in range(YD)], dtype=np.uint64)
            for wi, w in enumerate(WINDOWS):
                for relu in (0, 1):
                    for ci, cap in enumerate(caps(t)):
                        got = E.slots_act(rows, planes, w, D, relu, cap)
                        want = am.act_slots(v, planes, w, D, relu, cap)
                        flat = [cell for plane in want for row in plane for cell in row]
                        assert got.shape == (len(flat), n) and int(got.max()) < t
                        assert E.slots_decompose(got, n, n, 1).reshape(len(flat), n).tolist() == flat, (n, t, D, w, relu, cap)
                        if (relu, ci) == (wi % 2, wi) and D == Ds[wi % len(Ds)]:
                            assert [[int(c) for c in r] for r in got] == [sm.compose(cell, n, t) for cell in flat], (n, t, D, w, relu, cap, "rows")
                            if n == 64 and D == 3:
                                assert [[int(c) for c in r] for r in got] == am.act_rows(rows, planes, w, n, t, D, relu, cap)
                        # max-then-divide equals divide-then-max
                        if ci < 2:
                            assert am.act_slots(v, planes, w, D, relu, cap, divide_first=True) == want
                # relu = 0, cap = 0, a 1 x 1 window of stride 1: the rescale, bit for bit -- on words >= t and on any 64-bit words too
                if wi == 0:
                    big = rows.copy()
                    if t < (1 << 63):
                        big[:, ::3] += np.uint64(t)
                    rnd = np.random.RandomState(n).randint(0, 1 << 63, size=rows.shape, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
                    for r in (rows, big, rnd):
                        assert np.array_equal(E.slots_act(r, planes, w, D, 0, 0), E.slots_rescale(r, D)), (n, t, D)
                    assert np.array_equal(E.slots_act(big, planes, w, D, 1, caps(t)[2]), E.slots_act(rows, planes, w, D, 1, caps(t)[2]))
                    assert [[int(c) for c in r] for r in E.slots_rescale(rows[:2], D)] == [rm.rescale(rows[k], n, t, D) for k in range(2)]
        # words >= t under a window, and an all-zero input
        w = WINDOWS[2]
        assert np.array_equal(E.slots_act(big, planes, w, 3, 0, 0), E.slots_act(rows, planes, w, 3, 0, 0))
        assert not E.slots_act(np.zeros((XD * YD, n), dtype=np.uint64), 1, w, 3, 1, 1).any()
        E.close()


def test_refusals():
    import crcnn_amd as ca
    n, t = 256, 7681
    pl = np.ones((XD * YD, n), dtype=np.uint64); out = np.zeros((XD * YD, n), dtype=np.uint64)
    pp, po = pl.ctypes.data_as(ca.binding.PU), out.ctypes.data_as(ca.binding.PU)
    G = engine(n, t)
    call = lambda E, i, planes, w, D, relu, cap, o: E.L.crc_slots_act(E.c, i, planes, *w, D, relu, cap, o)
    W = WINDOWS[1]
    assert call(G, pp, 1, W, 3, 1, 5, po) == 0
    assert call(G, pp, 1, W, 0, 1, 5, po) == INVALID and call(G, pp, 1, W, (1 << 62) + 1, 0, 0, po) == INVALID and call(G, pp, 1, W, 1 << 62, 0, 0, po) == 0
    assert call(G, pp, 1, W, 3, 2, 0, po) == INVALID and call(G, pp, 1, W, 3, -1, 0, po) == INVALID               # relu outside {0, 1}
    assert call(G, pp, 1, W, 3, 0, (t - 1) // 2, po) == 0 and call(G, pp, 1, W, 3, 0, (t - 1) // 2 + 1, po) == INVALID
    for bad in [(XD, YD, 1, 1, 6, 1), (XD, YD, 1, 1, 1, 5), (XD, YD, 0, 1, 1, 1), (XD, YD, 1, 1, 0, 1), (0, YD, 1, 1, 1, 1), (XD, YD, 3, 3, 1, 1), (XD, YD, 1, 3, 1, 1)]:
        assert call(G, pp, 1, bad, 3, 0, 0, po) == INVALID, bad                                                    # (the last two: a stride remainder)
    assert call(G, None, 1, W, 3, 0, 0, po) == INVALID and call(G, pp, 1, W, 3, 0, 0, None) == INVALID
    assert call(G, pp, 0, W, 3, 0, 0, po) == 0                                                                      # no planes: nothing to do
    with pytest.raises(ca.binding.CrcError):
        G.slots_act(pl, 1, W, 0)
    G.close()
    E = engine(n, 1 << 20)                                     # no slots: CRC_ERR_PARAMETERS first, whatever else is wrong
    assert call(E, pp, 1, W, 3, 0, 0, po) == PARAMETERS and call(E, pp, 1, W, 0, 7, 1 << 40, po) == PARAMETERS and call(E, None, 1, (0, 0, 0, 0, 0, 0), 3, 0, 0, po) == PARAMETERS
    E.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/slots_act_kernel_check.cpp: the body of slots_act_kernel (csrc/slots_device.h) on the CPU, one thread per workgroup, with the address and
    undefined-behaviour sanitizers, equals the host twin bit for bit for both relu values, without and with the cap given, on buffers of exactly the documented
    sizes: lazy (13-, 30-, 50-bit t) and strict (60-bit t) butterflies, rings with the gap-1 stage fused (128, 1024, 8192), a pass of its own or absent, every
    window of the list -- 3 x 3 / 1 overlapping --, and the 1 x 1 window in place and against crc_slots_rescale"""
    import tempfile
    import crcnn_amd as ca
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "slots_act_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "slots_act_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    p30 = {n: ca.Engine.slots_prime(n, 30) for n in (256, 1024, 2048, 8192)}
    s60 = {n: ca.Engine.slots_prime(n, 60) for n in (128, 256, 8192)}
    one, pool, over, mixed = WINDOWS
    cases = [(64, 257, 3, pool, 5), (64, 257, 1, one, 100), (128, 257, 2, over, 7), (128, s60[128], 1 << 39, mixed, 1000), (256, 7681, 6, pool, 3000),
             (256, p30[256], 1 << 7, over, 1 << 20), (256, s60[256], 3, over, (s60[256] - 1) // 2), (256, s60[256], 1 << 62, one, 1), (512, 12289, 5, mixed, 6144),
             (1024, p30[1024], 1 << 7, pool, 77), (2048, p30[2048], 3, one, 12), (8192, p30[8192], 6, pool, 9), (8192, s60[8192], 1 << 39, over, 1 << 19),
             (16384, ca.Engine.slots_prime(16384, 50), 1 << 7, pool, 1 << 30)]
    for n, t, D, w, cap in cases:
        out = subprocess.run([exe, str(n), str(t), str(D)] + [str(x) for x in w] + [str(cap)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, t, D, w, out.stdout, out.stderr[-1500:])
        assert ("fused=1" in out.stdout) == (n in (128, 1024, 8192))              # log2 n = 3 m + 1
        assert ("lazy=1" in out.stdout) == (t < (1 << 57))


# ---- descriptions ------------------------------------------------------------------------------------------------------------------------------------------
def _driver():
    return os.path.join(ROOT, "crcnn_amd", "lib", "test_host")


def _describe(path, in_bits, w_bits):
    return subprocess.run([_driver(), "slots_describe", str(path), str(in_bits), str(w_bits)], capture_output=True, text=True)


def _ledger_rows(out):
    rows = [l.split() for l in out.stdout.splitlines()]
    return rows[:-1], rows[-1]


@pytest.mark.parametrize("name", ["tiny_client_maxpool", "tiny_client_relu_cap"])
def test_slots_describe_prints_the_models_ledger(name):
    from crcnn_amd import netrun
    path = os.path.join(SLOTS, name + ".net")
    layers = netrun.load_description(path)
    out = _describe(path, 4, 5)
    assert out.returncode == 0, out.stderr
    rows, last = _ledger_rows(out)
    want = am.ledger(list(layers), 4, 5)
    assert [(r[2], r[3]) for r in rows] == [(k, nm) for k, nm, _ in layers]
    assert [float(r[4]) for r in rows] + [float(last[1])] == [float(s) for s in want] and last[0] == "slot_scale"
    # by hand: 2^4 2^5 = 2^9 in front of mp1 (D = 2), 2^8 2^5 = 2^13 in front of mp2 and of a3 (D = 32), 2^13 behind fc4
    kinds = [k for k, _, _ in layers]
    assert [want[i] >> layers[i][2]["bits"] for i, k in enumerate(kinds) if k in am.CLIENT] == [2, 32, 32] and want[-1] == 1 << 13
    if name == "tiny_client_relu_cap":
        assert [am.cap_units(a) for k, _, a in layers if k in am.CLIENT] == [0, 128, 1536]


# conv c leaves 2 x 4 x 4 at sigma = 2^4 2^5 = 512
SMALL = "input 1 6 6\nconv c stride 1 1 filter 3 3 filters 2\n%sfc f 3\n"
LINES = [
    ("client_relu a 8\n", True), ("client_relu a 9\n", True), ("client_relu a 0\n", True), ("client_relu a 8 cap 6\n", True), ("client_relu a 0 cap 1.5\n", True),
    ("client_relu a 8 cap 0.002\n", True),                               # nearbyint(0.512) = 1
    ("client_maxpool m stride 2 2 window 2 2 bits 8\n", True), ("client_maxpool m stride 2 2 window 2 2 bits 8 relu\n", True),
    ("client_maxpool m stride 1 1 window 3 3 bits 0 relu cap 2.5\n", True), ("client_maxpool m stride 1 2 window 2 3 bits 9 cap 1\n", True),
    ("client_maxpool m stride 1 1 window 4 4 bits 8\n", True),
    ("client_relu a\n", False), ("client_relu\n", False), ("client_maxpool m stride 2 2 window 2 2\n", False), ("client_maxpool m stride 2 2 window 2 2 bits\n", False),
    ("client_maxpool m stride 2 2 window 2 2 8\n", False),               # BITS missing / without its keyword
    ("client_relu a 31\n", False), ("client_relu a -1\n", False), ("client_maxpool m stride 2 2 window 2 2 bits 31\n", False),
    ("client_relu a 10\n", False), ("client_maxpool m stride 2 2 window 2 2 bits 10\n", False),      # 2^10 does not divide 512
    ("client_relu a 8 cap 0.001\n", False), ("client_relu a 0 cap 0.5000001\n", True), ("client_relu a 0 cap 0.25\n", False), ("client_relu a 0 cap 0.5\n", False),      # nearbyint rounds half to even: 0 ("client_relu a 8 cap 0\n", False),
    ("client_relu a 8 cap -1\n", False), ("client_maxpool m stride 2 2 window 2 2 bits 8 cap 0.001\n", False), ("client_relu a 8 cap\n", False),
    ("client_relu a 8 cap x\n", False),
    ("client_relu a 8 9\n", False), ("client_relu a 8 relu\n", False), ("client_relu a 8 cap 6 7\n", False),
    ("client_maxpool m stride 2 2 window 2 2 bits 8 cap 1 relu\n", False), ("client_maxpool m stride 2 2 window 2 2 bits 8 relu relu\n", False),
    ("client_relu a 8 threads 2\n", False), ("client_maxpool m stride 2 2 window 2 2 bits 8 threads 2\n", False),
    ("client_maxpool m stride 1 1 window 5 5 bits 8\n", False), ("client_maxpool m stride 1 1 window 1 5 bits 8\n", False),      # larger than the 4 x 4 input
    ("client_maxpool m stride 3 3 window 1 1 bits 8\n", False), ("client_maxpool m stride 3 3 window 1 2 bits 8\n", False),      # a stride remainder
    ("client_maxpool m stride 0 1 window 2 2 bits 8\n", False),
]


@pytest.mark.parametrize("line,ok", LINES, ids=[l[0].strip().replace(" ", "_") or "empty" for l in LINES])
def test_client_lines_admitted_and_refused(tmp_path, line, ok):
    from crcnn_amd import netrun
    p = tmp_path / "d.net"
    p.write_text(SMALL % line)
    out = _describe(p, 4, 5)
    if ok:
        assert out.returncode == 0, out.stderr
        layers = netrun.parse_description(SMALL % line)
        rows, last = _ledger_rows(out)
        want = am.ledger(list(layers), 4, 5)
        assert [float(r[4]) for r in rows] + [float(last[1])] == [float(s) for s in want]
        assert want[2] == 1 << layers[1][2]["bits"] and want[1] == 512
        return
    assert out.returncode != 0 and "line 3:" in out.stderr, out.stderr
    # the Python parser refuses what is wrong with the line itself; the ledger (bits against sigma) is the C++ builder's and the model's
    if " 10\n" in line:
        with pytest.raises(ValueError):
            am.ledger(list(netrun.parse_description(SMALL % line)), 4, 5)
    else:
        with pytest.raises(ValueError, match="line 3:"):
            netrun.parse_description(SMALL % line)


def test_the_lines_need_slot_encoding(tmp_path):
    """what only the builder can refuse: outside slot encoding either line is refused with its line number (test_host build_plain: no engine, no slot encoding)"""
    for line in ("client_relu a 0\n", "client_maxpool m stride 2 2 window 2 2 bits 0 relu\n"):
        p = tmp_path / "first.net"
        p.write_text("input 1 4 4\n# a comment line\n" + line)
        out = subprocess.run([_driver(), "build_plain", str(p)], capture_output=True, text=True)
        assert out.returncode != 0 and "line 3: " + line.split()[0] + " needs slot encoding" in out.stderr, out.stderr
    p = tmp_path / "plain.net"
    p.write_text("input 1 4 4\npad p 1 1\n")
    out = subprocess.run([_driver(), "build_plain", str(p)], capture_output=True, text=True)
    assert out.returncode == 0 and "build_plain ok 1 layers" in out.stdout, out.stderr


def test_canonical_text_agrees_between_the_hosts():
    """`test_host describe` (NetworkDescription::str) and netrun.format_description print the same canonical text, comments and `threads 1` gone"""
    from crcnn_amd import netrun
    for name in ("tiny_client_maxpool", "tiny_client_relu_cap"):
        path = os.path.join(SLOTS, name + ".net")
        out = subprocess.run([_driver(), "describe", path], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        d = netrun.load_description(path)
        assert out.stdout == netrun.format_description(d)
        assert "client_maxpool mp1 stride 2 2 window 2 2 bits 8 relu\n" in out.stdout and "client_relu a3 8" in out.stdout
        again = netrun.parse_description(out.stdout)
        assert list(again) == list(d) and netrun.format_description(again) == out.stdout
    assert "client_relu a3 8 cap 6\n" in out.stdout and "bits 8 relu cap 0.5\n" in out.stdout
    # numbers are written as %.9g of their float32 on both sides
    import tempfile
    for line in [l for l, ok in LINES if ok]:
        with tempfile.NamedTemporaryFile("w", suffix=".net") as f:
            f.write(SMALL % line); f.flush()
            out = subprocess.run([_driver(), "describe", f.name], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout == netrun.format_description(netrun.parse_description(SMALL % line)), (line, out.stdout, out.stderr)
    # shapes pass through client_relu and change like a pool's through client_maxpool
    d = netrun.parse_description(SMALL % "client_maxpool m stride 2 2 window 2 2 bits 8 relu cap 0.5\n")
    assert [k for k, _, _ in d] == ["conv", "client_maxpool", "fc"] and d[2][2]["in_dim"] == 2 * 2 * 2
    assert d[1][2] == dict(xd=4, yd=4, zd=2, xs=2, ys=2, xf=2, yf=2, bits=8, relu=True, cap=0.5)
    d = netrun.parse_description(SMALL % "client_maxpool m stride 1 2 window 2 3 bits 8\n")
    assert d[2][2]["in_dim"] == 2 * 3 * 1 and d[1][2]["relu"] is False and d[1][2]["cap"] is None
    d = netrun.parse_description(SMALL % "client_relu a 8 cap 6\n")
    assert d[1][2] == dict(bits=8, cap=6.0) and d[2][2]["in_dim"] == 2 * 4 * 4
    # `relu` itself stays an unknown layer kind, and `rescale` keeps its grammar
    with pytest.raises(ValueError, match="line 3: unknown layer kind"):
        netrun.parse_description(SMALL % "relu act\n")
    with pytest.raises(ValueError, match="line 3:"):
        netrun.parse_description(SMALL % "rescale r 8 cap 6\n")


def test_netrun_refuses_to_run_either_line():
    import crcnn_amd as ca
    from crcnn_amd import netrun
    E = ca.Engine(256, Q1, 7681, device=-1)
    for line, in_dim in (("client_relu a 8\n", 32), ("client_maxpool m stride 2 2 window 2 2 bits 8 relu\n", 8)):
        w = {"c.weight": np.zeros(18, np.float32), "c.bias": np.zeros(2, np.float32), "f.weight": np.zeros(3 * in_dim, np.float32), "f.bias": np.zeros(3, np.float32)}
        text = SMALL % line
        assert [k for k, _, _ in netrun.parse_description(text)].count(line.split()[0]) == 1          # the parser takes the line: what refuses it is the driver
        with pytest.raises(ValueError, match="no slot mode"):
            netrun.Network(E, text, weights=w)
    E.close()
