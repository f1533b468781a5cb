"""Slot batching over several plain moduli on the host: crc_slots_crt_decompose / crc_slots_crt_act (the host twins, any context) against tests/slots_crt_model.py,
the degenerate base r = 1 against the existing calls, crc_slots_crt_primes, every refusal in its order, and the two kernels' own text on the CPU under sanitizers
against the twins.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import slots_crt_model as cm
import slots_model as sm
from test_gpu_slots_rescale import DIVISORS

Q1 = [0x3fffffff000001]
OK, INVALID, PARAMETERS, NOT_FOUND = 0, -1, -2, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


def bases():
    """(n, moduli) of the issue's table"""
    import crcnn_amd as ca
    return [(64, [769, 641]), (256, [15361, 13313, 12289, 11777]), (256, [ca.Engine.slots_prime(256, 40), 7681]), (2048, [1032193, 995329, 974849])]


def make_base(n, ts, device=-1, q=Q1):
    import crcnn_amd as ca
    return ca.SlotsCrt([ca.Engine(n, q, t, device=device) for t in ts])


def close(B):
    for e in B.E:
        e.close()


def edge_values(T, D):
    """0, +-1, the extremes, the ties +-D/2 and +-3D/2, +-D and +-D-+1, where they fit"""
    half = (T - 1) // 2
    v = [0, 1, -1, half, -half]
    for m in (1, 3):
        if D % 2 == 0:
            v += [m * (D // 2), -m * (D // 2)]
    v += [D, -D, D - 1, -D + 1]
    return [x for x in v if -half <= x <= half]


def rows_for(B, D, count, seed):
    """[r][count][n]: arbitrary 64-bit words; row 1 composed from the edge values of (T, D); row 2 the same with t_j added to every third word"""
    rng = np.random.RandomState(seed)
    r, n = B.r, B.n
    rows = rng.randint(0, 1 << 63, size=(r, count, n), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, size=(r, count, n)).astype(np.uint64)
    v = (edge_values(B.T, D) + [0] * n)[:n]
    one = B.compose(np.array([v], dtype=np.int64), 1, n, n, 1)
    for j in range(r):
        rows[j, 1] = one[j, 0]
        rows[j, 2] = one[j, 0]
        rows[j, 2, ::3] += np.uint64(B.ts[j])
    return rows, v


def slot_rows(B, rows):
    """the slots of every row mod its t_j by the existing host call (held against tests/slots_model.py by tests/test_slots_cpu.py): [r][count][n] Python ints"""
    return [B.E[j].slots_decompose(rows[j], B.n, B.n, 1).reshape(-1, B.n).tolist() for j in range(B.r)]


@pytest.mark.parametrize("case", range(4))
def test_host_twins_equal_the_model(case):
    n, ts = bases()[case]
    B = make_base(n, ts)
    assert B.supported and B.T == cm.product(ts) < 1 << 63
    half = (B.T - 1) // 2
    count = 4
    for D in [d for d in DIVISORS if d <= half]:
        rows, v = rows_for(B, D, count, 11 * n + D % 1000)
        slots = slot_rows(B, rows)
        want = [cm.decompose([slots[j][c] for j in range(B.r)], ts) for c in range(count)]
        assert want[1] == v and want[2] == v                    # what the composed rows hold, words >= t_j included
        assert B.decompose(rows, n, n, 1).reshape(count, n).tolist() == want, (n, ts, D)
        # image-major strides and fewer slots than n: untouched words stay
        part = n - 3
        got = B.decompose(rows, part, 1, count, size=part * count + 5)
        assert got[:part * count].reshape(part, count).T.tolist() == [w[:part] for w in want] and not got[part * count:].any()
        if n == 64:                                             # the whole path in the model: Horner at every point, no engine transform
            pure = [cm.decompose([sm.decompose([int(x) % ts[j] for x in rows[j][c]], n, ts[j]) for j in range(B.r)], ts) for c in range(count)]
            assert pure == want
        for relu, cap in ((0, 0), (1, 0), (0, min(1000, half)), (1, half), (1, 1)):
            got = B.act(rows, D, relu, cap)
            assert got.shape == (B.r, count, n) and all(int(got[j].max()) < ts[j] for j in range(B.r))
            back = slot_rows(B, got)
            for c in range(count):
                assert [back[j][c] for j in range(B.r)] == cm.act([slots[j][c] for j in range(B.r)], ts, D, relu, cap), (n, ts, D, relu, cap, c)
            # the results lift to the model's integers, and rows 1 and 2 agree
            assert B.decompose(got, n, n, 1).reshape(count, n)[1].tolist() == [cm.act_value(x, D, relu, cap) for x in v]
            assert all(np.array_equal(got[j, 1], got[j, 2]) for j in range(B.r))
            if n == 64 and D == 3:                              # the rows themselves, word for word, from the model's own interpolation
                for j in range(B.r):
                    assert [int(x) for x in got[j, 1]] == sm.compose(cm.act(slots_of(v, ts), ts, D, relu, cap)[j], n, ts[j])
    close(B)


def slots_of(v, ts):
    return [[x % t for x in v] for t in ts]


def test_one_modulus_is_the_existing_calls():
    """r = 1 is crc_slots_decompose and crc_slots_act on a 1 x 1 window, bit for bit -- lazy (30-bit) and strict (60-bit) butterflies"""
    import crcnn_amd as ca
    n = 256
    for t in (ca.Engine.slots_prime(n, 30), ca.Engine.slots_prime(n, 60)):
        B = make_base(n, [t])
        E = B.E[0]
        assert B.supported and B.T == t
        for D in DIVISORS:
            rows, _ = rows_for(B, D, 5, D % 1000)
            assert np.array_equal(B.decompose(rows, n, n, 1), E.slots_decompose(rows[0], n, n, 1))
            assert np.array_equal(B.decompose(rows, 7, 3, 40, size=300), E.slots_decompose(rows[0], 7, 3, 40, size=300))
            for relu, cap in ((0, 0), (1, 0), (1, 50), (0, (t - 1) // 2)):
                assert np.array_equal(B.act(rows, D, relu, cap)[0], E.slots_act(rows[0], 5, (1, 1, 1, 1, 1, 1), D, relu, cap)), (t, D, relu, cap)
            assert np.array_equal(B.act(rows, D)[0], E.slots_rescale(rows[0], D))
        close(B)


def test_primes():
    import crcnn_amd as ca
    P = ca.SlotsCrt.primes
    assert P(64, 2, 10) == [769, 641]
    assert P(256, 4, 14) == [15361, 13313, 12289, 11777]
    assert P(2048, 3, 20) == [1032193, 995329, 974849]
    assert P(256, 1, 40) == [ca.Engine.slots_prime(256, 40)]
    for n, r, bits in ((64, 2, 10), (256, 4, 14), (2048, 3, 20), (8192, 2, 31), (16384, 2, 31)):
        ts = P(n, r, bits)
        want, c = [], (1 << bits) - 1
        while len(want) < r:                                    # by trial, as tests/slots_model.py's slots_prime
            if c % (2 * n) == 1 and sm.is_prime(c):
                want.append(c)
            c -= 1
        assert ts == want
    L = ca.binding.load()
    t = np.full(5, 7, dtype=np.uint64)
    pt = t.ctypes.data_as(ca.binding.PU)
    assert L.crc_slots_crt_primes(4096, 4, 18, pt) == NOT_FOUND          # four 18-bit primes: the product passes 2^63
    assert L.crc_slots_crt_primes(4096, 4, 15, pt) == NOT_FOUND          # only 12289 ... too few primes 1 mod 8192 below 2^15
    assert L.crc_slots_crt_primes(4096, 0, 18, pt) == INVALID and L.crc_slots_crt_primes(4096, 5, 18, pt) == INVALID
    assert L.crc_slots_crt_primes(4095, 2, 18, pt) == INVALID and L.crc_slots_crt_primes(4096, 2, 61, pt) == INVALID and L.crc_slots_crt_primes(4096, 2, 18, None) == INVALID
    assert (t == 7).all()
    assert L.crc_slots_crt_primes(4096, 3, 18, pt) == OK and (t[3:] == 7).all()


def test_refusals_in_their_order():
    import crcnn_amd as ca
    n = 256
    L = ca.binding.load()
    good = [ca.Engine(n, Q1, t, device=-1) for t in (15361, 13313, 12289, 11777)]
    extra = ca.Engine(n, Q1, 10753, device=-1)                 # a fifth slot prime
    same = ca.Engine(n, Q1, 15361, device=-1)
    noslots = ca.Engine(n, Q1, 1 << 20, device=-1)
    other_n = ca.Engine(512, Q1, 12289, device=-1)
    big = [ca.Engine(n, Q1, ca.Engine.slots_prime(n, 40), device=-1), ca.Engine(n, Q1, ca.Engine.slots_prime(n, 30), device=-1)]      # the product passes 2^63
    arr = lambda es: (VP * len(es))(*[e.c if e is not None else None for e in es])
    count = 2
    bufs = [np.ones((count, n), dtype=np.uint64) for _ in range(4)]
    outs = [np.full((count, n), 5, dtype=np.uint64) for _ in range(4)]
    vals = np.full(count * n, 9, dtype=np.int64)
    rows = lambda bs: (VP * len(bs))(*[b.ctypes.data if b is not None else None for b in bs])
    pv = vals.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    T = 15361 * 13313
    dec = lambda es, r, pl=None, slots=n, ist=n, sst=1, v=pv: L.crc_slots_crt_decompose(arr(es), r, rows(pl if pl is not None else bufs[:len(es)]), count, slots, v, ist, sst)
    act = lambda es, r, D=3, relu=0, cap=0, i=None, o=None: L.crc_slots_crt_act(arr(es), r, rows(i if i is not None else bufs[:len(es)]), count, D, relu, cap,
                                                                                 rows(o if o is not None else outs[:len(es)]))
    assert L.crc_slots_crt_supported(arr(good), 4) == 1 and L.crc_slots_crt_supported(arr(good[:2]), 2) == 1 and L.crc_slots_crt_supported(arr(good[:1]), 1) == 1
    for es in ([good[0], same], [good[0], noslots], [good[0], other_n], big, [good[0], None]):
        assert L.crc_slots_crt_supported(arr(es), 2) == 0
    assert L.crc_slots_crt_supported(arr(good), 0) == 0 and L.crc_slots_crt_supported(arr(good + [extra]), 5) == 0 and L.crc_slots_crt_supported(None, 1) == 0
    # 1. r outside [1, 4] or a null entry: INVALID whatever else is wrong
    assert dec(good, 0) == INVALID and dec(good + [extra], 5) == INVALID and dec([good[0], None], 2) == INVALID and dec([noslots, None], 2, slots=0) == INVALID
    assert act(good, 0, D=0) == INVALID and act(good + [extra], 5) == INVALID and act([None, noslots], 2) == INVALID
    # 2. no base: PARAMETERS whatever else is wrong
    for es in ([good[0], same], [good[0], noslots], [good[0], other_n], big):
        assert dec(es, 2) == PARAMETERS and dec(es, 2, slots=0, ist=0) == PARAMETERS and dec(es, 2, pl=[None, None]) == PARAMETERS
        assert act(es, 2) == PARAMETERS and act(es, 2, D=0, relu=7, cap=1 << 63) == PARAMETERS
    # 3. the values
    two = good[:2]
    assert dec(two, 2) == OK and act(two, 2) == OK
    vals[:] = 9
    for o in outs:
        o[:] = 5
    assert dec(two, 2, slots=0) == INVALID and dec(two, 2, slots=n + 1) == INVALID and dec(two, 2, ist=0) == INVALID and dec(two, 2, sst=0) == INVALID
    assert dec(two, 2, pl=[bufs[0], None]) == INVALID and dec(two, 2, v=None) == INVALID
    assert act(two, 2, D=0) == INVALID and act(two, 2, D=(1 << 62) + 1) == INVALID and act(two, 2, D=1 << 62) == OK
    for o in outs:
        o[:] = 5
    assert act(two, 2, relu=2) == INVALID and act(two, 2, relu=-1) == INVALID
    assert act(two, 2, cap=(T - 1) // 2 + 1) == INVALID and act(two, 2, i=[bufs[0], None]) == INVALID and act(two, 2, o=[None, outs[1]]) == INVALID
    # an output row tensor is its own input or overlaps nothing
    assert act(two, 2, o=[bufs[1], bufs[0]]) == INVALID and act(two, 2, o=[outs[0], outs[0]]) == INVALID and act(two, 2, o=[outs[0], bufs[0]]) == INVALID
    both = np.ones((3 * count, n), dtype=np.uint64)
    assert act(two, 2, i=[both[:count], bufs[1]], o=[both[1:count + 1], outs[1]]) == INVALID
    assert (vals == 9).all() and all((o == 5).all() for o in outs) and all((b == 1).all() for b in bufs) and (both == 1).all()       # nothing written
    assert act(two, 2, cap=(T - 1) // 2) == OK
    io = [b.copy() for b in bufs[:2]]
    assert act(two, 2, i=io, o=io) == OK and all(np.array_equal(io[j], outs[j]) for j in range(2))                             # in place
    # count = 0
    assert L.crc_slots_crt_act(arr(two), 2, rows(bufs[:2]), 0, 3, 0, 0, rows(bufs[:2])) == OK
    assert L.crc_slots_crt_decompose(arr(two), 2, rows(bufs[:2]), 0, n, pv, n, 1) == OK
    B = ca.SlotsCrt(two)
    with pytest.raises(ca.CrcError):
        B.act(np.ones((2, 1, n), dtype=np.uint64), 0)
    assert B.refresh_dev_work_bytes(3) > 0 and ca.SlotsCrt([good[0], same]).refresh_dev_work_bytes(3) == 0 and B.refresh_dev_work_bytes(3, ca.NTTP) == 0
    # the device entry points on host-only contexts: INVALID, as from every device entry point
    assert L.crc_slots_crt_act_dev(arr(two), 2, rows(bufs[:2]), count, 3, 0, 0, rows(outs[:2]), None) == INVALID
    assert L.crc_slots_crt_decompose_dev(arr(two), 2, rows(bufs[:2]), count, n, vals.ctypes.data, n, 1, None) == INVALID
    for e in good + [extra, same, noslots, other_n] + big:
        e.close()


def test_the_kernels_text_on_the_cpu_under_sanitizers():
    """tests/cpp/slots_crt_kernel_check.cpp: the bodies of slots_crt_decompose_kernel and slots_crt_act_kernel (csrc/slots_device.h) on the CPU, one thread per
    workgroup, with the address and undefined-behaviour sanitizers, equal the host twins bit for bit on buffers of exactly the documented sizes, at n = 64 and
    256 (and 128, where the gap-1 stage is fused): r = 1 .. 4, moduli of unequal size, lazy butterflies and (r = 1, a 60-bit t) strict ones"""
    import tempfile
    import crcnn_amd as ca
    lib = os.path.join(ROOT, "crcnn_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "slots_crt_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "slots_crt_kernel_check.cpp"), "-o", exe, "-L", lib, "-lcrcnn_hip", "-Wl,-rpath," + lib])
    p40, s60 = ca.Engine.slots_prime(256, 40), ca.Engine.slots_prime(256, 60)
    cases = [(64, 3, 5, [769, 641]), (64, 1, 100, [257]), (128, 6, 9, [257, 769]), (128, 1 << 7, 3, [769, 257, 3329]),
             (256, 1 << 7, 1000, [15361, 13313, 12289, 11777]), (256, 1, 77, [p40, 7681]), (256, 1 << 39, 3, [7681, p40]), (256, 3, 1 << 30, [ca.Engine.slots_prime(256, 30), 7681, 12289]),
             (256, 3, 12, [s60]), (256, 1 << 62, 1, [s60]), (256, 1 << 39, (s60 - 1) // 2, [s60])]
    for n, D, cap, ts in cases:
        out = subprocess.run([exe, str(n), str(D), str(cap)] + [str(t) for t in ts], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (n, D, ts, out.stdout, out.stderr[-1500:])
        assert ("fused=1" in out.stdout) == (n == 128) and f"r={len(ts)} " in out.stdout
        assert ("lazy=1" in out.stdout) == all(t < (1 << 57) for t in ts)
