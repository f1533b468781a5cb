#!/usr/bin/env python3
"""The polynomial activation c2 x^2 + c1 x + c0 against the Square + pooling chain it extends -> profiles/poly_activation.md.

Shapes: CrCNN's act1 + pool2 -- 50 channels of 5 x 5, 2 x 2 / 1 window: 1250 -> 800 ciphertexts per image -- at (8192, 3) and (16384, 4), in launches the size
the bench uses (32 and 6 images), NTT-resident in and out.  Timed per squared ciphertext with HIP events, alternating in the same process and repeated
`--rounds` times each (median and spread): crc_square_pool_relin_forms (the parent's code, unchanged), crc_poly2_pool_relin_forms with the fused tail
(poly_tail = 0) and with poly2_tail_kernel (poly_tail = 1), and pool_kernel on the same input tensor (its rate prices the extra read).

The gate: the DEFAULT tail may take no more than the Square + pooling time of the same run, plus the time to read the window's extra 8 n 2k bytes per input
ciphertext at the rate pool_kernel reached in that run, plus the measured spread.

One process per step, each under its own `timeout`, run one after the other and stopped at the first that fails:
    measure_poly.py                      the driver: every step below, then the report
    measure_poly.py step N K IMAGES      one shape, in process; prints one JSON line
    measure_poly.py trace N K IMAGES     the same calls once each, for a separate `rocprofv3 --kernel-trace --stats` run (kernel times)
Options: --rounds R (default 3), --reps (calls per timing, default 2), --out DIR (default a temporary directory), --markdown FILE, --no-bench, --no-trace."""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 3, 32), (16384, 4, 6)]          # n, k, images per launch (tools/benchkit/configs.py: approx8192, wopad16384)
ZD, XD, YD, XS, YS, XF, YF = 50, 5, 5, 1, 1, 2, 2
TRIPLE = (0.1997, 0.5002, 0.1992)
HBM_TBS = 8.0


def setup(n, k, B):
    import numpy as np
    import torch
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, 1 << 30, device=0)
    dev = torch.device("cuda", 0)
    E.stream = torch.cuda.current_stream().cuda_stream or None
    xo, yo = (XD - XF) // XS + 1, (YD - YF) // YS + 1
    cnt, ocnt = B * ZD * XD * YD, B * ZD * xo * yo
    g = torch.Generator(device=dev); g.manual_seed(1)
    x = torch.empty((cnt * 2 * k, n), dtype=torch.int64, device=dev)
    for i in range(k):
        x[i::k] = torch.randint(0, q[i], (cnt * 2, n), dtype=torch.int64, device=dev, generator=g)
    sk, pk = E.keygen(3); evk = E.upload(E.gen_evk(4, sk))
    geom = (B, ZD, XD, YD, XS, YS, XF, YF)
    work = torch.empty(max(E.square_pool_relin_work_bytes(*geom), E.poly2_pool_relin_work_bytes(*geom)) // 8 + 64, dtype=torch.int64, device=dev)
    outs = [torch.empty((ocnt * 2 * k, n), dtype=torch.int64, device=dev) for _ in range(4)]
    rows = E.poly2_rows(*TRIPLE, window=XF * YF)
    assert all(r is not None for r in rows)

    def square():
        E.square_pool_relin(x, *geom, evk, outs[0], work, in_form=ca.NTT, out_form=ca.NTT)

    def poly(tail, out):
        def fn():
            E.L.crc_ctx_set_tuning(E.c, b"poly_tail", tail)          # (read on the host when the call is made: no synchronisation needed between calls)
            E.poly2_pool_relin(x, *geom, evk, *rows, out, work, in_form=ca.NTT, out_form=ca.NTT)
        return fn

    def pool():
        E.pool(x, *geom, None, ca.NTT, outs[3])
    calls = {"square + pooling (crc_square_pool_relin_forms)": square, "poly + pooling, fused tail": poly(0, outs[1]),
             "poly + pooling, separate tail (poly2_tail_kernel)": poly(1, outs[2]), "pool_kernel on the same input": pool}
    return E, torch, calls, outs, cnt, ocnt


def events_ms(E, fn, reps):
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    E.L.crc_event_create(E.c, ctypes.byref(e0)); E.L.crc_event_create(E.c, ctypes.byref(e1))
    E.L.crc_event_record(E.c, e0, E.stream)
    for _ in range(reps):
        fn()
    E.L.crc_event_record(E.c, e1, E.stream)
    E.sync()
    ms = ctypes.c_float()
    E.L.crc_event_elapsed_ms(E.c, e0, e1, ctypes.byref(ms))
    E.L.crc_event_destroy(E.c, e0); E.L.crc_event_destroy(E.c, e1)
    return ms.value / reps


def step(n, k, B, rounds, reps):
    E, torch, calls, outs, cnt, ocnt = setup(n, k, B)
    for fn in calls.values():                    # warm-up: module load, LDS opt-in, the work buffer's first touch
        fn()
    E.sync()
    # the two tails must agree before either is timed (and differ from the square: the polynomial is another function)
    same = bool(torch.equal(outs[1], outs[2])); differs = not bool(torch.equal(outs[0], outs[1]))
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    E.L.crc_ctx_set_tuning(E.c, b"poly_tail", 0)
    ctb = 2 * k * n * 8
    res = dict(n=n, k=k, images=B, cts_in=cnt, cts_out=ocnt, ct_bytes=ctb, tails_agree=same, differs_from_square=differs, rounds=rounds, reps=reps,
               ms={nm: v for nm, v in ms.items()})
    print(json.dumps(res), flush=True)
    E.close()
    return 0 if same and differs else 3


def trace(n, k, B):
    E, torch, calls, outs, cnt, ocnt = setup(n, k, B)
    for _ in range(2):
        for fn in calls.values():
            fn()
    E.sync(); E.close()
    return 0


def run(cmd, limit, log):
    """one child process under its own time limit; returns its stdout, or None when it failed (the caller stops there)"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    return p.stdout if p.returncode == 0 else None


def kernel_stats(d):
    """kernel name -> (calls, average ns) from rocprofv3's kernel_stats csv"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            try:
                out[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
            except (KeyError, ValueError):
                pass
    return out


def bench_lines(out_dir, log, steps=2):
    """ApproxPlainModel against approx_poly.net through bench_host model=, the bench's own (8192, 3) configuration"""
    import numpy as np
    import crcnn_amd as ca
    from crcnn_amd import synth
    n, k, t = 8192, 3, 1 << 42
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=-1)
    sk, pk = E.keygen(1)
    pl, _ = E.encode(synth.normalize(synth.synth_image(0)).reshape(-1))
    inp = os.path.join(out_dir, "in.u64")
    E.encrypt(pk, pl, 7).tofile(inp)
    E.close()
    h5 = os.path.join(ROOT, "tests", "golden", "models", "ApproxPlainModel.h5")
    res = {}
    for tag, model in (("ApproxPlainModel (square act1)", "ApproxPlainModel"),
                       ("approx_poly.net (poly act1 0.1997 0.5002 0.1992)", os.path.join(ROOT, "tests", "golden", "activations", "approx_poly.net"))):
        cmd = [os.path.join(ROOT, "crcnn_amd", "lib", "bench_host"), f"model={model}", f"h5={h5}", f"n={n}", f"k={k}", f"t={t}", "q=" + ",".join(str(v) for v in q),
               f"inputs={inp}", "distinct=1", "batch=256", "chunk=32", "group=2", f"steps={steps}", "warmup=1"]
        out = run(cmd, 420, log)
        if out is None:
            return None
        res[tag] = json.loads(out.strip().splitlines()[-1])["images_per_s"]
    return res


def report(results, stats, bench, a):
    L = ["# Polynomial activation: poly + pooling against Square + pooling", "",
         "CrCNN's act1 + pool2 (50 channels of 5 x 5, 2 x 2 / 1 window: 1250 -> 800 ciphertexts per image), NTT-resident in and out, launches the size the bench uses.",
         f"HIP events around {a.reps} calls, the four calls alternating in one process, {a.rounds} rounds each: median (min .. max) in us per SQUARED ciphertext.", ""]
    verdicts = []
    for r in results:
        n, k, cnt = r["n"], r["k"], r["cts_in"]
        us = {nm: [1e3 * v / cnt for v in vs] for nm, vs in r["ms"].items()}
        names = list(us)
        sq, fused, sep, pool = (us[nm] for nm in names)
        L += [f"## (n, k) = ({n}, {k}), {r['images']} images per launch ({cnt} -> {r['cts_out']} ciphertexts)", "", "| call | us per squared ciphertext | min .. max |", "|---|---|---|"]
        for nm in names:
            L.append(f"| {nm} | {statistics.median(us[nm]):.3f} | {min(us[nm]):.3f} .. {max(us[nm]):.3f} |")
        pool_bytes = (cnt + r["cts_out"]) * r["ct_bytes"]
        pool_rate = pool_bytes / (statistics.median(r["ms"][names[3]]) * 1e-3)
        extra_us = r["ct_bytes"] / pool_rate * 1e6                      # 8 n 2k bytes per input ciphertext at pool_kernel's rate
        spread = max(max(v) - min(v) for v in (sq, fused, sep))
        bound = statistics.median(sq) + extra_us + spread
        fm, sm = statistics.median(fused), statistics.median(sep)
        default = "fused" if a.default == "fused" else "separate"
        dm = fm if default == "fused" else sm
        ok = dm <= bound
        verdicts.append(ok)
        L += ["", f"pool_kernel moved {pool_bytes / 2 ** 30:.2f} GiB at {pool_rate / 1e12:.2f} TB/s; reading one more ciphertext ({r['ct_bytes']} bytes) per input at that rate: {extra_us:.3f} us.",
              f"Gate: default tail ({default}) {dm:.3f} us <= Square + pooling {statistics.median(sq):.3f} + extra read {extra_us:.3f} + spread {spread:.3f} = {bound:.3f} us: "
              f"**{'met' if ok else 'NOT met'}**.  Fused {fm:.3f} us, separate {sm:.3f} us: the {'fused' if fm <= sm else 'separate'} tail is the faster one.",
              f"The two tails agree bit for bit: {r['tails_agree']}.", ""]
        st = stats.get((n, k))
        if st:
            tail = [(nm, v) for nm, v in st.items() if "poly2_tail_kernel" in nm]
            k3 = [(nm, v) for nm, v in st.items() if "relin_inv_crt" in nm]
            if tail:
                ns = tail[0][1][1]
                moved = (2 * r["cts_out"] + cnt) * r["ct_bytes"]
                L.append(f"`poly2_tail_kernel` (rocprofv3 --kernel-trace --stats, a run of its own): {ns / 1e3:.1f} us per call, {moved / 2 ** 30:.2f} GiB algorithmic "
                         f"(result rows read and written, every input row once) = {moved / ns / 1e3:.2f} TB/s = {moved / ns / 1e3 / HBM_TBS:.2f} of the {HBM_TBS:.0f} TB/s roofline.")
            for nm, (calls, ns) in k3:
                L.append(f"`{nm[:110]}`: {calls} calls, {ns / 1e3:.1f} us on average.")
            L.append("")
    if bench:
        L += ["## Whole network, `bench_host model=` at (8192, 3), batch 256, chunk 32", "", "| model | images/s |", "|---|---|"]
        L += [f"| {nm} | {v:.2f} |" for nm, v in bench.items()]
        L.append("")
    L += [f"command: python tools/measure_poly.py --rounds {a.rounds} --reps {a.reps}", ""]
    return "\n".join(L), all(verdicts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "poly_activation.md"))
    ap.add_argument("--default", default="fused", choices=("fused", "separate"), help="the tail the engine ships as its default (the gate is about that one)")
    ap.add_argument("--no-bench", action="store_true"); ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.mode == "step":
        return step(*a.shape, a.rounds, a.reps)
    if a.mode == "trace":
        return trace(*a.shape)
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, results, stats, bench = [], [], {}, None
    me = [sys.executable, os.path.abspath(__file__)]
    ok = True
    for n, k, B in SHAPES:
        out = run(me + ["step", str(n), str(k), str(B), "--rounds", str(a.rounds), "--reps", str(a.reps)], 300, log)
        if out is None:
            ok = False
            break
        results.append(json.loads(out.strip().splitlines()[-1]))
    if ok and not a.no_trace:
        for n, k, B in SHAPES:
            d = os.path.join(out_dir, f"trace_{n}_{k}")
            out = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["trace", str(n), str(k), str(B)], 300, log)
            if out is None:
                ok = False
                break
            stats[(n, k)] = kernel_stats(d)
    if ok and not a.no_bench:
        bench = bench_lines(out_dir, log)
        ok = bench is not None
    open(os.path.join(out_dir, "measure_poly.log"), "w").write("\n".join(log))
    if not results:
        print("\n".join(log)[-3000:])
        return 2
    text, met = report(results, stats, bench, a)
    print(text)
    if a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok and met else 1


if __name__ == "__main__":
    sys.exit(main())
