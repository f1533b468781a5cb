#!/usr/bin/env python3
"""The client-side activation priced on one MI355X -> profiles/slots_act.md.

(a) slots_act_kernel (crc_slots_act_dev) at a 2 x 2 / 2 and a 3 x 3 / 1 window, ReLU on, on `--planes` planes of 16 x 16 rows at n = 2048 .. 16384 (t =
    crc_slots_prime(n, 30), divisor 2^7) against its composition from the public calls that existed before it: crc_slots_decompose_dev of every input row, the
    window maximum and the ReLU on the int64 tensor (torch, same stream), crc_slots_compose_dev of the outputs and crc_slots_rescale_dev in place (ReLU commutes
    with the division).  Both results are compared with each other before anything is timed.  us per OUTPUT row.
(b) the new kernel at a 1 x 1 window without ReLU or cap against slots_rescale_kernel on the same rows: us per row.
(c) crc_slots_refresh_act_dev with a 2 x 2 / 2 window against crc_slots_refresh_dev on the same `--cts` NTT-form ciphertexts at (4096, 2): us per INPUT
    ciphertext.
HIP events around `--reps` calls, the compared calls alternating in one process, `--rounds` rounds: median and min .. max.

One process per step, each under its own `timeout`, run one after the other and stopped at the first that fails:
    measure_slots_act.py                 the driver
    measure_slots_act.py kernel N        one ring, in process; prints one JSON line
    measure_slots_act.py refresh         the refresh at (4096, 2), in process; prints one JSON line
Options: --rounds (7), --reps (20), --planes (16), --cts (2048), --markdown FILE."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from measure_slots_rescale import events_ms      # noqa: E402

RINGS = [2048, 4096, 8192, 16384]
DIVISOR = 1 << 7
SIDE = 16
WINDOWS = {"2x2/2": (SIDE, SIDE, 2, 2, 2, 2), "3x3/1": (SIDE, SIDE, 1, 1, 3, 3)}


def rounds_of(E, calls, rounds, reps):
    for fn in calls.values():
        fn()
    E.sync()
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    return ms


def kernel_step(n, planes, rounds, reps):
    import numpy as np
    import torch
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(n)[:1]
    t = ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    rows = planes * SIDE * SIDE
    p = np.random.RandomState(2).randint(0, t, size=(rows, n)).astype(np.uint64)
    d_p = E.upload(p)
    vals = torch.empty((planes, SIDE, SIDE, n), dtype=torch.int64, device="cuda")
    res = dict(n=n, t=t, planes=planes, rows=rows, windows={})
    ok = True
    for name, w in WINDOWS.items():
        xd, yd, xs, ys, xf, yf = w
        xo, yo = (xd - xf) // xs + 1, (yd - yf) // ys + 1
        outs = planes * xo * yo
        d_f, d_c = E.alloc(outs * n * 8), E.alloc(outs * n * 8)

        def composed():
            E.slots_decompose_dev(d_p, rows, n, vals, n, 1)
            m = vals[:, 0:xs * (xo - 1) + 1:xs, 0:ys * (yo - 1) + 1:ys]
            for a in range(xf):
                for b in range(yf):
                    if a or b:
                        m = torch.maximum(m, vals[:, a:a + xs * (xo - 1) + 1:xs, b:b + ys * (yo - 1) + 1:ys])
            m = torch.clamp_min(m, 0).contiguous()
            E.slots_compose_dev(m, outs, n, n, 1, d_c)
            E.slots_rescale_dev(d_c, outs, DIVISOR, d_c)
        fused = lambda: E.slots_act_dev(d_p, planes, w, DIVISOR, 1, 0, d_f)
        fused(); composed()
        equal = bool(np.array_equal(E.download(d_f, (outs, n)), E.download(d_c, (outs, n))))
        ok = ok and equal
        res["windows"][name] = dict(outs=outs, equal=equal, ms=rounds_of(E, {"fused": fused, "composed": composed}, rounds, reps))
    d_a, d_r = E.alloc(rows * n * 8), E.alloc(rows * n * 8)
    one = (SIDE, SIDE, 1, 1, 1, 1)
    calls = {"act 1x1": lambda: E.slots_act_dev(d_p, planes, one, DIVISOR, 0, 0, d_a), "rescale": lambda: E.slots_rescale_dev(d_p, rows, DIVISOR, d_r)}
    for fn in calls.values():
        fn()
    equal = bool(np.array_equal(E.download(d_a, (rows, n)), E.download(d_r, (rows, n))))
    res["one"] = dict(equal=equal, ms=rounds_of(E, calls, rounds, reps))
    print(json.dumps(res), flush=True)
    return 0 if ok and equal else 3


def refresh_step(cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    n, k = 4096, 2
    q = ca.default_coeff_modulus_128(n)[:k]
    t = ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    sk, pk = E.keygen(3)
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    planes = cts // (SIDE * SIDE)
    cts = planes * SIDE * SIDE
    w = WINDOWS["2x2/2"]
    d_pl = E.upload(np.random.RandomState(4).randint(0, t, size=(cts, n)).astype(np.uint64))
    d_ct, d_out = E.alloc(cts * 2 * k * n * 8), E.alloc(cts * 2 * k * n * 8)
    E.encrypt_dev_forms(d_pk, d_pl, cts, 5, ca.NTT, d_ct, E.alloc(E.encrypt_dev_work_bytes(cts)))
    d_w = E.alloc(max(E.slots_refresh_dev_work_bytes(cts, ca.NTT), E.slots_refresh_act_dev_work_bytes(planes, w, ca.NTT)))
    calls = {"crc_slots_refresh_act_dev 2x2/2": lambda: E.slots_refresh_act_dev(d_sk, d_pk, d_ct, planes, w, DIVISOR, 1, 0, 9, d_out, d_w, in_form=ca.NTT, out_form=ca.NTT),
             "crc_slots_refresh_dev": lambda: E.slots_refresh_dev(d_sk, d_pk, d_ct, cts, DIVISOR, 9, d_out, d_w, in_form=ca.NTT, out_form=ca.NTT)}
    print(json.dumps(dict(n=n, k=k, t=t, cts=cts, outs=cts // 4, ms=rounds_of(E, calls, rounds, reps))), flush=True)
    return 0


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_slots_act] exit {p.returncode}: {' '.join(cmd[-6:])}", file=sys.stderr, flush=True)
    return p.stdout if p.returncode == 0 else None


def med_spread(vals, per):
    us = [1e3 * v / per for v in vals]
    return statistics.median(us), min(us), max(us)


def report(kern, refresh, a):
    L = ["# The client-side activation: the fused window kernel against its composition, the 1 x 1 case against the rescale kernel, the whole refresh", "",
         f"One MI355X.  HIP events around {a.reps} calls, the compared calls alternating in one process, {a.rounds} rounds: median (min .. max).", "",
         "## slots_act_kernel against decompose + max / ReLU + compose + rescale", "",
         f"{a.planes} planes of {SIDE} x {SIDE} rows per call, t = crc_slots_prime(n, 30), divisor 2^7, ReLU on; us per output row.", "",
         "| n | window | fused | min .. max | composed | min .. max | ratio | results equal |", "|---|---|---|---|---|---|---|---|"]
    slower = []
    for r in kern:
        for name, wr in r["windows"].items():
            m1, lo1, hi1 = med_spread(wr["ms"]["fused"], wr["outs"]); m2, lo2, hi2 = med_spread(wr["ms"]["composed"], wr["outs"])
            L.append(f"| {r['n']} | {name} | {m1:.3f} | {lo1:.3f} .. {hi1:.3f} | {m2:.3f} | {lo2:.3f} .. {hi2:.3f} | {m1 / m2:.2f} | {wr['equal']} |")
            if m1 / m2 > 1.0:
                slower.append(f"{r['n']} ({name})")
    L += ["", ("**The fused kernel is slower than the composition (median ratio above 1.00) at n = " + ", ".join(slower) + "**." if slower
               else "The fused kernel is no slower than the composition (median ratio at most 1.00) at every n and window measured."), "",
          "## The 1 x 1 window without ReLU or cap against slots_rescale_kernel", "", "The same rows and divisor; us per row.", "",
          "| n | act 1 x 1 | min .. max | rescale | min .. max | ratio | beyond the spread | results equal |", "|---|---|---|---|---|---|---|---|"]
    beyond = []
    for r in kern:
        m1, lo1, hi1 = med_spread(r["one"]["ms"]["act 1x1"], r["rows"]); m2, lo2, hi2 = med_spread(r["one"]["ms"]["rescale"], r["rows"])
        b = m1 > m2 + max(hi1 - lo1, hi2 - lo2)
        if b:
            beyond.append(str(r["n"]))
        L.append(f"| {r['n']} | {m1:.3f} | {lo1:.3f} .. {hi1:.3f} | {m2:.3f} | {lo2:.3f} .. {hi2:.3f} | {m1 / m2:.2f} | {b} | {r['one']['equal']} |")
    L += ["", ("The new kernel is slower than slots_rescale_kernel beyond the run-to-run spread of either at n = " + ", ".join(beyond) + "." if beyond
               else "The new kernel is not slower than slots_rescale_kernel beyond the run-to-run spread of either at any n."), "",
          "## crc_slots_refresh_act_dev (2 x 2 / 2) against crc_slots_refresh_dev at (4096, 2)", ""]
    if refresh is None:
        L += ["not measured (the step failed; see the log)", ""]
    else:
        L += [f"{refresh['cts']} NTT-form ciphertexts in ({refresh['cts'] // (SIDE * SIDE)} planes of {SIDE} x {SIDE}), NTT form out, public-key re-encryption in both; the windowed "
              f"call re-encrypts {refresh['outs']}, the plain refresh all of them; us per input ciphertext.", "", "| call | us per input ciphertext | min .. max |", "|---|---|---|"]
        meds = []
        for nm, vs in refresh["ms"].items():
            m, lo, hi = med_spread(vs, refresh["cts"])
            meds.append(m)
            L.append(f"| {nm} | {m:.3f} | {lo:.3f} .. {hi:.3f} |")
        L += ["", f"ratio (windowed / plain): {meds[0] / meds[1]:.2f}", ""]
    L += [f"command: python tools/measure_slots_act.py --rounds {a.rounds} --reps {a.reps} --planes {a.planes} --cts {a.cts}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--cts", type=int, default=2048)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "slots_act.md"))
    a = ap.parse_args()
    if a.mode == "kernel":
        return kernel_step(a.shape[0], a.planes, a.rounds, a.reps)
    if a.mode == "refresh":
        return refresh_step(a.cts, a.rounds, a.reps)
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, kern, refresh = [], [], None
    me = [sys.executable, os.path.abspath(__file__)]
    opts = ["--rounds", str(a.rounds), "--reps", str(a.reps), "--planes", str(a.planes), "--cts", str(a.cts)]
    ok = True
    for n in RINGS:
        out = run(me + ["kernel", str(n)] + opts, 240, log)
        if out is None:
            ok = False
            break
        kern.append(json.loads(out.strip().splitlines()[-1]))
    if ok:
        out = run(me + ["refresh"] + opts, 240, log)
        ok = out is not None
        if ok:
            refresh = json.loads(out.strip().splitlines()[-1])
    open(os.path.join(out_dir, "measure_slots_act.log"), "w").write("\n".join(log))
    if not kern:
        print("\n".join(log)[-3000:])
        return 2
    text = report(kern, refresh, a)
    print(text)
    if ok and a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
