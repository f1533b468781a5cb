#!/usr/bin/env python3
"""Slot batching over several plain moduli priced on one MI355X -> profiles/slots_crt.md.

At (n, k) = (4096, 2) and (8192, 3), r = 2 and 3 twenty-bit slot primes, `--rows` plaintext rows per modulus, divisor 2^8:
(a) slots_crt_act_kernel (crc_slots_crt_act_dev) beside r crc_slots_rescale_dev calls on the same rows: the same transforms, the Garner fold and the residues on
    top.  The results differ by construction (the rescale divides every residue on its own), so only the times are compared.  us per row and modulus.
(b) slots_crt_decompose_kernel (crc_slots_crt_decompose_dev) beside r crc_slots_decompose_dev calls.  us per row and modulus.
(c) crc_slots_crt_refresh_dev_key beside its composition from the public calls (r crc_decrypt_dev, crc_slots_crt_act_dev, r crc_encrypt_dev_key_forms) on
    `--cts` NTT-form ciphertexts per modulus, NTT form out; the two results are compared bit for bit before anything is timed.  us per ciphertext and modulus.
HIP events around `--reps` calls, the compared calls alternating in one process, `--rounds` rounds after a warm-up call of each: median and min .. max.

One process per step, each under its own `timeout`, run one after the other and stopped at the first that fails:
    measure_slots_crt.py                 the driver
    measure_slots_crt.py step N K R      one parameter set and base, in process; prints one JSON line
Options: --rounds (7), --reps (20), --rows (1024), --cts (256), --markdown FILE."""
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

SETS = [(4096, 2), (8192, 3)]
BASES = [2, 3]
DIVISOR = 1 << 8
KEY = bytes(range(32))


def rounds_of(E, calls, rounds, reps):
    for fn in calls.values():
        fn()
    E.sync()
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    return ms


def step(n, k, r, rows, cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(n)[:k]
    ts = ca.SlotsCrt.primes(n, r, 20)
    B = ca.SlotsCrt([ca.Engine(n, q, t, device=0) for t in ts])
    E = B.E[0]
    rng = np.random.RandomState(2)
    d_p = [E.upload(rng.randint(0, t, size=(rows, n)).astype(np.uint64)) for t in ts]
    d_o = [E.alloc(rows * n * 8) for _ in ts]
    d_v = [E.alloc(rows * n * 8) for _ in ts]

    def rescales():
        for e, i, o in zip(B.E, d_p, d_o):
            e.slots_rescale_dev(i, rows, DIVISOR, o)

    def decomposes():
        for e, i, v in zip(B.E, d_p, d_v):
            e.slots_decompose_dev(i, rows, n, v, n, 1)
    res = dict(n=n, k=k, r=r, ts=ts, rows=rows)
    res["act"] = rounds_of(E, {"crt": lambda: B.act_dev(d_p, rows, DIVISOR, 1, 0, d_o), "single": rescales}, rounds, reps)
    res["decompose"] = rounds_of(E, {"crt": lambda: B.decompose_dev(d_p, rows, n, d_v[0], n, 1), "single": decomposes}, rounds, reps)
    # the refresh
    sk, pk = E.keygen(3)
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    ctb = 2 * k * n * 8
    d_ct, d_f, d_c, d_pl = [], [], [], []
    for j, e in enumerate(B.E):
        d = E.alloc(cts * ctb)
        e.encrypt_dev_forms(d_pk, d_p[j], cts, 5 + j, ca.NTT, d, E.alloc(e.encrypt_dev_work_bytes(cts)))
        d_ct.append(d); d_f.append(E.alloc(cts * ctb)); d_c.append(E.alloc(cts * ctb)); d_pl.append(E.alloc(cts * n * 8))
    d_w = E.alloc(max(B.refresh_dev_work_bytes(cts, ca.NTT), E.decrypt_dev_work_bytes(cts, 2, ca.NTT), E.encrypt_dev_work_bytes(cts)))

    def composed():
        for j, e in enumerate(B.E):
            e.decrypt_dev(d_sk, d_ct[j], cts, d_pl[j], d_w, in_form=ca.NTT)
        B.act_dev(d_pl, cts, DIVISOR, 1, 0, d_pl)
        for j, e in enumerate(B.E):
            e.encrypt_dev_key_forms(d_pk, d_pl[j], cts, KEY, 7 + j * cts, ca.NTT, d_c[j], d_w)
    fused = lambda: B.refresh_dev(d_sk, d_pk, d_ct, cts, DIVISOR, 1, 0, KEY, 7, d_f, d_w, in_form=ca.NTT, out_form=ca.NTT)
    fused(); composed()
    equal = all(bool(np.array_equal(E.download(a, (cts, 2, k, n)), E.download(b, (cts, 2, k, n)))) for a, b in zip(d_f, d_c))
    res["refresh"] = dict(cts=cts, equal=equal, ms=rounds_of(E, {"crt": fused, "single": composed}, rounds, reps))
    print(json.dumps(res), flush=True)
    return 0 if equal else 3


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_slots_crt] exit {p.returncode}: {' '.join(cmd[-8:])}", file=sys.stderr, flush=True)
    return p.stdout if p.returncode == 0 else None


def med_spread(vals, per):
    us = [1e3 * v / per for v in vals]
    return statistics.median(us), min(us), max(us)


def table(L, results, key, per, first, second):
    L += [f"| n | k | r | {first} | min .. max | {second} | min .. max | ratio |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        ms = r[key]["ms"] if "ms" in r[key] else r[key]
        m1, lo1, hi1 = med_spread(ms["crt"], per(r)); m2, lo2, hi2 = med_spread(ms["single"], per(r))
        L.append(f"| {r['n']} | {r['k']} | {r['r']} | {m1:.3f} | {lo1:.3f} .. {hi1:.3f} | {m2:.3f} | {lo2:.3f} .. {hi2:.3f} | {m1 / m2:.2f} |")
    L.append("")


def report(results, a):
    L = ["# Several plain moduli: the CRT activation, the CRT decompose and the refresh over a residue base", "",
         f"One MI355X.  HIP events around {a.reps} calls, the compared calls alternating in one process, {a.rounds} rounds after a warm-up call of each: median "
         "(min .. max).  Twenty-bit slot primes (crc_slots_crt_primes(n, r, 20)), divisor 2^8, ReLU on.", "",
         "## slots_crt_act_kernel beside r crc_slots_rescale_dev calls", "", f"{a.rows} rows per modulus; us per row and modulus.  The same transforms run in both; "
         "the CRT kernel adds the Garner fold and the r residues and launches once.", ""]
    table(L, results, "act", lambda r: r["rows"] * r["r"], "crc_slots_crt_act_dev", "r x crc_slots_rescale_dev")
    L += ["## slots_crt_decompose_kernel beside r crc_slots_decompose_dev calls", "", f"{a.rows} rows per modulus, all n slots, item-major; us per row and modulus.", ""]
    table(L, results, "decompose", lambda r: r["rows"] * r["r"], "crc_slots_crt_decompose_dev", "r x crc_slots_decompose_dev")
    L += ["## crc_slots_crt_refresh_dev_key beside its composition from the public calls", "",
          f"{a.cts} NTT-form ciphertexts per modulus in, NTT form out, public-key re-encryption; us per ciphertext and modulus.  Results equal bit for bit: "
          + ", ".join(str(r["refresh"]["equal"]) for r in results) + ".", ""]
    table(L, results, "refresh", lambda r: r["refresh"]["cts"] * r["r"], "fused", "composed")
    L += [f"command: python tools/measure_slots_crt.py --rounds {a.rounds} --reps {a.reps} --rows {a.rows} --cts {a.cts}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cts", type=int, default=256)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "slots_crt.md"))
    a = ap.parse_args()
    if a.mode == "step":
        return step(a.shape[0], a.shape[1], a.shape[2], a.rows, a.cts, a.rounds, a.reps)
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, results = [], []
    me = [sys.executable, os.path.abspath(__file__)]
    opts = ["--rounds", str(a.rounds), "--reps", str(a.reps), "--rows", str(a.rows), "--cts", str(a.cts)]
    ok = True
    for n, k in SETS:
        for r in BASES:
            out = run(me + ["step", str(n), str(k), str(r)] + opts, 240, log) if ok else None
            if out is None:
                ok = False
                break
            results.append(json.loads(out.strip().splitlines()[-1]))
    open(os.path.join(out_dir, "measure_slots_crt.log"), "w").write("\n".join(log))
    if not results:
        print("\n".join(log)[-3000:])
        return 2
    text = report(results, a)
    print(text)
    if ok and a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
