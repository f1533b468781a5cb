#!/usr/bin/env python3
"""Noise flooding priced on one MI355X -> profiles/flood.md.

(1) crc_flood_dev on `--cts` size-2 ciphertexts at (n, k) = (4096, 2) and (8192, 3), both forms: us per ciphertext, beside its composition from public calls --
    crc_encrypt_dev_forms of all-zero plaintexts into a second tensor, then crc_add -- and beside crc_encrypt_dev_forms alone, which is what a flood cannot beat
    by much (the same three transforms per modulus and the same sampling).
(2) the response of one PlainModelTiny image at (4096, 2): the smallest budget of the ten logits, after a flood of crc_flood_bits(a-priori budget, 40) bits and
    after the switch to one prime, and whether the logits decode to the same numbers.

HIP events around `--reps` calls, the compared calls alternating in one process, `--rounds` rounds: median and spread.  The flood is checked against its host twin
before anything is timed.  One process per step, each under its own `timeout`, stopped at the first that fails:
    measure_flood.py                  the driver
    measure_flood.py flood N K CTS    step (1) of one shape, in process; prints one JSON line
    measure_flood.py response         step (2)
Options: --rounds (7), --reps (10), --cts (1024), --markdown FILE."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from measure_mod_switch import alternate, cell, med, primes, random_cts  # noqa: E402

SHAPES = [(4096, 2), (8192, 3)]
T = 65537
NET_BUDGET = 42                 # the a-priori budget tests/test_gpu_flood_cpp.py floods PlainModelTiny's logits by


def flood_step(n, k, cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = primes(n, k)
    E = ca.Engine(n, q, T, device=0)
    _, pk = E.keygen(3)
    B = 64                       # admitted at both shapes; the work does not depend on the width
    x = random_cts(q, n, cts, 3)
    d_pk, d_x, d_z = E.upload(pk), E.upload(x), E.alloc(x.nbytes)
    d_zero = E.alloc(cts * n * 8); E.L.crc_memset(E.c, d_zero.ptr, 0, cts * n * 8, E.stream)
    d_w = E.alloc(max(E.flood_dev_work_bytes(cts, ca.NTT), E.encrypt_dev_work_bytes(cts)))
    head = min(cts, 4)
    equal = {}
    for name, form in (("coeff", ca.COEFF), ("ntt", ca.NTT)):
        d_t = E.upload(x)
        E.flood_dev(d_pk, d_t, cts, B, d_w, form=form, seed=9)
        equal[name] = bool(np.array_equal(E.download(d_t, x.shape)[:head], E.flood(pk, x[:head], B, form=form, seed=9)))
    calls = {}
    for name, form in (("coeff", ca.COEFF), ("ntt", ca.NTT)):
        # (in place on d_x: the values stop meaning anything after the first repetition, the work does not depend on them)
        calls["flood " + name] = lambda form=form: E.flood_dev(d_pk, d_x, cts, B, d_w, form=form, seed=9)

        def composition(form=form):
            E.encrypt_dev_forms(d_pk, d_zero, cts, 9, form, d_z, d_w); E.add(d_x, d_z, cts)
        calls["composition " + name] = composition
        calls["encrypt " + name] = lambda form=form: E.encrypt_dev_forms(d_pk, d_zero, cts, 9, form, d_z, d_w)
    ms = alternate(E, calls, rounds, reps)
    print(json.dumps(dict(n=n, k=k, cts=cts, flood_bits=B, equal=equal, ms=ms)), flush=True)
    return 0 if all(equal.values()) else 3


def response_step():
    import numpy as np
    import crcnn_amd as ca
    from crcnn_amd import synth
    from crcnn_amd.netrun import Network
    from netcommon import GOLD, load_net_golden
    g = load_net_golden("tiny4096")
    n, q, t = g["n"], g["q"], g["t"]
    A = ca.Engine(n, q, t, device=0); L = A.level(1)
    sk, pk = A.keygen(g["key_seed"])
    pl, _ = A.encode(synth.normalize(synth.synth_image(0)).reshape(-1))
    x = A.encrypt(pk, pl, g["enc_seed"]).reshape(1, 28 * 28, 2, A.k, n)
    net = Network(A, "PlainModelTiny", h5_path=os.path.join(GOLD, "models", "PlainModelTiny.h5"), resident=True, d_evk=A.upload(A.gen_evk(g["evk_seed"], sk)))
    net.prepare(1)
    d_out = net.forward(A.upload(x), 1)
    full = A.download(d_out, (10, 2, A.k, n))
    before = min(A.noise_budget(sk, c) for c in full)
    B = A.flood_bits(NET_BUDGET, 40)
    A.flood_dev(A.upload(pk), d_out, 10, B, A.alloc(A.flood_dev_work_bytes(10)), key=A.random_key(), stream_base=0)
    flooded = A.download(d_out, (10, 2, A.k, n))
    mid = min(A.noise_budget(sk, c) for c in flooded)
    d_low = A.alloc(10 * 2 * n * 8)
    A.mod_switch_dev(L, d_out, 10, d_low, A.alloc(A.mod_switch_work_bytes(L, 10)))
    low = L.download(d_low, (10, 2, 1, n)); skL = np.ascontiguousarray(sk[:1])
    after = min(L.noise_budget(skL, c) for c in low)
    la = [A.decode(p) for p in A.decrypt(sk, full)]; lb = [L.decode(p) for p in L.decrypt(skL, low)]
    print(json.dumps(dict(n=n, k=A.k, t=t, a_priori=NET_BUDGET, flood_bits=B, budget_before=before, budget_flooded=mid, budget_after=after,
                          bound=A.flood_budget_bound(before, B), logits_equal=la == lb)), flush=True)
    return 0


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_flood] exit {p.returncode}: {' '.join(cmd[-6:])}", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else None


def report(rows, resp, a):
    L = ["# Noise flooding: crc_flood_dev beside its composition from public calls, and the response of one image", "",
         f"One MI355X.  HIP events around {a.reps} calls, the compared calls alternating in one process, {a.rounds} rounds: median (min .. max), us per ciphertext.  "
         "The flood is checked against its host twin before anything is timed.  `composition` is crc_encrypt_dev_forms of all-zero plaintexts into a second tensor, "
         "then crc_add; `encrypt` is that crc_encrypt_dev_forms alone.", "",
         "| n | k | form | ciphertexts | flood bits | flood | composition | flood / composition | encrypt | equals the host twin |", "|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for r in rows:
        for form in ("coeff", "ntt"):
            c = r["cts"]
            mf, lf, hf = med(r["ms"]["flood " + form], c); mc, lc, hc = med(r["ms"]["composition " + form], c)
            L.append(f"| {r['n']} | {r['k']} | {form} | {c} | {r['flood_bits']} | {cell(r['ms']['flood ' + form], c)} | {cell(r['ms']['composition ' + form], c)} | "
                     f"{mf / mc:.2f} | {cell(r['ms']['encrypt ' + form], c)} | {r['equal'][form]} |")
            if mf > mc + max(hf - lf, hc - lc):
                slower.append(f"({r['n']}, {r['k']}) {form}")
    L += ["", ("**SLOWER than the composition by more than the measured spread at " + ", ".join(slower) + "**: the join kernel runs the generic LDS passes of "
               "ntt_device.h (one workgroup barrier per pass), the composition the wave-local row transform with its fused product; see DESIGN 4.27."
               if slower else "The flood is not slower than its composition at any measured shape."), "",
          "## The response of one PlainModelTiny image", ""]
    if resp is None:
        L += ["not measured (the step failed; see the log)", ""]
    else:
        L += [f"(n, k) = ({resp['n']}, {resp['k']}), t = {resp['t']}; ten logits; a-priori budget {resp['a_priori']} bits, flood_bits = crc_flood_bits(., 40) = {resp['flood_bits']}.", "",
              f"* smallest budget of the ten logits: {resp['budget_before']} bits as computed, {resp['budget_flooded']} after the flood (derived lower bound "
              f"{resp['bound']} less 2), {resp['budget_after']} after the switch to one prime",
              f"* logits decode to the same numbers: {resp['logits_equal']}", ""]
    L += [f"command: python tools/measure_flood.py --rounds {a.rounds} --reps {a.reps} --cts {a.cts}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--cts", type=int, default=1024)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "flood.md"))
    a = ap.parse_args()
    if a.mode == "flood":
        return flood_step(*a.shape[:3], a.rounds, a.reps)
    if a.mode == "response":
        return response_step()
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, rows, resp = [], [], None
    me = [sys.executable, os.path.abspath(__file__)]
    ok = True
    for n, k in SHAPES:
        r = run(me + ["flood", str(n), str(k), str(a.cts), "--rounds", str(a.rounds), "--reps", str(a.reps)], 240, log)
        if r is None:
            ok = False
            break
        rows.append(r)
    if ok:
        resp = run(me + ["response"], 240, log)
        ok = resp is not None
    open(os.path.join(out_dir, "measure_flood.log"), "w").write("\n".join(log))
    if not rows:
        print("\n".join(log)[-3000:])
        return 2
    text = report(rows, resp, a)
    print(text)
    if len(rows) == len(SHAPES) and a.markdown:          # (a failed response step is reported as not measured)
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if len(rows) == len(SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
