#!/usr/bin/env python3
"""Modulus switching priced on one MI355X -> profiles/mod_switch.md.

(1) the coefficient kernel (COEFF -> COEFF) on `--cts` size-2 ciphertexts at (n, k -> k') = (4096, 3 -> 2), (4096, 2 -> 1), (8192, 3 -> 2), (16384, 4 -> 3): us per
    ciphertext and achieved bytes/s over the algorithmic bytes 2 (k + k') n 8 per ciphertext, beside crc_add (an existing bandwidth-bound kernel: 3 tensors of
    traffic) on as many ciphertexts of the upper level as move the same bytes.  Recorded, not gated.
(2) the fused NTT -> NTT call against its composition from public calls -- crc_ntt_inv on the upper level, the coefficient kernel, crc_ntt_fwd on the lower -- at
    the same shapes; by transform count the fused call should take about (d + k') / (k + k') of the composition.
(3) what the lower level buys: crc_square_relin_forms and one crc_rotate_rows_forms step per ciphertext (NTT form in and out) at (8192, 3) against (8192, 2) and
    at (4096, 2) against (4096, 1), with the switch's own cost beside them.
(4) the response of one PlainModelTiny image at (4096, 2): bytes before and after 2 -> 1, the smallest budget of the ten logits on either side, and whether the
    logits decode to the same numbers.

HIP events around `--reps` calls, the compared calls alternating in one process, `--rounds` rounds: median and spread.  Outputs are checked equal (device against
the host twin, fused against composition) before anything is timed.  One process per step, each under its own `timeout`, stopped at the first that fails:
    measure_mod_switch.py                      the driver
    measure_mod_switch.py switch N K KEPT CTS  steps (1) and (2) of one shape, in process; prints one JSON line
    measure_mod_switch.py lower N K CTS        step (3) of one pair of levels
    measure_mod_switch.py response             step (4)
Options: --rounds (7), --reps (10), --cts (1024), --lower-cts (256), --markdown FILE."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = [(4096, 3, 2), (4096, 2, 1), (8192, 3, 2), (16384, 4, 3)]
LOWER = [(8192, 3), (4096, 2)]
T = 65537


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


def primes(n, k):
    import crcnn_amd as ca
    out = []
    for m in (n, 8192, 16384):
        if m >= n:
            out += [p for p in ca.default_coeff_modulus_128(m) if p not in out]
    return out[:k]


def alternate(E, calls, rounds, reps):
    for fn in calls.values():
        fn()
    E.sync()
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    return ms


def random_cts(q, n, cts, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    x = np.zeros((cts, 2, len(q), n), dtype=np.uint64)
    for i, qi in enumerate(q):
        x[:, :, i, :] = (rng.randint(0, 1 << 62, size=(cts, 2, n), dtype=np.int64) % qi).astype(np.uint64)
    return x


def switch_step(n, k, kept, cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = primes(n, k)
    A = ca.Engine(n, q, T, device=0); B = A.level(kept)
    x = random_cts(q, n, cts, 3)
    d_x, d_o, d_c = A.upload(x), A.alloc(cts * 2 * kept * n * 8), A.alloc(cts * 2 * kept * n * 8)
    d_w = A.alloc(max(A.mod_switch_work_bytes(B, cts, in_form=f, out_form=g) for f in (0, 1) for g in (0, 1)))
    head = min(cts, 4)
    A.mod_switch_dev(B, d_x, cts, d_o, d_w)
    eq_coeff = bool(np.array_equal(A.download(d_o, (cts, 2, kept, n))[:head], A.mod_switch(B, x[:head])))
    # the composition, on a copy (crc_ntt_inv works in place)
    d_t = A.upload(x)
    A.ntt_inv(d_t, cts); A.mod_switch_dev(B, d_t, cts, d_c, d_w); B.ntt_fwd(d_c, cts)
    A.mod_switch_dev(B, d_x, cts, d_o, d_w, in_form=ca.NTT, out_form=ca.NTT)
    fused = A.download(d_o, (cts, 2, kept, n))
    eq_fused = bool(np.array_equal(fused, A.download(d_c, (cts, 2, kept, n))) and np.array_equal(fused[:head], A.mod_switch(B, x[:head], in_form=ca.NTT, out_form=ca.NTT)))
    # crc_add on as many upper-level ciphertexts as move the coefficient kernel's bytes: 3 tensors of 2 k n 8 bytes each against 2 (k + k') n 8
    add_cts = max(1, round(cts * (k + kept) / (3 * k)))
    d_a, d_b = A.upload(x[:add_cts]), A.upload(x[:add_cts])

    def composition():                     # (in place on d_t: the values stop meaning anything after the first repetition, the work does not depend on them)
        A.ntt_inv(d_t, cts); A.mod_switch_dev(B, d_t, cts, d_c, d_w); B.ntt_fwd(d_c, cts)
    ms = alternate(A, {"coeff": lambda: A.mod_switch_dev(B, d_x, cts, d_o, d_w), "crc_add": lambda: A.add(d_a, d_b, add_cts),
                       "fused": lambda: A.mod_switch_dev(B, d_x, cts, d_o, d_w, in_form=ca.NTT, out_form=ca.NTT), "composition": composition}, rounds, reps)
    print(json.dumps(dict(n=n, k=k, kept=kept, cts=cts, add_cts=add_cts, equal_coeff=eq_coeff, equal_fused=eq_fused, ms=ms)), flush=True)
    return 0 if eq_coeff and eq_fused else 3


def lower_step(n, k, cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = primes(n, k)
    t = ca.Engine.slots_prime(n, 20)
    A = ca.Engine(n, q, t, device=0); B = A.level(k - 1)
    sk, pk = A.keygen(3)
    levels = {}
    rng = np.random.RandomState(4)
    plains = rng.randint(0, t, size=(cts, n)).astype(np.uint64)
    for nm, E, s in (("upper", A, sk), ("lower", B, np.ascontiguousarray(sk[:k - 1]))):
        elt = E.galois_elt_rows(1)
        elts, gk = E.gen_galois_keys(6, s, 16, [elt])
        d_ct = E.alloc(cts * 2 * E.k * n * 8)
        pkl = np.ascontiguousarray(pk[:, :E.k])
        E.encrypt_dev_forms(E.upload(pkl), E.upload(plains), cts, 5, ca.NTT, d_ct, E.alloc(E.encrypt_dev_work_bytes(cts)))
        levels[nm] = dict(E=E, d_ct=d_ct, d_y=E.alloc(cts * 2 * E.k * n * 8), d_evk=E.upload(E.gen_evk(7, s)), d_gk=E.upload(gk), elts=elts,
                          d_w=E.alloc(max(E.square_relin_work_bytes(cts), E.apply_galois_work_bytes(cts))))
    U, Lo = levels["upper"], levels["lower"]
    d_o, d_w = A.alloc(cts * 2 * (k - 1) * n * 8), A.alloc(max(A.mod_switch_work_bytes(B, cts, in_form=ca.NTT, out_form=g) for g in (ca.COEFF, ca.NTT)))
    # the switched tensor decrypts like the upper one before anything is timed
    A.mod_switch_dev(B, U["d_ct"], cts, d_o, d_w, in_form=ca.NTT, out_form=ca.COEFF)
    head = min(cts, 4)
    equal = bool(np.array_equal(B.decrypt(np.ascontiguousarray(sk[:k - 1]), B.download(d_o, (cts, 2, k - 1, n))[:head]), plains[:head]))

    def sq(L):
        return lambda: L["E"].square_relin(L["d_ct"], cts, L["d_evk"], L["d_y"], L["d_w"], 16, ca.NTT, ca.NTT)

    def rot(L):
        return lambda: L["E"].rotate_rows(L["d_ct"], cts, 1, L["d_gk"], L["elts"], L["d_y"], L["d_w"], 16, ca.NTT, ca.NTT)
    ms = alternate(A, {"square_relin upper": sq(U), "square_relin lower": sq(Lo), "rotate_rows upper": rot(U), "rotate_rows lower": rot(Lo),
                       "switch": lambda: A.mod_switch_dev(B, U["d_ct"], cts, d_o, d_w, in_form=ca.NTT, out_form=ca.NTT)}, rounds, reps)
    print(json.dumps(dict(n=n, k=k, cts=cts, equal_decrypt=equal, ms=ms)), flush=True)
    return 0 if equal else 3


def response_step():
    import numpy as np
    import crcnn_amd as ca
    from crcnn_amd import synth
    from crcnn_amd.netrun import Network
    from netcommon import GOLD, load_net_golden
    g = load_net_golden("tiny4096")
    n, q, t = g["n"], g["q"], g["t"]
    A = ca.Engine(n, q, t, device=0); B = A.level(1)
    sk, pk = A.keygen(g["key_seed"])
    pl, _ = A.encode(synth.normalize(synth.synth_image(0)).reshape(-1))
    x = A.encrypt(pk, pl, g["enc_seed"]).reshape(1, 28 * 28, 2, A.k, n)
    net = Network(A, "PlainModelTiny", h5_path=os.path.join(GOLD, "models", "PlainModelTiny.h5"), resident=True, d_evk=A.upload(A.gen_evk(g["evk_seed"], sk)))
    net.prepare(1)
    d_out = net.forward(A.upload(x), 1)
    d_low = A.alloc(10 * 2 * n * 8)
    A.mod_switch_dev(B, d_out, 10, d_low, A.alloc(A.mod_switch_work_bytes(B, 10)))
    skB = np.ascontiguousarray(sk[:1])
    d_bits = A.alloc(40)
    A.noise_budget_dev(A.upload(sk), d_out, 10, d_bits, A.alloc(A.noise_budget_dev_work_bytes(10)))
    before = [int(v) for v in A.download(d_bits, (10,), dtype=np.int32)]
    B.noise_budget_dev(B.upload(skB), d_low, 10, d_bits, B.alloc(B.noise_budget_dev_work_bytes(10)))
    after = [int(v) for v in B.download(d_bits, (10,), dtype=np.int32)]
    full, low = A.download(d_out, (10, 2, A.k, n)), B.download(d_low, (10, 2, 1, n))
    la = [A.decode(p) for p in A.decrypt(sk, full)]; lb = [B.decode(p) for p in B.decrypt(skB, low)]
    print(json.dumps(dict(n=n, k=A.k, t=t, bytes_before=int(full.nbytes), bytes_after=int(low.nbytes), wire_before=10 * A.L.crc_seal_ct_bytes(A.c, 2),
                          wire_after=10 * B.L.crc_seal_ct_bytes(B.c, 2), budget_before=min(before), budget_after=min(after), logits_equal=la == lb,
                          argmax=int(np.argmax(lb)), golden_argmax=int(np.argmax(g["logits"])))), flush=True)
    return 0 if la == lb else 3


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_mod_switch] exit {p.returncode}: {' '.join(cmd[-7:])}", file=sys.stderr, flush=True)
    return json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else None


def med(vals, per):
    us = [1e3 * v / per for v in vals]
    return statistics.median(us), min(us), max(us)


def cell(vals, per):
    m, lo, hi = med(vals, per)
    return f"{m:.3f} ({lo:.3f} .. {hi:.3f})"


def report(sw, lower, resp, a):
    L = ["# Modulus switching: the coefficient kernel, the fused NTT-form call, what a lower level buys, and the response", "",
         f"One MI355X.  HIP events around {a.reps} calls, the compared calls alternating in one process, {a.rounds} rounds: median (min .. max).  Every step checks its "
         "outputs (device against the host twin, fused against composition, decryption across levels) before it times anything.", "",
         "## 1. modswitch_coeff_kernel beside crc_add", "",
         "us per ciphertext (size 2); bytes/s over the algorithmic bytes 2 (k + k') n 8 per ciphertext; crc_add on as many upper-level ciphertexts as move the same bytes "
         "(three tensors of traffic).  Recorded, not gated.", "",
         "| n | k -> k' | ciphertexts | switch us/ct | switch TB/s | crc_add cts | crc_add TB/s | equals the host twin |", "|---|---|---|---|---|---|---|---|"]
    for r in sw:
        n, k, kp, cts = r["n"], r["k"], r["kept"], r["cts"]
        m, _, _ = med(r["ms"]["coeff"], cts); ma, _, _ = med(r["ms"]["crc_add"], 1)
        bts = 2 * (k + kp) * n * 8
        L.append(f"| {n} | {k} -> {kp} | {cts} | {cell(r['ms']['coeff'], cts)} | {bts / m / 1e6:.2f} | {r['add_cts']} | {3 * 2 * k * n * 8 * r['add_cts'] / ma / 1e6:.2f} | {r['equal_coeff']} |")
    L += ["", "## 2. The fused NTT -> NTT call against crc_ntt_inv + coefficient kernel + crc_ntt_fwd", "",
          "us per ciphertext; `expected` is (d + k') / (k + k'), the ratio of row transforms.", "",
          "| n | k -> k' | fused | composition | ratio | expected | equal |", "|---|---|---|---|---|---|---|"]
    losers = []
    for r in sw:
        n, k, kp, cts = r["n"], r["k"], r["kept"], r["cts"]
        mf, lf, hf = med(r["ms"]["fused"], cts); mc, lc, hc = med(r["ms"]["composition"], cts)
        L.append(f"| {n} | {k} -> {kp} | {cell(r['ms']['fused'], cts)} | {cell(r['ms']['composition'], cts)} | {mf / mc:.2f} | {k / (k + kp):.2f} | {r['equal_fused']} |")
        if mf > mc + max(hf - lf, hc - lc):
            losers.append((n, k, kp))
    L += ["", ("**The fused call is slower than the composition by more than the measured spread at " + ", ".join(f"({n}, {k} -> {kp})" for n, k, kp in losers) + "**."
               if losers else "The fused call is not slower than the composition at any shape: it is what crc_mod_switch_forms does for NTT -> NTT."), ""]
    L += ["## 3. What the lower level buys", "", "us per ciphertext, NTT form in and out, dbc 16; `switch` is the NTT -> NTT switch from the upper to the lower level.", "",
          "| n | k -> k - 1 | ciphertexts | square_relin upper | lower | rotate_rows upper | lower | switch | switch / (saved per square) | switch / (saved per rotation) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in lower:
        c = r["cts"]; m = {nm: med(v, c)[0] for nm, v in r["ms"].items()}
        ds, dr = m["square_relin upper"] - m["square_relin lower"], m["rotate_rows upper"] - m["rotate_rows lower"]
        L.append(f"| {r['n']} | {r['k']} -> {r['k'] - 1} | {c} | {cell(r['ms']['square_relin upper'], c)} | {cell(r['ms']['square_relin lower'], c)} | "
                 f"{cell(r['ms']['rotate_rows upper'], c)} | {cell(r['ms']['rotate_rows lower'], c)} | {cell(r['ms']['switch'], c)} | "
                 f"{m['switch'] / ds if ds > 0 else float('inf'):.2f} | {m['switch'] / dr if dr > 0 else float('inf'):.2f} |")
    L += ["", "The last two columns: after how many downstream operations of that kind the switch has paid for itself.", ""]
    L += ["## 4. The response of one PlainModelTiny image", ""]
    if resp is None:
        L += ["not measured (the step failed; see the log)", ""]
    else:
        L += [f"(n, k) = ({resp['n']}, {resp['k']}), t = {resp['t']}; ten logits.", "",
              f"* residue bytes: {resp['bytes_before']} before, {resp['bytes_after']} after 2 -> 1; in SEAL's wire format {resp['wire_before']} and {resp['wire_after']}",
              f"* smallest budget of the ten logits: {resp['budget_before']} bits before, {resp['budget_after']} after",
              f"* logits decode to the same numbers: {resp['logits_equal']} (argmax {resp['argmax']}, the golden run's {resp['golden_argmax']})", ""]
    L += [f"command: python tools/measure_mod_switch.py --rounds {a.rounds} --reps {a.reps} --cts {a.cts} --lower-cts {a.lower_cts}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--cts", type=int, default=1024)
    ap.add_argument("--lower-cts", type=int, default=256)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "mod_switch.md"))
    a = ap.parse_args()
    if a.mode == "switch":
        return switch_step(*a.shape[:4], a.rounds, a.reps)
    if a.mode == "lower":
        return lower_step(*a.shape[:3], a.rounds, a.reps)
    if a.mode == "response":
        return response_step()
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, sw, lower, resp = [], [], [], None
    me = [sys.executable, os.path.abspath(__file__)]
    opts = ["--rounds", str(a.rounds), "--reps", str(a.reps)]
    ok = True
    for n, k, kept in SHAPES:
        r = run(me + ["switch", str(n), str(k), str(kept), str(a.cts)] + opts, 240, log)
        if r is None:
            ok = False
            break
        sw.append(r)
    for n, k in LOWER if ok else []:
        r = run(me + ["lower", str(n), str(k), str(a.lower_cts)] + opts, 300, log)
        if r is None:
            ok = False
            break
        lower.append(r)
    if ok:
        resp = run(me + ["response"], 240, log)
        ok = resp is not None
    open(os.path.join(out_dir, "measure_mod_switch.log"), "w").write("\n".join(log))
    if not sw:
        print("\n".join(log)[-3000:])
        return 2
    text = report(sw, lower, resp, a)
    print(text)
    if ok and a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
