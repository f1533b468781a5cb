#!/usr/bin/env python3
"""Measure the dense layer over channel planes on one GPU and write profiles/dense_planes.md.

    python tools/measure_dense_planes.py [--out profiles/dense_planes.md] [--calls 3] [--rounds 3] [--sets 0,1] [--append]
    python tools/measure_dense_planes.py --trace N            # N batched calls of fc3 (lattice outputs, count = 1) at (4096, 2) and nothing else: the program to
                                                              # put behind `rocprofv3 --kernel-trace --stats`, a run of its own
    python tools/measure_dense_planes.py --k2-stats FILE       # (rocprofv3's .db or stats .csv) no GPU: the keyed K2's bytes per second from that run's kernel statistics, appended to --out

Per parameter set ((4096, 2 moduli), (8192, 3 moduli)) and count in (1, 16): HIP events around `calls` calls, the candidates alternating `rounds` times in ONE
process, median (min, max) per call.  NTT form in and out, dbc = 16, prepared keys given (crc_galois_prepare_keys_dev; its one-time cost is a column).
Shapes -- PlainModelTiny behind conv2 + pool2, 64 planes of 4 x 4 pixels at slots 4 (28 y + x):
  * fc3, 512 outputs on contiguous slots (M = 1024) and on the input lattice continued, output m at slot 4 m (M = 2048); the step counts are the planner's
  * fc4, Cin = 1: the 512 lattice outputs -> 10 outputs at slots 4 m
Candidates: crc_dense_planes_forms batched (planes_batch = 2) and step by step (planes_batch = 1); for the lattice layout of fc3 also the composition from the
entry points that existed before it: one crc_diag_mac_forms per plane (it rotates the INPUTS: the same number of elements, Cin times as many key switches, its
keys prepared by every call) and crc_add -- one call per round, it takes seconds.
Times do not depend on the values of keys or plaintext rows: the rows are device copies of one random block [Cin][k][n] and the key blobs device copies of ONE
generated key; the element lists are the real ones.
"""
import argparse
import csv
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_galois import fmt, timed  # noqa: E402

COUNTS = (1, 16)
LATTICE = [4 * (28 * y + x) for y in range(4) for x in range(4)]
HBM = 8.0e12                                                           # bytes per second: the roofline the keyed K2 is held against


def shapes(n):
    """{name: (Cin, plan)}"""
    from crcnn_amd.binding import dense_planes_plan
    lat = [4 * m for m in range(512)]
    return {"fc3 contiguous": (64, dense_planes_plan(n, 1024, LATTICE, 512)), "fc3 lattice": (64, dense_planes_plan(n, 2048, LATTICE, lat)),
            "fc4": (1, dense_planes_plan(n, 2048, lat, lat[:10]))}


def digits(E, dbc=16):
    return E.L.crc_evk_words(E.c, dbc) // (2 * E.k * E.n)


def k2_bytes(E, keyed, count, Cin, R):
    """what one call's keyed K2 launches move: per pass every prepared key once, and over the call the digit values and the sums of keyed x count ciphertexts
    once.  A pass is min(count, 1024 . 8 / (Cin + R)) ciphertexts per channel (square_chunk = 1024 at both parameter sets)"""
    D, n, k = digits(E), E.n, E.k
    ch = min(count, max(1, min(1024, 1024 * 8 // (Cin + R))))
    passes = -(-count // ch)
    return passes * keyed * E.galois_prepared_key_words() * 8 + keyed * count * D * 2 * n * 8 + keyed * count * 2 * k * 2 * n * 8


class Case:
    """device operands of one parameter set, sized for the largest shape"""
    def __init__(self, n, k, t, prepare_all=True):
        import crcnn_amd as ca
        self.ca = ca
        q = ca.binding.default_coeff_modulus_128(n)[:k]
        self.E = E = ca.Engine(n, q, t, device=0)
        self.H = H = ca.Engine(n, q, t, device=-1)
        self.n, self.k, self.q = n, k, q
        self.shapes = shapes(n)
        sk, _ = H.keygen(1)
        self.all_elts = sorted({e for _, p in self.shapes.values() for e in p.elements} - {1})
        _, one = H.gen_galois_keys(2, sk, elts=[self.all_elts[0]])
        self.kb = one.nbytes
        ne = len(self.all_elts)
        self.d_cg = E.alloc(self.kb * ne)
        d_one = E.upload(one)
        for e in range(ne):
            E.copy_d2d(self.d_cg.ptr + e * self.kb, d_one, self.kb)
        self.d_pk = E.alloc(ne * E.galois_prepared_key_words() * 8)
        if prepare_all:
            self.prep_ms = timed(E, lambda: E.galois_prepare_keys(self.d_cg, self.all_elts, d_pk=self.d_pk), 1)
        else:                                                           # (--trace: one preparation, so that its kernels stay out of the call's statistics)
            E.galois_prepare_keys(self.d_cg, self.all_elts[:1], d_pk=self.d_pk)
            pkb = E.galois_prepared_key_words() * 8
            for e in range(1, ne):
                E.copy_d2d(self.d_pk.ptr + e * pkb, self.d_pk, pkb)
        self.cmax = max(COUNTS)
        rng = np.random.RandomState(n)
        cin = max(c for c, _ in self.shapes.values())
        x = np.stack([(rng.randint(0, 1 << 62, size=(cin * self.cmax, 2, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=2)
        self.d_x = E.upload(x)
        self.rowb = k * n * 8; self.ctb = 2 * self.rowb
        self.d_y = E.alloc(self.cmax * self.ctb)
        self.block = np.stack([(rng.randint(0, 1 << 62, size=(cin, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=1)
        self.d_rows = {}

    def rows(self, name):
        """[R][Cin][k][n] NTT-form rows of the shape: copies of the random block"""
        if name not in self.d_rows:
            Cin, plan = self.shapes[name]
            d_b = self.E.upload(self.block[:Cin])
            d = self.E.alloc(len(plan.steps) * Cin * self.rowb)
            for j in range(len(plan.steps)):
                self.E.copy_d2d(d.ptr + j * Cin * self.rowb, d_b, Cin * self.rowb)
            self.d_rows[name] = d
        return self.d_rows[name]

    def fused(self, name, count, d_work):
        Cin, plan = self.shapes[name]
        d_p = self.rows(name)
        return lambda: self.E.dense_planes(self.d_x, count, Cin, plan.elements, d_p, self.d_cg, self.all_elts, self.d_y, d_work, d_pk=self.d_pk,
                                           in_form=self.ca.NTT, out_form=self.ca.NTT)


def alternate(E, cands, rounds):
    """{name: [ms per round]}; a candidate is (planes_batch, calls, function).  The key is set outside the timed region (set_tuning synchronises)"""
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (batch, calls, fn) in cands.items():
            E.set_tuning("planes_batch", batch)
            out[k].append(timed(E, fn, calls))
            E.set_tuning("planes_batch", 0)
    return out


def measure(n, k, t, calls, rounds):
    C = Case(n, k, t)
    E, ca = C.E, C.ca
    need = [E.dense_planes_work_bytes(C.cmax, Cin, len(p.steps), prepared=True) for Cin, p in C.shapes.values()]
    need.append(E.diag_mac_work_bytes(C.cmax, len(C.shapes["fc3 lattice"][1].steps)))
    d_work = E.alloc(max(need))
    d_tmp = E.alloc(C.cmax * C.ctb)
    pkb = E.galois_prepared_key_words() * 8
    lines = [f"## n = {n}, {k} moduli (one conjugated key: {C.kb} bytes, prepared: {pkb} bytes; preparing all {len(C.all_elts)} keys of the three shapes once: "
             f"{C.prep_ms:.3f} ms)", "",
             "| shape | Cin | steps R | count | keys: conjugated, prepared bytes | rows bytes | batched (planes_batch = 2) | step by step (planes_batch = 1) | batched / step by step | "
             "one crc_diag_mac_forms per plane + crc_add | keyed K2 bytes per call |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, (Cin, plan) in C.shapes.items():
        R = len(plan.steps)
        for count in COUNTS:
            cands = {"batched": (2, calls, C.fused(name, count, d_work)), "steps": (1, calls, C.fused(name, count, d_work))}
            if name == "fc3 lattice":
                # rotating the inputs takes an element per difference (out - in) mod M -- as many as there are steps; the times do not depend on which, so the
                # steps' own elements (whose key blobs are there) stand in for them: one row per element, Cin calls, Cin - 1 adds
                gs = plan.elements
                d_p = C.rows(name)

                def composed(gs=gs, d_p=d_p, count=count, Cin=Cin):
                    for c in range(Cin):
                        dst = C.d_y if c == 0 else d_tmp
                        E.diag_mac(C.d_x.ptr + c * count * C.ctb, count, gs, d_p.ptr + c * R * C.rowb, C.d_cg, C.all_elts, dst, d_work, in_form=ca.NTT, out_form=ca.NTT)
                        if c:
                            E.add(C.d_y, d_tmp, count)
                cands["composed"] = (0, 1, composed)
            r = alternate(E, cands, rounds)
            med = {k_: statistics.median(v) for k_, v in r.items()}
            keyed = R - (1 if 0 in plan.steps else 0)
            lines.append(f"| {name} | {Cin} | {R} | {count} | {keyed * C.kb}, {keyed * pkb} | {R * Cin * C.rowb} | {fmt(r['batched'])} | {fmt(r['steps'])} | "
                         f"{med['batched'] / med['steps']:.3f} | {fmt(r['composed']) if 'composed' in r else ''} | {k2_bytes(E, keyed, count, Cin, R)} |")
            print(lines[-1], flush=True)
    E.close(); C.H.close()
    return lines + [""]


def trace(calls):
    C = Case(4096, 2, 65537, prepare_all=False)
    name = "fc3 lattice"
    Cin, plan = C.shapes[name]
    d_work = C.E.alloc(C.E.dense_planes_work_bytes(1, Cin, len(plan.steps), prepared=True))
    fn = C.fused(name, 1, d_work)
    C.E.set_tuning("planes_batch", 2)
    for _ in range(calls + 1):
        fn()
    C.E.sync()
    C.E.set_tuning("planes_batch", 0)
    keyed = len(plan.steps) - (1 if 0 in plan.steps else 0)
    print(f"trace: {calls + 1} calls of {name} at count 1, {keyed} keyed steps, keyed K2 bytes per call {k2_bytes(C.E, keyed, 1, Cin, len(plan.steps))}", flush=True)
    C.E.close(); C.H.close()


def k2_stats(path, out):
    """the keyed K2's rows of a rocprofv3 kernel-statistics file against the bytes of --trace's shape: no GPU needed"""
    import crcnn_amd as ca
    E = ca.Engine(4096, ca.binding.default_coeff_modulus_128(4096)[:2], 65537, device=-1)
    plan = shapes(4096)["fc3 lattice"][1]
    keyed = len(plan.steps) - 1
    per_call = k2_bytes(E, keyed, 1, 64, len(plan.steps))
    if path.endswith(".db"):                                            # rocprofv3's database output: the view top_kernels, microseconds
        import sqlite3
        stats = [(str(r[0]), int(r[1]), float(r[2]) * 1e3) for r in sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels")]
    else:                                                               # its CSV kernel statistics
        stats = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path)) if r.get("Name")]
    launches = sum(n_ for name, n_, _ in stats if "relin_mac_keyed" in name)
    total_ns = sum(ns for name, _, ns in stats if "relin_mac_keyed" in name)
    if not launches:
        raise SystemExit("no relin_mac_keyed kernel in " + path)
    sub = -(-keyed // 1024)                                              # launches per call: square_chunk = 1024 steps of one ciphertext each
    calls = launches / sub
    bps = per_call * calls / (total_ns * 1e-9)
    text = ["## The keyed K2 against the HBM roofline", "",
            f"rocprofv3 --kernel-trace --stats around `--trace` (fc3 lattice, count = 1, (4096, 2)): {launches} launches of relin_mac_keyed_f64_kernel in {calls:.0f} calls, "
            f"{total_ns / launches / 1e3:.1f} us per launch.  A call's launches read {keyed} prepared keys once each, the digit values once and write the sums once: "
            f"{per_call} bytes, i.e. {bps / 1e12:.2f} TB/s achieved, {100 * bps / HBM:.0f} % of the 8 TB/s HBM roofline (the kernel is bound by bytes: 7 flops per "
            "8-byte key value).", "",
            "## Every kernel of that run", "",
            f"The same statistics file, every kernel, launches and time divided by the {calls:.0f} calls.  The run's set-up launches three kernels once (it prepares "
            "ONE key and copies the blob to the other slots): the two the entry point never launches are marked, the third is one inverse transform more among "
            "the call's.  Share: of the kernel time of the call's own kernels.", "",
            "| kernel | launches per call | us per call | share |", "|---|---|---|---|"]
    short = lambda name: name.split("(")[0].split("<")[0].replace("void ", "").strip()
    own = [s for s in stats if s[1] >= calls and not s[0].startswith("__amd_rocclr")]       # (the runtime's copy kernels: the set-up's device copies)
    own_ns = sum(ns for _, _, ns in own)
    for name, n_, ns in sorted(own, key=lambda s: -s[2]):
        text.append(f"| {short(name)} | {n_ // round(calls)} | {ns / calls / 1e3:.1f} | {ns / own_ns:.2f} |")
    text.append(f"| all of a call | {sum(n_ // round(calls) for _, n_, _ in own)} | {own_ns / calls / 1e3:.1f} | 1.00 |")
    for name, n_, ns in sorted((s for s in stats if s not in own), key=lambda s: -s[2]):
        text.append(f"| (set-up, {n_} in the run) {short(name)} |  | {ns / 1e3:.1f} in the run |  |")
    text.append("")
    with open(out, "a") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    E.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_planes.md"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="0,1")
    ap.add_argument("--append", action="store_true", help="add the chosen sets' tables to an existing file (a run per parameter set)")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--k2-stats", default="")
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace)
    if a.k2_stats:
        return k2_stats(a.k2_stats, a.out)
    import crcnn_amd as ca
    out = [] if a.append else [
        "# Dense layer over channel planes: measurements", "",
        f"tools/measure_dense_planes.py on one GPU: HIP events around {a.calls} calls, candidates alternating {a.rounds} times in one process, median (min, max) per "
        "call.  NTT form in and out, dbc = 16, prepared keys given.  PlainModelTiny's fc3 behind conv2 + pool2 (64 planes of 4 x 4 pixels at slots 4 (28 y + x) -> 512 "
        "outputs, on contiguous slots and on the input lattice continued) and fc4 (Cin = 1, 512 -> 10).  `batched`: the keyed steps of a pass in sub-batches through "
        "relin_mac_keyed_f64_kernel; `step by step`: one key switch per step, as crc_diag_mac_bsgs_forms' giant stage; the composition (lattice layout only, one "
        "call per round): one crc_diag_mac_forms per plane, which rotates the inputs, and crc_add.  Key blobs are device copies of one generated key and the rows "
        "copies of one random block: times do not depend on their values.", ""]
    sets = ((4096, 2, 65537), (8192, 3, ca.Engine.slots_prime(8192, 30)))
    for i in (int(v) for v in a.sets.split(",")):
        out += measure(*sets[i], a.calls, a.rounds)
    text = "\n".join(out)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
