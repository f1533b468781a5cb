#!/usr/bin/env python3
"""Slot batching priced on one MI355X -> profiles/slot_batching.md.

(a) crc_slots_compose_dev / crc_slots_decompose_dev at (n, k) = (2048, 1), (4096, 2), (8192, 3), t = crc_slots_prime(n, 30), `--rows` rows of n slots per call, in the
    item-major (slots, 1) and the image-major (1, rows) layout: HIP events around `--reps` calls, the calls alternating in one process, `--rounds` rounds, median and
    spread in us per row; beside them crc_ntt_inv / crc_ntt_fwd of the same build on as many rows of ONE coefficient modulus of the same ring (the row transform
    the kernels are made of), and the host twins crc_slots_compose / crc_slots_decompose on the host's threads (wall clock).  No ratio is fixed in advance.  Where
    compose costs more than the row transform plus what an 8-byte-granular gather of the row can explain -- every value read drags a 64-byte sector in, so a
    strided row moves up to 64 n bytes instead of 8 n; at the HBM rate the row transform itself reaches that is up to 8 x its read time -- the report says so.
(b) End to end, PlainModelTiny quantised at (--input-bits, --weight-bits) on (4096, 2): the exact integer network (tests/slots_model.py, Python integers, no
    modulus) on --images synthetic images gives the largest logit; the smallest `bits` whose crc_slots_prime(4096, bits) exceeds twice that is the smallest plain
    modulus that carries the logits without wrap-around.  `test_host slots_build` runs the network there: the decoded logits must equal the integer model's, and
    the report gives the noise budget left (minNoiseBudget), milliseconds per tensor evaluation and images/s = slots x evaluations/s.  If the budget is 0 at that
    t, no plain modulus carries the network at these parameters and the report says so.

One process per step, each under its own `timeout`, run one after the other and stopped at the first that fails:
    measure_slots.py                 the driver
    measure_slots.py step N K ROWS   one ring, in process; prints one JSON line
Options: --rounds (5), --reps (20), --rows (4096), --images (8), --input-bits (4), --weight-bits (5), --markdown FILE."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = [(2048, 1), (4096, 2), (8192, 3)]


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


def step(n, k, rows, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(n)[:k]
    t = ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    E1 = ca.Engine(n, q[:1], t, device=0)                      # rows of one modulus: a size-2 ciphertext of k = 1 is two rows
    H = ca.Engine(n, q, t, device=-1)
    rng = np.random.RandomState(1)
    v = rng.randint(-(t // 2), t // 2 + 1, size=(rows, n)).astype(np.int64)
    d_v, d_vt = E.upload(v), E.upload(np.ascontiguousarray(v.T))
    d_p, d_o = E.alloc(rows * n * 8), E.alloc(rows * n * 8)
    d_r = E1.upload(rng.randint(0, q[0], size=(rows, n)).astype(np.uint64))
    calls = {
        "compose item-major": lambda: E.slots_compose_dev(d_v, rows, n, n, 1, d_p),
        "compose image-major": lambda: E.slots_compose_dev(d_vt, rows, n, 1, rows, d_p),
        "decompose item-major": lambda: E.slots_decompose_dev(d_p, rows, n, d_o, n, 1),
        "decompose image-major": lambda: E.slots_decompose_dev(d_p, rows, n, d_o, 1, rows),
        "crc_ntt_inv": lambda: E1.ntt_inv(d_r, rows // 2),
        "crc_ntt_fwd": lambda: E1.ntt_fwd(d_r, rows // 2),
    }
    for fn in calls.values():                                  # warm-up: code objects, the tables of t, the LDS opt-in
        fn()
    E.sync(); E1.sync()
    # the two layouts carry the same numbers, and a round trip gives them back -- before anything is timed
    calls["compose item-major"](); a = E.download(d_p, (rows, n))
    calls["compose image-major"](); same = bool(np.array_equal(E.download(d_p, (rows, n)), a))
    calls["decompose item-major"](); back = bool(np.array_equal(E.download(d_o, (rows, n), dtype=np.int64), v))
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E1 if nm.startswith("crc_ntt") else E, fn, reps))
    host = {}
    hrows = min(rows, 1024)
    for nm, fn in (("compose", lambda: H.slots_compose(v[:hrows], hrows, n, n, 1)), ("decompose", lambda: H.slots_decompose(a[:hrows], n, n, 1))):
        fn()
        t0 = time.perf_counter(); fn(); host[nm] = 1e3 * (time.perf_counter() - t0) / hrows * rows
    print(json.dumps(dict(n=n, k=k, t=t, rows=rows, layouts_equal=same, round_trip=back, rounds=rounds, reps=reps, ms=ms, host_ms=host,
                          host_threads=E.L.crc_host_thread_limit())), flush=True)
    return 0 if same and back else 3


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_slots] exit {p.returncode}: {' '.join(cmd[-8:])}", file=sys.stderr, flush=True)
    return p.stdout if p.returncode == 0 else None


def end_to_end(a, log):
    """-> dict for the report, or None when a step failed"""
    import numpy as np
    import crcnn_amd as ca
    import slots_model as sm
    from crcnn_amd import netrun
    from netcommon import GOLD, model_weights
    n, k, S = 4096, 2, a.images
    q = ca.default_coeff_modulus_128(n)[:k]
    layers = netrun.load_description("PlainModelTiny")
    W = model_weights("PlainModelTiny")
    images = np.random.RandomState(7).uniform(-1, 1, size=(S,) + tuple(layers.input_shape)).astype(np.float32)
    exact, scale = sm.network_forward(list(layers), W, images, 1 << 400, a.input_bits, a.weight_bits)      # a modulus no value reaches: the exact integers
    peak = max(abs(v) for row in exact for v in row)
    def prime(b):
        try:
            return ca.Engine.slots_prime(n, b)
        except ca.CrcError:                                    # no prime of that shape below 2^b
            return 0
    bits = next(b for b in range(n.bit_length() + 1, 61) if prime(b) > 2 * peak)
    t = ca.Engine.slots_prime(n, bits)
    res = dict(n=n, k=k, S=S, scale=scale, peak=peak, bits=bits, t=t, q_bits=sum(int(v).bit_length() for v in q), input_bits=a.input_bits, weight_bits=a.weight_bits)
    if any(t >= v for v in q):
        res["failed"] = "the plain modulus would not be below the coefficient moduli"
        return res
    d = tempfile.mkdtemp()
    np.array([n, k, t] + q, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    out = run([os.path.join(ROOT, "crcnn_amd", "lib", "test_host"), "slots_build", "PlainModelTiny", os.path.join(GOLD, "models", "PlainModelTiny.h5"), d, str(S),
               str(a.input_bits), str(a.weight_bits), str(a.forward_reps)], 400, log)
    if out is None:
        return None
    lines = dict(l.split(" ", 1) for l in out.splitlines() if " " in l)
    got = np.fromfile(os.path.join(d, "slots_fused.i64"), dtype=np.int64).reshape(S, -1)
    res.update(budget=int(lines["budget"].split()[3]), budget_unfused=int(lines["budget"].split()[1]), forward_ms=float(lines["forward_ms"]),
               logits_equal=got.tolist() == exact)
    return res


def report(results, e2e, a):
    L = ["# Slot batching: compose / decompose on the device, and n images per ciphertext end to end", "",
         f"One MI355X.  `crc_slots_compose_dev` / `crc_slots_decompose_dev` on {a.rows} rows of n slots per call, t = crc_slots_prime(n, 30); HIP events around {a.reps} calls,",
         f"the calls alternating in one process, {a.rounds} rounds: median (min .. max) in us per row.  `crc_ntt_inv` / `crc_ntt_fwd`: the same build's row transform on as",
         "many rows of one coefficient modulus.  Host twins: wall clock on the host's threads, scaled from at most 1024 rows.", ""]
    for r in results:
        n, rows = r["n"], r["rows"]
        us = {nm: [1e3 * v / rows for v in vs] for nm, vs in r["ms"].items()}
        med = {nm: statistics.median(v) for nm, v in us.items()}
        L += [f"## (n, k) = ({n}, {r['k']}), t = {r['t']}", "", "| call | us per row | min .. max | against the row transform | algorithmic TB/s (16 n bytes per row) |", "|---|---|---|---|---|"]
        for nm in us:
            base = "crc_ntt_inv" if nm.startswith("compose") or nm == "crc_ntt_inv" else "crc_ntt_fwd"
            L.append(f"| {nm} | {med[nm]:.3f} | {min(us[nm]):.3f} .. {max(us[nm]):.3f} | {med[nm] / med[base]:.2f} x {base} | {16 * n / med[nm] / 1e6:.2f} |")
        for nm, ms in r["host_ms"].items():
            L.append(f"| host {nm} ({r['host_threads']} threads) | {1e3 * ms / rows:.2f} | | {1e3 * ms / rows / med[nm + ' item-major']:.0f} x the device call | |")
        L += ["", f"Both layouts give the same plaintexts: {r['layouts_equal']}; decompose(compose(v)) == v: {r['round_trip']}.", ""]
        for kind, base in (("compose", "crc_ntt_inv"), ("decompose", "crc_ntt_fwd")):
            extra = med[kind + " image-major"] - med[base]
            gather = 7 * 8 * n / (16 * n / med[base])          # 56 n more bytes at the rate the row transform moves its 16 n
            if extra > gather:
                L.append(f"{kind}, image-major: {extra:.3f} us per row above the row transform, more than the {gather:.3f} us an 8-byte-granular access to 64-byte sectors "
                         "explains: the rest is the slot-order LDS accesses of the permutation (scattered 8-byte writes / reads, bank conflicts at random) and, at "
                         "n = 8192, the gap-1 stage run as a pass of its own.")
            else:
                L.append(f"{kind}, image-major: {extra:+.3f} us per row against the row transform, within the {gather:.3f} us an 8-byte-granular access to 64-byte sectors explains.")
        L.append("")
    L += ["## End to end: PlainModelTiny, quantised, at (4096, 2)", ""]
    if e2e is None:
        L += ["not measured (the run failed; see the log)", ""]
    else:
        L += [f"input_bits = {e2e['input_bits']}, weight_bits = {e2e['weight_bits']}: output scale {e2e['scale']} = 2^{int(e2e['scale']).bit_length() - 1}; the exact integer network "
              f"(tests/slots_model.py) on {e2e['S']} synthetic images has logits up to {e2e['peak']} in magnitude, so the smallest plain modulus that carries them without "
              f"wrap-around is crc_slots_prime(4096, **{e2e['bits']}**) = {e2e['t']} (coefficient modulus: {e2e['q_bits']} bits).", ""]
        if "failed" in e2e:
            L += [f"No t below q carries it: {e2e['failed']}.", ""]
        else:
            ok = e2e["logits_equal"] and e2e["budget"] > 0
            L += [f"`test_host slots_build` there: decoded logits of every image equal the integer model's: **{e2e['logits_equal']}**; noise budget left (minNoiseBudget of the output "
                  f"tensor): **{e2e['budget']}** bits fused, {e2e['budget_unfused']} unfused; {e2e['forward_ms']:.3f} ms per tensor evaluation (fused, wall clock over "
                  f"{a.forward_reps} forwards between two stream synchronisations) = {1e3 / e2e['forward_ms']:.1f} evaluations/s.", ""]
            if ok:
                L += [f"Every slot is an image: images/s = slots x evaluations/s = {e2e['n']} x {1e3 / e2e['forward_ms']:.1f} = **{e2e['n'] * 1e3 / e2e['forward_ms']:.0f}** with all "
                      f"{e2e['n']} slots filled ({e2e['S']} were checked against the model; the evaluation does not depend on how many slots are in use).", ""]
            else:
                L += ["**No plain modulus carries the network at these parameters**: the smallest t without wrap-around leaves no noise budget (or the logits differ).  A smaller "
                      "weight_bits / input_bits, a larger ring, or several plain moduli with a CRT over them (out of scope) would be needed.", ""]
    L += [f"command: python tools/measure_slots.py --rounds {a.rounds} --reps {a.reps} --rows {a.rows} --images {a.images} --input-bits {a.input_bits} --weight-bits {a.weight_bits}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--images", type=int, default=8); ap.add_argument("--input-bits", type=int, default=4); ap.add_argument("--weight-bits", type=int, default=5)
    ap.add_argument("--forward-reps", type=int, default=20)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "slot_batching.md"))
    a = ap.parse_args()
    if a.mode == "step":
        return step(a.shape[0], a.shape[1], a.shape[2], a.rounds, a.reps)
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, results = [], []
    me = [sys.executable, os.path.abspath(__file__)]
    ok = True
    for n, k in SHAPES:
        out = run(me + ["step", str(n), str(k), str(a.rows), "--rounds", str(a.rounds), "--reps", str(a.reps)], 240, log)
        if out is None:
            ok = False
            break
        results.append(json.loads(out.strip().splitlines()[-1]))
    e2e = end_to_end(a, log) if ok else None
    open(os.path.join(out_dir, "measure_slots.log"), "w").write("\n".join(log))
    if not results:
        print("\n".join(log)[-3000:])
        return 2
    text = report(results, e2e, a)
    print(text)
    if ok and e2e is not None and a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok and e2e is not None else 1


if __name__ == "__main__":
    sys.exit(main())
