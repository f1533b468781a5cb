#!/usr/bin/env python3
"""The scalar limb form (CRC_NTTLS) against the row path, layer by layer, on one MI355X -> profiles/scalar_mac.md.

The conv / dense layers behind conv1 of PlainModelTiny at (n, k) = (4096, 2) and of ApproxPlainModel at (8192, 3), as a slot-batched forward launches them: ONE
ciphertext tensor (B = 1), input handed over in the packed form, result in NTT form.  Per layer
  off   crc_conv2d_forms on the weight form crc_plan_mac gives the layer at B = 1 (constant rows: mac_stream_kernel / mac3_kernel on CRC_NTTP, or the per-slot limb
        GEMM on CRC_NTTL), and
  on    the same call with w_form = CRC_NTTLS on crc_scalar_pack_weights' result,
HIP events around `--reps` calls, off and on alternating `--rounds` times in one process on one device; median over the rounds and the spread (max - min) / median
of each.  The two results must be the same bits.  Beside the times the resident weight bytes of either form.  Nothing is fixed in advance: the table decides
crc_plan_mac_scalar's default (tuning key scalar_mac).

What this tool does NOT do: build the parent commit and check the off path against it (the off path here is this build's row path), and run the layers through
the host classes (tests/test_gpu_scalar_net.py does that at n = 256).

One process per ring, each under its own `timeout`, stopped at the first that fails:
    measure_scalar_mac.py                the driver
    measure_scalar_mac.py step MODEL     one model, in process; prints one JSON line per layer
Options: --rounds (3), --reps (10), --markdown FILE."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (zd, xd, yd, xs, ys, xf, yf, nf) as the fused networks run them (tests/test_abi_cpu.py)
MODELS = {
    "PlainModelTiny": (4096, 2, [("conv2+pool2", (32, 12, 12, 2, 2, 6, 6, 64)), ("fc3", (1024, 1, 1, 1, 1, 1, 1, 512)), ("fc4", (512, 1, 1, 1, 1, 1, 1, 10))]),
    "ApproxPlainModel": (8192, 3, [("conv2", (20, 11, 11, 2, 2, 3, 3, 50)), ("fc3", (800, 1, 1, 1, 1, 1, 1, 500)), ("fc4", (500, 1, 1, 1, 1, 1, 1, 10))]),
}
FORM_NAMES = {1: "CRC_NTT", 2: "CRC_NTTP", 3: "CRC_NTTL"}


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


def step(model, rounds, reps):
    import numpy as np
    import torch
    import crcnn_amd as ca
    n, k, layers = MODELS[model]
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, ca.Engine.slots_prime(n, 20), device=0)
    rng = np.random.default_rng(n)
    qa = np.array(q, dtype=np.uint64)
    for name, g in layers:
        zd, xd, yd, xs, ys, xf, yf, nf = g
        P = ((xd - xf) // xs + 1) * ((yd - yf) // ys + 1)
        ws = rng.integers(0, 1 << 62, size=(nf, zd, xf, yf, k), dtype=np.uint64) % qa
        x = rng.integers(0, 1 << 62, size=(1, zd, xd, yd, 2, k, n), dtype=np.uint64) % qa.reshape(k, 1)
        bias = rng.integers(0, 1 << 62, size=(nf, k, n), dtype=np.uint64) % qa.reshape(k, 1)
        # constant rows, expanded on the device (torch is plumbing only: fc3's rows are tens of GB)
        rows = torch.from_numpy(ws.view(np.int64)).to("cuda:0")[..., None].expand(nf, zd, xf, yf, k, n).contiguous()
        torch.cuda.synchronize()
        d_x = E.upload(x); E.pack28(d_x, zd * xd * yd * 2 * k); d_b = E.upload(bias)
        d_ws = E.alloc(E.scalar_weights_bytes(nf, zd, xf, yf))
        assert E.scalar_supported(1, *g) and E.scalar_pack_weights(rows, n, nf, zd, xf, yf, d_ws)
        off_form = E.plan_mac(*g, 1)
        row_bytes = rows.numel() * 8
        if off_form == ca.NTTL:
            d_wl = E.alloc(E.limb_weights_bytes(nf, zd, xf, yf)); E.limb_pack_weights(rows, nf, zd, xf, yf, d_wl)
            d_woff, row_bytes = d_wl, E.limb_weights_bytes(nf, zd, xf, yf)
            del rows; torch.cuda.empty_cache()
        else:
            if off_form == ca.NTTP:
                E.pack28(rows, nf * zd * xf * yf * k)
            d_woff = rows
        ybytes = nf * P * 2 * k * n * 8
        d_y = {f: E.alloc(ybytes) for f in ("off", "on")}
        work = {"off": E.alloc(E.conv2d_forms_work_bytes(1, *g, ca.NTTP, off_form, ca.NTT)), "on": E.alloc(E.conv2d_forms_work_bytes(1, *g, ca.NTTP, ca.NTTLS, ca.NTT))}
        run = {"off": lambda: E.conv2d(d_x, d_woff, d_b, 1, *g, ca.NTTP, ca.NTT, d_y["off"], work["off"], w_form=off_form),
               "on": lambda: E.conv2d(d_x, d_ws, d_b, 1, *g, ca.NTTP, ca.NTT, d_y["on"], work["on"], w_form=ca.NTTLS)}
        for f in run.values():
            f(); f()
        E.sync()
        same = bool(np.array_equal(E.download(d_y["off"], (nf * P * 2 * k, n)), E.download(d_y["on"], (nf * P * 2 * k, n))))
        times = {"off": [], "on": []}
        for _ in range(rounds):
            for key in ("off", "on"):
                times[key].append(events_ms(E, run[key], reps))
        print(json.dumps({"model": model, "n": n, "k": k, "layer": name, "geometry": list(g), "off_form": FORM_NAMES.get(off_form, str(off_form)), "same_bits": same,
                          "off_ms": times["off"], "on_ms": times["on"], "row_bytes": int(row_bytes), "scalar_bytes": int(E.scalar_weights_bytes(nf, zd, xf, yf))}), flush=True)
        del d_woff, d_x, d_b, d_ws, d_y, work, run
        torch.cuda.empty_cache()
    E.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "scalar_mac.md"))
    a = ap.parse_args()
    if a.cmd and a.cmd[0] == "step":
        return step(a.cmd[1], a.rounds, a.reps)
    res = []
    for model in MODELS:
        out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "step", model, "--rounds", str(a.rounds), "--reps", str(a.reps)],
                             capture_output=True, text=True)
        sys.stderr.write(out.stderr[-2000:])
        if out.returncode != 0:
            sys.exit(f"step {model} failed with status {out.returncode}: nothing further is started")
        res += [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    lines = ["# Scalar limb form (CRC_NTTLS) against the row path", "",
             f"tools/measure_scalar_mac.py: one MI355X, one ciphertext tensor per launch (B = 1), in_form CRC_NTTP, out_form CRC_NTT; HIP events around {a.reps} calls, off and",
             f"on alternating {a.rounds} times in one process; median of the rounds, spread = (max - min) / median.  The off path is this build's row path (not",
             "checked against a build of the parent commit).", "",
             "| model (n, k) | layer | row path | off ms | spread | on ms | spread | off / on | same bits | row-path weight bytes | scalar weight bytes |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['model']} ({r['n']}, {r['k']}) | {r['layer']} | {r['off_form']} | {med(r['off_ms']):.4f} | {spread(r['off_ms']):.1%} | {med(r['on_ms']):.4f} | "
                     f"{spread(r['on_ms']):.1%} | {med(r['off_ms']) / med(r['on_ms']):.2f} | {'yes' if r['same_bits'] else 'NO'} | {r['row_bytes']} | {r['scalar_bytes']} |")
    lines += ["", "Raw rounds (ms): " + json.dumps([{k: r[k] for k in ("model", "layer", "off_ms", "on_ms")} for r in res])]
    os.makedirs(os.path.dirname(a.markdown), exist_ok=True)
    open(a.markdown, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if not all(r["same_bits"] for r in res):
        sys.exit("the two paths disagree")


if __name__ == "__main__":
    main()
