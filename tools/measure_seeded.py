#!/usr/bin/env python3
"""Streamed inputs as SEEDED secret-key ciphertexts (the c0 rows and a public seed; c1 regenerated on the device) against streamed full ciphertexts.

bench.py prepares a configuration's inputs and leaves its bench_host command line (CRC_BENCH_KEEP, run with --full --stream-inputs both so that plain_inputs.u64
exists); that command line then runs `--runs` times with stream_inputs=ciphertext,seeded -- both modes in the SAME bench_host invocation, behind its resident
measurement.  The ciphertext mode is code the seeded form does not touch: its figure is the figure of the commit in front of it.

gate (tiny4096): the median seeded rate exceeds the median ciphertext rate by more than the larger of the two modes' max - min over the invocations.
Every reported run must state outputs_identical_to_resident (ciphertext) and outputs_decrypt_identical_to_resident (seeded).  Each bench_host run is a child of
its own under `timeout -k 10`; the tool stops at the first non-zero exit.

  --kernels   one process, nothing but kernels (for `rocprofv3 --kernel-trace --stats -- python tools/measure_seeded.py --kernels`): seeded_expand_kernel and
              enc_sym_sample_kernel<false> (inside crc_encrypt_sym_dev_forms) on the same ciphertext counts at (4096, 2), (2048, 1), (8192, 3); HIP-event
              times of the two CALLS are printed as well (the sampler's call includes its forward transform: the trace separates the kernels)

usage: measure_seeded.py [--configs tiny4096,approx8192] [--runs 3] [--stream-steps N] [--markdown profiles/seeded_inputs.md] [--kernels]"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_SETS = [dict(n=4096, k=2, t=1 << 29, count=128 * 784), dict(n=2048, k=1, t=1 << 18, count=256 * 784), dict(n=8192, k=3, t=1 << 42, count=32 * 784)]
BAND = {"tiny4096": (523.0, 526.0)}          # the streamed-ciphertext line of the commit in front of this one


def kernels(reps):
    import numpy as np
    import crcnn_amd as ca
    for s in KERNEL_SETS:
        n, k, t, count = s["n"], s["k"], s["t"], s["count"]
        q = ca.default_coeff_modulus_128(n)[:k]
        E = ca.Engine(n, q, t, device=0)
        sk, _ = E.keygen(11)
        d_sk = E.upload(sk)
        d_c0 = E.alloc(count * k * n * 8); d_ct = E.alloc(count * 2 * k * n * 8); d_pl = E.alloc(count * n * 8)
        d_w = E.alloc(E.encrypt_sym_dev_work_bytes(count))
        E.L.crc_memset(E.c, E.p(d_c0), 0, count * k * n * 8, E.stream); E.L.crc_memset(E.c, E.p(d_pl), 0, count * n * 8, E.stream)
        seed = bytes(range(32))

        def timed(fn):
            e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
            E.L.crc_event_create(E.c, ctypes.byref(e0)); E.L.crc_event_create(E.c, ctypes.byref(e1))
            fn(); fn()
            E.L.crc_event_record(E.c, e0, E.stream)
            for _ in range(reps):
                fn()
            E.L.crc_event_record(E.c, e1, E.stream)
            E.sync()
            ms = ctypes.c_float()
            E.L.crc_event_elapsed_ms(E.c, e0, e1, ctypes.byref(ms))
            E.L.crc_event_destroy(E.c, e0); E.L.crc_event_destroy(E.c, e1)
            return ms.value * 1e3 / reps / count

        ex = timed(lambda: E.seeded_expand_dev(d_c0, count, seed, 0, ca.NTT, d_ct))
        en = timed(lambda: E.encrypt_sym_dev_forms(d_sk, d_pl, count, 5, ca.NTT, d_ct, d_w))
        byts = 3 * k * n * 8
        print(f"({n}, {k}) {count} ciphertexts: crc_seeded_expand_dev {ex:.4f} us per ciphertext ({byts / ex / 1e6:.3f} TB/s algorithmic: {k * n * 8} B read + "
              f"{2 * k * n * 8} B written); crc_encrypt_sym_dev_forms (sampler + transform) {en:.4f} us per ciphertext")
        E.close()
    return 0


def bench_host_runs(name, runs, stream_steps, step_timeout):
    keep = tempfile.mkdtemp(prefix="crc_seeded_")
    env = dict(os.environ, CRC_BENCH_KEEP=keep, CRC_BENCH_KEEP_CONFIGS=name)
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--config", name, "--cpu-seconds", "0", "--also", "none",
                    "--full", "--stream-inputs", "both", "--stream-steps", "1"], check=True, env=env, stdout=subprocess.DEVNULL, timeout=step_timeout)
    cmd = open(os.path.join(keep, name, f"cmd_{name}.txt")).read().split()
    cmd = [c for c in cmd if not c.startswith(("stream_inputs=", "stream_steps=", "steps=", "warmup="))]
    cmd += ["steps=1", "warmup=0", "stream_inputs=ciphertext,seeded", f"stream_steps={stream_steps}"]
    rows = []
    try:
        for _ in range(runs):
            p = subprocess.run(["timeout", "-k", "10", str(step_timeout)] + cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise SystemExit(f"measure_seeded: bench_host exited with {p.returncode}: {p.stderr[-1500:]}")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            modes = {s["mode"]: s for s in line["streamed"]}
            assert modes["ciphertext"]["outputs_identical_to_resident"] is True, "ciphertext mode: outputs differ from the resident launch's"
            assert modes["seeded"]["outputs_decrypt_identical_to_resident"] is True, "seeded mode: outputs decrypt differently from the resident launch's"
            assert line["last_timed_launch_identical_to_first"] is True
            rows.append(dict(resident=line["images_per_s"], **{m: dict(rate=s["images_per_s"], gbps=s["h2d_GBps"], bytes=s["bytes_per_image"], elapsed=s["elapsed_s"])
                                                               for m, s in modes.items()}))
    finally:
        shutil.rmtree(keep, ignore_errors=True)
    return rows, " ".join(os.path.basename(c) if c.startswith("/") else c for c in cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="tiny4096,approx8192")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--stream-steps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.reps)
    if a.runs < 3:
        ap.error("--runs: at least 3")
    import torch
    pr = torch.cuda.get_device_properties(0)
    box = f"{pr.name} ({pr.gcnArchName}, {pr.multi_processor_count} CUs, {pr.total_memory >> 30} GiB), torch {torch.__version__}"
    lines, ok = [], True
    for name in [c for c in a.configs.split(",") if c]:
        rows, cmd = bench_host_runs(name, a.runs, a.stream_steps, a.step_timeout)
        lines += [f"## {name}", "", "| invocation | resident images/s | ciphertext images/s (of resident) | h2d GB/s | seeded images/s (of resident) | h2d GB/s | timed window s (ciphertext, seeded) |",
                  "|---|---|---|---|---|---|---|"]
        for i, r in enumerate(rows):
            c, s = r["ciphertext"], r["seeded"]
            lines.append(f"| {i + 1} | {r['resident']:.1f} | {c['rate']:.1f} ({c['rate'] / r['resident']:.3f}) | {c['gbps']:.1f} | {s['rate']:.1f} ({s['rate'] / r['resident']:.3f}) | "
                         f"{s['gbps']:.1f} | {c['elapsed']:.2f}, {s['elapsed']:.2f} |")
        cr, sr = [r["ciphertext"]["rate"] for r in rows], [r["seeded"]["rate"] for r in rows]
        mc, ms = statistics.median(cr), statistics.median(sr)
        spread = max(max(cr) - min(cr), max(sr) - min(sr))
        lines += ["", f"bytes per image: ciphertext {rows[0]['ciphertext']['bytes']}, seeded {rows[0]['seeded']['bytes']}",
                  f"median ciphertext {mc:.1f} images/s, median seeded {ms:.1f} images/s: seeded / ciphertext = {ms / mc:.3f}; larger max - min of the two modes {spread:.1f} images/s"]
        if name in BAND:
            lo, hi = BAND[name]
            lines.append(f"ciphertext mode (unchanged code: the figure of the commit in front of this one) against DESIGN.md's recorded {lo:.0f}-{hi:.0f} images/s: "
                         + ("inside the band" if lo <= mc <= hi else f"OUTSIDE the band ({mc:.1f}): this box differs from the one that recorded it; reported, not adjusted"))
            gate = ms - mc > spread
            ok = ok and gate
            lines.append(f"GATE: the median seeded rate exceeds the median ciphertext rate by {ms - mc:.1f} images/s, " + ("more" if gate else "NOT more") + f" than the spread of {spread:.1f}: "
                         + ("passed" if gate else "FAILED"))
        else:
            verdict = "slower by more than the spread: the cost of the expansion shows" if mc - ms > spread else ("faster by more than the spread" if ms - mc > spread else
                                                                                                           "within the spread of the ciphertext mode")
            lines.append(f"no gate for this configuration; seeded is {verdict}")
        lines += ["", f"bench_host arguments: {cmd}", ""]
    lines += [f"box: {box}",
              f"command: python tools/measure_seeded.py --configs {a.configs} --runs {a.runs} --stream-steps {a.stream_steps}"]
    text = "\n".join(lines)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
