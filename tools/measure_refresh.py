#!/usr/bin/env python3
"""A/B of the client-side refresh: re-encryption under the public key (crc_refresh_dev, Encryptor::encrypt: the reference's refresh and the default) against
re-encryption under the secret key (crc_refresh_sym_dev), in ONE process on one device, on the same NTT-form tensors.

  approx4096r   (4096, 2, t = 2^29)  800 ciphertexts per image  (ApproxPlainModel in front of bn2),  64 images per refresh (the configuration's chunk)
  tiny2048r     (2048, 1, t = 2^18)  1024 ciphertexts per image (PlainModelTiny in front of fc3),   256 images per refresh
  ring8192      (8192, 3, t = 2^42)  800 ciphertexts per image,                                      32 images per refresh

The tensors are encryptions of seeded values (the encoder's plaintexts, as a refresh sees them), 8 distinct images tiled on the device, NTT form in and out (what
an NTT-resident network hands over).  HIP events around `--reps` calls; the two modes ALTERNATE, `--rounds` rounds each after `--warmup` untimed calls of each;
the figure is the median over the rounds, the spread their max - min.  The public-key path is the code of the commit in front of this one, unchanged: its
figure is that commit's.  The floats both modes report are asserted identical.

  --kernels      a few calls of one mode and nothing else (for `rocprofv3 --kernel-trace --stats -- python tools/measure_refresh.py --kernels MODE`)
  --bench-host   also T_REENC and images/s of crcnn_amd/lib/bench_host ... reenc_sym=0|1 for the two published configurations (command lines from bench.py
                 through CRC_BENCH_KEEP, alternating, `--bench-steps` steps)

usage: measure_refresh.py [--config NAME|all] [--rounds 7] [--reps 10] [--warmup 3] [--markdown FILE] [--kernels pk|sym] [--bench-host]"""
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
import numpy as np  # noqa: E402
import crcnn_amd as ca  # noqa: E402

CONFIGS = {
    "approx4096r": dict(n=4096, k=2, t=1 << 29, per_image=800, images=64, section_4_7_us=0.30),
    "tiny2048r": dict(n=2048, k=1, t=1 << 18, per_image=1024, images=256, section_4_7_us=0.11),
    "ring8192": dict(n=8192, k=3, t=1 << 42, per_image=800, images=32, section_4_7_us=None),
}
DISTINCT = 8


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


def setup(name):
    cfg = CONFIGS[name]
    n, k, t = cfg["n"], cfg["k"], cfg["t"]
    q = ca.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    sk, pk = E.keygen(11)
    count = cfg["per_image"] * cfg["images"]
    ctb = 2 * k * n * 8
    distinct = DISTINCT * cfg["per_image"]
    rng = np.random.default_rng(3)
    pl, _ = E.encode((rng.standard_normal(distinct) * 3).astype(np.float32))
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    d_in = E.alloc(count * ctb)
    d_pl = E.upload(pl); d_w = E.alloc(E.encrypt_dev_work_bytes(distinct))
    E.encrypt_dev_forms(d_pk, d_pl, distinct, 5, ca.NTT, d_in, d_w)
    E.sync()
    for o in range(distinct, count, distinct):
        c = min(distinct, count - o)
        E.L.crc_memcpy_d2d(E.c, E.p(d_in) + o * ctb, E.p(d_in), c * ctb, E.stream)
    E.sync()
    d_pl.free(); d_w.free()
    d_out = E.alloc(count * ctb); d_vals = E.alloc(count * 4)
    d_work = E.alloc(max(E.refresh_dev_work_bytes(count, ca.NTT), E.refresh_sym_dev_work_bytes(count, ca.NTT)))
    seed = [1000]

    def run_pk():
        seed[0] += 1
        E.refresh_dev(d_sk, d_pk, d_in, count, seed[0], d_out, d_work, in_form=ca.NTT, out_form=ca.NTT, d_values=d_vals)

    def run_sym():
        seed[0] += 1
        E.refresh_sym_dev(d_sk, d_in, count, seed[0], d_out, d_work, in_form=ca.NTT, out_form=ca.NTT, d_values=d_vals)

    return E, cfg, count, run_pk, run_sym, d_vals, (d_sk, d_pk, d_in, d_out, d_work)


def measure(name, rounds, reps, warmup):
    E, cfg, count, run_pk, run_sym, d_vals, keep = setup(name)
    for _ in range(warmup):
        run_pk(); run_sym()
    run_pk(); v_pk = E.download(d_vals, (count,), dtype=np.float32)
    run_sym(); v_sym = E.download(d_vals, (count,), dtype=np.float32)
    assert np.array_equal(v_pk.view(np.uint32), v_sym.view(np.uint32)), "the two refreshes report different floats"
    pk, sym = [], []
    for _ in range(rounds):
        pk.append(events_ms(E, run_pk, reps)); sym.append(events_ms(E, run_sym, reps))
    E.close()
    us = lambda ms: ms * 1e3 / count
    r = dict(config=name, n=cfg["n"], k=cfg["k"], count=count, images=cfg["images"], rounds=rounds, reps=reps,
             pk_us=us(statistics.median(pk)), sym_us=us(statistics.median(sym)), pk_spread_us=us(max(pk) - min(pk)), sym_spread_us=us(max(sym) - min(sym)),
             pk_rounds_us=[round(us(v), 4) for v in pk], sym_rounds_us=[round(us(v), 4) for v in sym], section_4_7_us=cfg["section_4_7_us"])
    r["ratio"] = r["sym_us"] / r["pk_us"]
    r["gate"] = r["pk_us"] - r["sym_us"] > max(r["pk_spread_us"], r["sym_spread_us"])
    return r


def bench_host_ab(name, steps):
    """T_REENC and images/s of bench_host with reenc_sym=0 and 1: bench.py prepares the inputs and leaves its command line (CRC_BENCH_KEEP), run twice each, alternating"""
    import shutil
    keep = tempfile.mkdtemp(prefix="crc_refresh_ab_")
    env = dict(os.environ, CRC_BENCH_KEEP=keep, CRC_BENCH_KEEP_CONFIGS=name)
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--config", name], check=True, env=env,
                   stdout=subprocess.DEVNULL, timeout=900)
    cmd = open(os.path.join(keep, name, f"cmd_{name}.txt")).read().split()
    cmd = [c for c in cmd if not c.startswith(("steps=", "warmup="))] + [f"steps={steps}", "warmup=1"]
    out = {0: [], 1: []}
    for _ in range(2):
        for mode in (0, 1):
            p = subprocess.run(cmd + [f"reenc_sym={mode}"], check=True, capture_output=True, text=True, timeout=900)
            line = json.loads(p.stdout.strip().splitlines()[-1])
            out[mode].append((line["T_REENC_ms_per_image"], line["images_per_s"], line["ms_per_image"]))
    shutil.rmtree(keep, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=sorted(CONFIGS) + ["all"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--markdown", default=None, help="also write the tables to this file")
    ap.add_argument("--kernels", default=None, choices=["pk", "sym"], help="four calls of one mode per configuration and nothing else (for a kernel trace)")
    ap.add_argument("--bench-host", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=3)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5")
    names = [c for c in ("approx4096r", "tiny2048r", "ring8192") if a.config in ("all", c)]
    if a.kernels:
        for name in names:
            E, cfg, count, run_pk, run_sym, d_vals, keep = setup(name)
            fn = run_pk if a.kernels == "pk" else run_sym
            for _ in range(4):
                fn()
            E.sync(); E.close()
            print(f"{name}: 4 calls of the {a.kernels} refresh on {count} ciphertexts")
        return 0
    rows = [measure(name, a.rounds, a.reps, a.warmup) for name in names]
    import torch
    pr = torch.cuda.get_device_properties(0)
    box = f"{pr.name} ({pr.gcnArchName}, {pr.multi_processor_count} CUs, {pr.total_memory >> 30} GiB), torch {torch.__version__}"
    lines = ["| tensor | ciphertexts per call | public key: us per ciphertext (spread) | secret key: us per ciphertext (spread) | secret / public | faster by more than the spread | DESIGN 4.7's public-key figure |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['config']} ({r['n']}, {r['k']}), {r['images']} images | {r['count']} | {r['pk_us']:.4f} ({r['pk_spread_us']:.4f}) | {r['sym_us']:.4f} ({r['sym_spread_us']:.4f}) | "
                     f"{r['ratio']:.3f} | {'yes' if r['gate'] else 'NO'} | {r['section_4_7_us'] if r['section_4_7_us'] else '-'} |")
    lines.append("")
    for r in rows:
        lines.append(f"rounds {r['config']}: public {r['pk_rounds_us']} secret {r['sym_rounds_us']}")
    if a.bench_host:
        lines += ["", "| configuration | reenc_sym | T_REENC ms per image (two runs) | images/s (two runs) | ms per image (two runs) |", "|---|---|---|---|---|"]
        for name in ("approx4096r", "tiny2048r"):
            if a.config not in ("all", name):
                continue
            ab = bench_host_ab(name, a.bench_steps)
            for mode in (0, 1):
                lines.append(f"| {name} | {mode} | {', '.join(f'{v[0]:.4f}' for v in ab[mode])} | {', '.join(f'{v[1]:.1f}' for v in ab[mode])} | {', '.join(f'{v[2]:.4f}' for v in ab[mode])} |")
    lines.append("")
    lines.append(f"box: {box}")
    lines.append(f"command: python tools/measure_refresh.py --config {a.config} --rounds {a.rounds} --reps {a.reps} --warmup {a.warmup}" + (" --bench-host" if a.bench_host else ""))
    text = "\n".join(lines)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["gate"] for r in rows) else 3


if __name__ == "__main__":
    sys.exit(main())
