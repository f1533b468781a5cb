#!/usr/bin/env python3
"""The device encryptor of the seeded form against the host one.

One process alternates, for `--rounds` rounds and on the same encoder-made plaintexts, at (2048, 1), (4096, 2) and (8192, 3):
  (a) crc_encrypt_sym_seeded           host, CRC_HOST_THREADS threads (16 by default), wall clock around the call
  (b) crc_encrypt_sym_seeded_dev       HIP events around `--reps` calls, plaintexts and key resident
  (c) crc_encrypt_sym_dev_forms(NTT)   HIP events, the same way
(a) and (c) are code of the commit in front of the device encryptor: the yardsticks.  (b) is never compared with itself.  The counts are whole 28 x 28 images
(784 ciphertexts each), 1/16 of the per-layer counts of profiles/seeded_inputs.md, so that a host call takes a fraction of a second to seconds.  Before the
timing the device rows are compared with the host's, bit for bit.

gate: at every set the median of (b) is below the median of (a) by more than the larger max - min of the two.  (b) against (c) is reported without a gate.

Then the whole client call: crcnn_amd/lib/seeded_host time (encryptImageSeeded, host path against device path, per image, upload and download included), a child
process per set under `timeout -k 10`.

  --kernels   one process, nothing but kernels (for `rocprofv3 --kernel-trace --stats -- python tools/measure_seeded_encrypt.py --kernels`): the two encryptors
              on zero plaintexts at the real counts of profiles/seeded_inputs.md

--markdown FILE writes the report (the tables, the gate's verdicts, the box and the command) to FILE: profiles/seeded_encrypt_runs.md is that file as committed;
profiles/seeded_encrypt.md, written by hand, holds the compiler's resource report, the kernel trace and the reading of both.

usage: measure_seeded_encrypt.py [--rounds 7] [--reps 20] [--markdown profiles/seeded_encrypt_runs.md] [--kernels]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [dict(n=2048, k=1, t=1 << 18, images=16), dict(n=4096, k=2, t=1 << 29, images=8), dict(n=8192, k=3, t=1 << 42, images=2)]
KERNEL_SETS = [dict(n=4096, k=2, t=1 << 29, count=128 * 784), dict(n=2048, k=1, t=1 << 18, count=256 * 784), dict(n=8192, k=3, t=1 << 42, count=32 * 784)]
SEEDED_HOST = os.path.join(ROOT, "crcnn_amd", "lib", "seeded_host")


def event_us(E, fn, reps, count):
    """microseconds per ciphertext of fn(), HIP events around `reps` calls on the engine's stream"""
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
    return ms.value * 1e3 / reps / count


def kernels(reps):
    import crcnn_amd as ca
    for s in KERNEL_SETS:
        n, k, t, count = s["n"], s["k"], s["t"], s["count"]
        E = ca.Engine(n, ca.default_coeff_modulus_128(n)[:k], t, device=0)
        sk, _ = E.keygen(11)
        d_sk = E.upload(sk)
        d_c0 = E.alloc(count * k * n * 8); d_ct = E.alloc(count * 2 * k * n * 8); d_pl = E.alloc(count * n * 8)
        d_w = E.alloc(E.encrypt_sym_dev_work_bytes(count))
        E.L.crc_memset(E.c, E.p(d_pl), 0, count * n * 8, E.stream)
        seeded = lambda: E.encrypt_sym_seeded_dev(d_sk, d_pl, count, 5, d_c0)
        sym = lambda: E.encrypt_sym_dev_forms(d_sk, d_pl, count, 5, ca.NTT, d_ct, d_w)
        seeded(); sym(); E.sync()
        b, c = event_us(E, seeded, reps, count), event_us(E, sym, reps, count)
        print(f"({n}, {k}) {count} ciphertexts: crc_encrypt_sym_seeded_dev {b:.4f} us per ciphertext, crc_encrypt_sym_dev_forms(NTT) {c:.4f} us per ciphertext")
        E.close()
    return 0


def stats(v):
    return statistics.median(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--host-images", type=int, default=4, help="images per encryptImageSeeded call of seeded_host time")
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.reps)
    import numpy as np
    import torch
    import crcnn_amd as ca
    pr = torch.cuda.get_device_properties(0)
    box = f"{pr.name} ({pr.gcnArchName}, {pr.multi_processor_count} CUs, {pr.total_memory >> 30} GiB), torch {torch.__version__}"
    threads = os.environ.get("CRC_HOST_THREADS", "default (the hardware's, at most 16)")
    lines, ok = [f"# crc_encrypt_sym_seeded_dev against crc_encrypt_sym_seeded: microseconds per ciphertext, {a.rounds} alternating rounds", ""], True
    PU = ctypes.POINTER(ctypes.c_uint64)
    for s in SETS:
        n, k, t, count = s["n"], s["k"], s["t"], s["images"] * 784
        E = ca.Engine(n, ca.default_coeff_modulus_128(n)[:k], t, device=0)
        sk, _ = E.keygen(11)
        rng = np.random.default_rng(3)
        pl, _ = E.encode(((rng.random(count) - 0.1307) / 0.3081).astype(np.float32))
        d_sk = E.upload(sk); d_pl = E.upload(pl)
        d_c0 = E.alloc(count * k * n * 8); d_ct = E.alloc(count * 2 * k * n * 8); d_w = E.alloc(E.encrypt_sym_dev_work_bytes(count))
        h_c0 = np.zeros((count, k, n), dtype=np.uint64)
        host = lambda: E.L.crc_encrypt_sym_seeded(E.c, sk.ctypes.data_as(PU), pl.ctypes.data_as(PU), count, 5, h_c0.ctypes.data_as(PU))
        seeded = lambda: E.encrypt_sym_seeded_dev(d_sk, d_pl, count, 5, d_c0)
        sym = lambda: E.encrypt_sym_dev_forms(d_sk, d_pl, count, 5, ca.NTT, d_ct, d_w)
        assert host() == 0
        seeded(); sym(); E.sync()
        assert np.array_equal(E.download(d_c0, (count, k, n)), h_c0), "the device rows differ from the host's"
        A, B, C = [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); rc = host(); A.append((time.perf_counter() - t0) * 1e6 / count)
            assert rc == 0
            B.append(event_us(E, seeded, a.reps, count))
            C.append(event_us(E, sym, a.reps, count))
        (ma, sa), (mb, sb), (mc, sc) = stats(A), stats(B), stats(C)
        gate = ma - mb > max(sa, sb)
        ok = ok and gate
        lines += [f"## ({n}, {k}), {count} ciphertexts ({s['images']} images)", "", "| round | (a) host crc_encrypt_sym_seeded | (b) crc_encrypt_sym_seeded_dev | (c) crc_encrypt_sym_dev_forms(NTT) |",
                  "|---|---|---|---|"]
        lines += [f"| {i + 1} | {A[i]:.3f} | {B[i]:.4f} | {C[i]:.4f} |" for i in range(a.rounds)]
        lines += [f"| median | {ma:.3f} | {mb:.4f} | {mc:.4f} |", f"| max - min | {sa:.3f} | {sb:.4f} | {sc:.4f} |", "",
                  f"GATE: median (b) is below median (a) by {ma - mb:.3f} us, " + ("more" if gate else "NOT more") + f" than the larger max - min of the two ({max(sa, sb):.3f} us): "
                  + ("passed" if gate else "FAILED") + f".  (a) / (b) = {ma / mb:.0f}.",
                  f"No gate: (b) / (c) = {mb / mc:.3f} (the seeded encryptor runs {1 + (k + 1) // 2} ChaCha20 blocks per coefficient pair, the secret-key encryptor {k // 2 + 1}).", ""]
        E.close()
    lines += ["# The whole client call: encryptImageSeeded per 28 x 28 image, host path against device path (wall clock, upload and download included)", ""]
    for s in SETS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), SEEDED_HOST, "time", str(s["n"]), str(s["t"]), str(a.host_images), str(a.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(f"measure_seeded_encrypt: seeded_host exited with {p.returncode}: {p.stderr[-1500:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        lines += [f"## ({r['n']}, {r['k']}), {r['images']} images per call, ms per image", "", "| path | " + " | ".join(f"round {i + 1}" for i in range(a.rounds)) + " | median | max - min |",
                  "|---|" + "---|" * (a.rounds + 2)]
        for path in ("host", "device"):
            v = r[path]
            lines.append(f"| {path} | " + " | ".join(f"{x:.2f}" for x in v["rounds"]) + f" | {v['median']:.2f} | {v['max_minus_min']:.2f} |")
        lines += ["", f"host / device = {r['host']['median'] / r['device']['median']:.1f}", ""]
    lines += [f"box: {box}; host threads: {threads}",
              f"command: python tools/measure_seeded_encrypt.py --rounds {a.rounds} --reps {a.reps} --host-images {a.host_images} --markdown profiles/seeded_encrypt_runs.md"]
    text = "\n".join(lines)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
