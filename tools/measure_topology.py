#!/usr/bin/env python3
"""Moved-bytes rate of pad_kernel (crc_pad) beside pool_kernel's (crc_pool) in the same run, on the same tensor.

The tensor has the shape of ApproxPlainModel's conv1 output, [B][20][12][12] ciphertexts, with B chosen so that it is several times the 256-MiB last-level
cache: 3 GiB at (n, k) = (4096, 2), 5.6 GiB at (16384, 4).  pool: the 2 x 2 / 1 sum pooling behind conv1 (-> 11 x 11); pad: one ring of zero ciphertexts
(-> 14 x 14).  Both in NTT form (the form an NTT-resident network hands them).  Moved bytes are what the algorithm needs: every input byte once, every output
byte once (a pooling window's overlapping reads are the caches' business; a pad's border rows are written, not read).  HIP events around `--reps` calls after
`--warmup` calls, `--rounds` rounds alternating the two kernels; the table gives the median round and the spread.

usage: measure_topology.py [--reps 20] [--warmup 3] [--rounds 5] [--markdown FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crcnn_amd as ca  # noqa: E402

SETS = [(4096, 2, 8), (16384, 4, 2)]          # n, k, B
ZD, XD, YD = 20, 12, 12


def events_ms(E, fn, reps, warmup):
    for _ in range(warmup):
        fn()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--markdown")
    a = ap.parse_args()
    rows = []
    for n, k, B in SETS:
        E = ca.Engine(n, ca.default_coeff_modulus_128(n)[:k], 1 << 20, device=0)
        ctb = 2 * k * n * 8
        cts_in, cts_pool, cts_pad = B * ZD * XD * YD, B * ZD * (XD - 1) * (YD - 1), B * ZD * (XD + 2) * (YD + 2)
        d_x = E.alloc(cts_in * ctb); d_pool = E.alloc(cts_pool * ctb); d_pad = E.alloc(cts_pad * ctb)
        E.L.crc_memset(E.c, d_x.ptr, 0, cts_in * ctb, E.stream)
        E.sync()
        kernels = {
            "pool_kernel (2x2/1 sum)": (lambda: E.pool(d_x, B, ZD, XD, YD, 1, 1, 2, 2, None, ca.NTT, d_pool), (cts_in + cts_pool) * ctb),
            "pad_kernel (pad 1 1)": (lambda: E.pad(d_x, B, ZD, XD, YD, 1, 1, 1, 1, ca.NTT, d_pad), (cts_in + cts_pad) * ctb),
            "pad_kernel (pad 0 0: copy)": (lambda: E.pad(d_x, B, ZD, XD, YD, 0, 0, 0, 0, ca.NTT, d_pad), 2 * cts_in * ctb),
        }
        ms = {nm: [] for nm in kernels}
        for _ in range(a.rounds):
            for nm, (fn, _) in kernels.items():
                ms[nm].append(events_ms(E, fn, a.reps, a.warmup))
        for nm, (_, moved) in kernels.items():
            med = statistics.median(ms[nm])
            rows.append(dict(n=n, k=k, B=B, kernel=nm, gib=moved / 2 ** 30, ms=med, ms_min=min(ms[nm]), ms_max=max(ms[nm]), tbs=moved / (med * 1e-3) / 1e12))
            print(rows[-1], flush=True)
        E.close()
    lines = ["| n | k | images | kernel | moved GiB | ms (median of %d rounds) | min .. max ms | TB/s |" % a.rounds, "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['k']} | {r['B']} | {r['kernel']} | {r['gib']:.2f} | {r['ms']:.3f} | {r['ms_min']:.3f} .. {r['ms_max']:.3f} | {r['tbs']:.2f} |")
    lines.append("")
    lines.append(f"command: python tools/measure_topology.py --reps {a.reps} --warmup {a.warmup} --rounds {a.rounds}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)


if __name__ == "__main__":
    main()
