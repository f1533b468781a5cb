#!/usr/bin/env python3
"""Seeded key-switching keys priced on one MI355X -> profiles/seeded_keys.md.

At (n, k) = (4096, 2) and (8192, 3), dbc 16, with 22 and 512 Galois elements (3, 5, 7, ...):
(1) generation: crc_gen_keys_seeded_dev_key (HIP events, the rows stay on the device) per key, against crc_gen_galois_keys_key on the host threads (wall clock;
    that function is what every key set cost before this form existed).
(2) expansion: crc_seeded_keys_expand_dev in written bytes per second, beside crc_seeded_expand_dev on as many ciphertexts as write the same bytes (the same
    work under another nonce) and beside the crc_memcpy_h2d of the second halves that the expansion replaces (pageable host memory, as generateGaloisKeys uploads).
(3) conjugation: the one-pass form (conjugate = 1) against the composition crc_seeded_keys_expand_dev (conjugate = 0) + crc_galois_conjugate_keys_dev in a second
    buffer, alternating in one process: medians, and the spread of the composition itself -- the one-pass form stays only if it wins by more than that spread.
(4) the host classes end to end: installGaloisKeys (upload of the rows, both expansions) against generateGaloisKeys (host generation, upload, conjugation),
    by crcnn_amd/lib/seeded_keys_host's timing mode.

Outputs are checked equal (device against the host twin on the first keys, one-pass against composed conjugation on all) before anything is timed.  One process per
step, each under its own `timeout`, stopped at the first that fails:
    measure_seeded_keys.py                       the driver
    measure_seeded_keys.py step N K ELEMENTS     steps (1) - (3) of one shape, in process; prints one JSON line
Options: --rounds (7), --reps (5: the least number of calls in a timed window; short calls are repeated until the window is about 20 ms), --markdown FILE."""
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
SHAPES = [(4096, 2), (8192, 3)]
ELEMENTS = [22, 512]
DBC = 16
T = 65537
WINDOW_MS = 20.0
KEY = bytes(range(1, 33))
PUB = bytes(range(101, 133))


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


def wall_ms(E, fn):
    E.sync()
    t0 = time.perf_counter()
    fn()
    E.sync()
    return (time.perf_counter() - t0) * 1e3


def primes(n, k):
    import crcnn_amd as ca
    return (ca.default_coeff_modulus_128(n) if n == 4096 else ca.default_coeff_modulus_128(8192))[:k]


def step(n, k, elements, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = primes(n, k)
    E = ca.Engine(n, q, T, device=0)
    sk, _ = E.keygen(3)
    ids = np.array([2 * i + 3 for i in range(elements)], dtype=np.uint64)
    w = E.seeded_key_words(DBC)
    pairs = w // (k * n)
    d_sk = E.upload(sk)
    d_first = E.alloc(elements * w * 8)
    d_out, d_conj, d_tmp = (E.alloc(elements * 2 * w * 8) for _ in range(3))
    # correctness first: the first keys against the host twin, the two conjugations against each other on the whole set
    head = min(elements, 3)
    E.gen_keys_seeded_dev(0, d_sk, ids, d_first, dbc=DBC, key=KEY, public_seed=PUB)
    want, _ = E.gen_keys_seeded(0, sk, ids[:head], dbc=DBC, key=KEY, public_seed=PUB)
    eq_gen = bool(np.array_equal(E.download(d_first, (elements, w))[:head], want))
    E.seeded_keys_expand_dev(d_first, ids, PUB, d_out, dbc=DBC)
    eq_exp = bool(np.array_equal(E.download(d_out, (elements, 2 * w))[:head], E.seeded_keys_expand(want, ids[:head], PUB, dbc=DBC)))

    def composed():
        E.seeded_keys_expand_dev(d_first, ids, PUB, d_tmp, dbc=DBC)
        E.galois_conjugate_keys_dev(ids, d_tmp, d_conj, dbc=DBC)

    def one_pass():
        E.seeded_keys_expand_dev(d_first, ids, PUB, d_out, dbc=DBC, conjugate=True)
    composed(); one_pass()
    eq_conj = bool(np.array_equal(E.download(d_out, (elements, 2 * w)), E.download(d_conj, (elements, 2 * w))))
    # (2): the same bytes through the seeded ciphertext expansion, and the upload the expansion replaces
    cts = elements * pairs
    halves = np.zeros(elements * w, dtype=np.uint64)
    calls = {"generate": lambda: E.gen_keys_seeded_dev(0, d_sk, ids, d_first, dbc=DBC, key=KEY, public_seed=PUB),
             "expand": lambda: E.seeded_keys_expand_dev(d_first, ids, PUB, d_tmp, dbc=DBC),
             "seeded_ct_expand": lambda: E.seeded_expand_dev(d_first, cts, PUB, 0, ca.NTT, d_tmp),
             "conj_one_pass": one_pass, "conj_composed": composed}
    for fn in calls.values():
        fn()
    E.sync()
    # a timed window of a few calls of some tens of microseconds measures the clock and the scheduler: as many calls per window as fill about WINDOW_MS
    per_call = {nm: max(reps, min(2000, int(WINDOW_MS / max(events_ms(E, fn, 3), 1e-4)) + 1)) for nm, fn in calls.items()}
    ms = {nm: [] for nm in calls}
    ms["upload_second_halves"] = []; ms["host_generate"] = []
    for r in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, per_call[nm]))
        ms["upload_second_halves"].append(wall_ms(E, lambda: E.L.crc_memcpy_h2d(E.c, d_tmp.ptr, halves.ctypes.data, halves.nbytes, E.stream)))
        if r < 3:                                                        # (seconds per round at 512 elements: three rounds say enough)
            gk = np.zeros((elements, 2 * w), dtype=np.uint64)
            pu = ca.binding._pu
            ms["host_generate"].append(wall_ms(E, lambda: E.L.crc_gen_galois_keys_key(E.c, E._key(KEY), pu(sk), DBC, pu(ids), elements, pu(gk))))
    # the last thing the rows went through was `generate`: still the host twin's
    eq_gen = eq_gen and bool(np.array_equal(E.download(d_first, (elements, w))[:head], want))
    print(json.dumps(dict(n=n, k=k, elements=elements, pairs=pairs, blob_bytes=2 * w * 8, host_threads=os.environ.get("CRC_HOST_THREADS", "default"),
                          equal_gen=eq_gen, equal_expand=eq_exp, equal_conj=eq_conj, calls_per_window=per_call, ms=ms)), flush=True)
    E.close()
    return 0 if eq_gen and eq_exp and eq_conj else 3


def med(v):
    return statistics.median(v)


def spread(v):
    return (max(v) - min(v)) / med(v) if v else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver")
    ap.add_argument("args", nargs="*")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "seeded_keys.md"))
    a = ap.parse_args()
    if a.mode == "step":
        n, k, elements = (int(v) for v in a.args)
        return step(n, k, elements, a.rounds, a.reps)
    env = dict(os.environ); env.setdefault("CRC_HOST_THREADS", "16")
    rows, host = [], []
    for n, k in SHAPES:
        for elements in ELEMENTS:
            out = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "step", str(n), str(k), str(elements),
                                  "--rounds", str(a.rounds), "--reps", str(a.reps)], capture_output=True, text=True, env=env)
            sys.stderr.write(out.stderr[-2000:])
            if out.returncode:
                print(f"step {n} {k} {elements} failed with status {out.returncode}; stopping", file=sys.stderr)
                return out.returncode
            rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
            d = tempfile.mkdtemp()
            import numpy as np
            np.array([n, k, T] + [int(v) for v in primes(n, k)], dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
            out = subprocess.run(["timeout", "-k", "10", "420", os.path.join(ROOT, "crcnn_amd", "lib", "seeded_keys_host"), d, "time", str(elements), "3"],
                                 capture_output=True, text=True, env=env)
            if out.returncode or "seeded_keys_host time ok" not in out.stdout:
                print(f"host classes {n} {k} {elements} failed with status {out.returncode}: {out.stderr[-500:]}; stopping", file=sys.stderr)
                return out.returncode or 3
            t = [l.split() for l in out.stdout.splitlines() if l.startswith("time ")]
            host.append(dict(n=n, k=k, elements=elements, generate=[float(l[2]) for l in t], install=[float(l[4]) for l in t]))
            print(host[-1], flush=True)
    L = ["# Seeded key-switching keys on one MI355X", "",
         f"`tools/measure_seeded_keys.py --rounds {a.rounds} --reps {a.reps}`: dbc {DBC}, elements 3, 5, 7, ...; HIP events around at least {a.reps} calls (as many as fill {WINDOW_MS:.0f} ms), {a.rounds} rounds,",
         "the compared calls alternating in one process; medians, spread = (max - min) / median.  Device results equal the host twin and the two conjugations equal",
         "each other in every step (checked before timing).  Host generation ran on " + env["CRC_HOST_THREADS"] + " host threads.", "",
         "## Generation per key", "", "| n | k | elements | device us / key | spread | host (crc_gen_galois_keys_key) us / key | host / device |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        g, h = med(r["ms"]["generate"]) * 1e3 / r["elements"], med(r["ms"]["host_generate"]) * 1e3 / r["elements"]
        L.append(f"| {r['n']} | {r['k']} | {r['elements']} | {g:.1f} | {spread(r['ms']['generate']):.1%} | {h:.0f} | {h / g:.0f}x |")
    L += ["", "## Expansion (written bytes per second)", "",
          "| n | k | elements | blob bytes written | expand GB/s | spread | crc_seeded_expand_dev, same bytes GB/s | crc_memcpy_h2d of the second halves GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["elements"] * r["blob_bytes"]
        gb = lambda ms, bytes_=b: bytes_ / (ms * 1e-3) / 1e9
        L.append(f"| {r['n']} | {r['k']} | {r['elements']} | {b} | {gb(med(r['ms']['expand'])):.0f} | {spread(r['ms']['expand']):.1%} | "
                 f"{gb(med(r['ms']['seeded_ct_expand'])):.0f} | {gb(med(r['ms']['upload_second_halves']), b // 2):.1f} |")
    L += ["", "## Conjugated blobs: one pass against expand + crc_galois_conjugate_keys_dev", "",
          "| n | k | elements | one pass ms | composed ms | composed spread | one pass / composed | wins by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    keep = True
    for r in rows:
        o, c, s = med(r["ms"]["conj_one_pass"]), med(r["ms"]["conj_composed"]), spread(r["ms"]["conj_composed"])
        win = o < c * (1 - s)
        keep = keep and win
        L.append(f"| {r['n']} | {r['k']} | {r['elements']} | {o:.3f} | {c:.3f} | {s:.1%} | {o / c:.2f} | {'yes' if win else 'NO'} |")
    L += ["", ("The one-pass form wins at every shape by more than the composition's own spread: it is the form `crc_seeded_keys_expand_dev` keeps."
               if keep else "The one-pass form does NOT win everywhere by more than the composition's spread: the entry point should compose the two steps."), "",
          "## Host classes end to end (wall clock, both end in a stream synchronise)", "",
          "| n | k | elements | generateGaloisKeys ms | installGaloisKeys ms | ratio |", "|---|---|---|---|---|---|"]
    for h in host:
        g, i = med(h["generate"]), med(h["install"])
        L.append(f"| {h['n']} | {h['k']} | {h['elements']} | {g:.0f} | {i:.1f} | {g / i:.0f}x |")
    os.makedirs(os.path.dirname(a.markdown), exist_ok=True)
    with open(a.markdown, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", a.markdown)
    return 0


if __name__ == "__main__":
    sys.exit(main())
