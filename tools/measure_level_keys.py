#!/usr/bin/env python3
"""Key-switching keys of a derived level priced on one MI355X -> profiles/level_keys.md.

At (n, k -> k') = (4096, 3 -> 2) and (8192, 3 -> 2), dbc 16, with 22 and 512 Galois elements (3, 5, 7, ...):
(1) restriction: crc_keys_restrict_dev (HIP events) per key and in moved bytes per second (read + written = twice the level's blobs), beside crc_add on as many
    parent ciphertexts as move the same bytes (two reads and a write each), in the same process.
(2) device derivation against host regeneration: the restriction time of (1) beside what the parent commit needs for keys at the level -- crc_gen_galois_keys_key
    on the plain prefix context on the host threads plus the upload of the blobs (wall clock, pageable host memory).
(3) the fused seeded route: crc_seeded_keys_expand_level_dev against the composition crc_seeded_keys_expand_dev at the parent + crc_keys_restrict_dev, alternating
    in one process: medians, and the spread of the composition itself -- the fused form stays only where it wins by more than that spread.

Outputs are checked equal (device restriction against the host twin on the first keys, fused against composed on all) before anything is timed.  One process per
step, each under its own `timeout`, stopped at the first that fails:
    measure_level_keys.py                            the driver
    measure_level_keys.py step N K KEPT ELEMENTS     one shape, in process; prints one JSON line
Options: --rounds (7), --reps (5: the least number of calls in a timed window; short calls are repeated until the window is about 20 ms), --markdown FILE."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from measure_seeded_keys import DBC, KEY, PUB, T, WINDOW_MS, events_ms, wall_ms       # noqa: E402  (one timing method for both profiles)

SHAPES = [(4096, 3, 2), (8192, 3, 2)]
ELEMENTS = [22, 512]


def primes(n, k):
    import crcnn_amd as ca
    out = []
    for m in (n, 8192, 16384):
        if m >= n:
            out += [p for p in ca.default_coeff_modulus_128(m) if p not in out]
    return out[:k]


def step(n, k, kept, elements, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = primes(n, k)
    A = ca.Engine(n, q, T, device=0); B = A.derived_level(kept); C = A.level(kept)
    sk, _ = A.keygen(3)
    skB = np.ascontiguousarray(sk[:kept])
    ids = np.array([2 * i + 3 for i in range(elements)], dtype=np.uint64)
    rw, wA, wB = A.seeded_key_words(DBC), A.L.crc_evk_words(A.c, DBC), B.L.crc_evk_words(B.c, DBC)
    d_first = A.alloc(elements * rw * 8)
    d_blobs = A.alloc(elements * wA * 8)
    d_low, d_fused = A.alloc(elements * wB * 8), A.alloc(elements * wB * 8)
    A.gen_keys_seeded_dev(0, A.upload(sk), ids, d_first, dbc=DBC, key=KEY, public_seed=PUB)
    A.seeded_keys_expand_dev(d_first, ids, PUB, d_blobs, dbc=DBC)

    def restrict():
        A.keys_restrict_dev(B, d_blobs, elements, d_low, dbc=DBC)

    def composed():
        A.seeded_keys_expand_dev(d_first, ids, PUB, d_blobs, dbc=DBC)
        A.keys_restrict_dev(B, d_blobs, elements, d_low, dbc=DBC)

    def fused():
        A.seeded_keys_expand_level_dev(B, d_first, ids, PUB, d_fused, dbc=DBC)
    # correctness first: the first keys against the host twin, fused against composed on the whole set
    head = min(elements, 3)
    composed(); fused()
    low = A.download(d_low, (elements, wB))
    eq_restrict = bool(np.array_equal(low[:head], A.keys_restrict(B, A.download(d_blobs, (head, wA)), dbc=DBC)))
    eq_fused = bool(np.array_equal(A.download(d_fused, (elements, wB)), low))
    del low
    # crc_add on the bytes the restriction moves: one ciphertext is two reads and a write of 2 k n words
    ct_bytes = 2 * k * n * 8
    moved = 2 * elements * wB * 8
    cts = max(1, moved // (3 * ct_bytes))
    d_x, d_y = A.alloc(cts * ct_bytes), A.alloc(cts * ct_bytes)
    A.L.crc_memset(A.c, d_x.ptr, 0, cts * ct_bytes, A.stream); A.L.crc_memset(A.c, d_y.ptr, 0, cts * ct_bytes, A.stream)
    calls = {"restrict": restrict, "add_same_bytes": lambda: A.add(d_x, d_y, cts), "fused": fused, "composed": composed}
    for fn in calls.values():
        fn()
    A.sync()
    per_call = {nm: max(reps, min(2000, int(WINDOW_MS / max(events_ms(A, fn, 3), 1e-4)) + 1)) for nm, fn in calls.items()}
    ms = {nm: [] for nm in calls}
    ms["host_generate"] = []; ms["upload"] = []
    pu = ca.binding._pu
    for r in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(A, fn, per_call[nm]))
        if r < 3:                                                        # (seconds per round at 512 elements: three rounds say enough)
            gk = np.zeros((elements, wB), dtype=np.uint64)
            ms["host_generate"].append(wall_ms(C, lambda: C.L.crc_gen_galois_keys_key(C.c, C._key(KEY), pu(skB), DBC, pu(ids), elements, pu(gk))))
            ms["upload"].append(wall_ms(C, lambda: C.L.crc_memcpy_h2d(C.c, d_low.ptr, gk.ctypes.data, gk.nbytes, C.stream)))
    print(json.dumps(dict(n=n, k=k, kept=kept, elements=elements, parent_blob_bytes=wA * 8, level_blob_bytes=wB * 8, add_cts=cts, add_bytes=3 * cts * ct_bytes,
                          host_threads=os.environ.get("CRC_HOST_THREADS", "default"), equal_restrict=eq_restrict, equal_fused=eq_fused, calls_per_window=per_call,
                          ms=ms)), flush=True)
    for e in (A, B, C):
        e.close()
    return 0 if eq_restrict and eq_fused else 3


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
    ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "level_keys.md"))
    a = ap.parse_args()
    if a.mode == "step":
        n, k, kept, elements = (int(v) for v in a.args)
        return step(n, k, kept, elements, a.rounds, a.reps)
    env = dict(os.environ); env.setdefault("CRC_HOST_THREADS", "16")
    rows = []
    for n, k, kept in SHAPES:
        for elements in ELEMENTS:
            out = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "step", str(n), str(k), str(kept), str(elements),
                                  "--rounds", str(a.rounds), "--reps", str(a.reps)], capture_output=True, text=True, env=env)
            sys.stderr.write(out.stderr[-2000:])
            if out.returncode:
                print(f"step {n} {k} {kept} {elements} failed with status {out.returncode}; stopping", file=sys.stderr)
                return out.returncode
            rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
    L = ["# Key-switching keys of a derived level on one MI355X", "",
         f"`tools/measure_level_keys.py --rounds {a.rounds} --reps {a.reps}`: dbc {DBC}, elements 3, 5, 7, ...; HIP events around at least {a.reps} calls (as many as fill {WINDOW_MS:.0f} ms), {a.rounds} rounds,",
         "the compared calls alternating in one process; medians, spread = (max - min) / median.  The device restriction equals the host twin and the fused seeded",
         "route equals the composition in every step (checked before timing).  Host generation ran on " + env["CRC_HOST_THREADS"] + " host threads.", "",
         "## Restriction (moved bytes = read + written = twice the level's blobs)", "",
         "| n | k -> k' | elements | level blob bytes | restrict us / key | spread | restrict GB/s | crc_add, same bytes GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        t = med(r["ms"]["restrict"])
        L.append(f"| {r['n']} | {r['k']} -> {r['kept']} | {r['elements']} | {r['level_blob_bytes']} | {t * 1e3 / r['elements']:.2f} | {spread(r['ms']['restrict']):.1%} | "
                 f"{2 * r['elements'] * r['level_blob_bytes'] / (t * 1e-3) / 1e9:.0f} | {r['add_bytes'] / (med(r['ms']['add_same_bytes']) * 1e-3) / 1e9:.0f} |")
    L += ["", "At 22 elements the moved bytes (46 and 92 MB) stay inside the 256 MiB last-level cache from call to call: those rows are cache rates, for both calls alike;",
          "512 elements (1.1 and 2.1 GB) stream from HBM."]
    L += ["", "## Keys for the level: restriction on the device against regeneration on the host", "",
          "| n | k -> k' | elements | restrict ms | crc_gen_galois_keys_key at the level ms | upload ms | host route / device |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        t, g, u = med(r["ms"]["restrict"]), med(r["ms"]["host_generate"]), med(r["ms"]["upload"])
        L.append(f"| {r['n']} | {r['k']} -> {r['kept']} | {r['elements']} | {t:.3f} | {g:.0f} | {u:.1f} | {(g + u) / t:.0f}x |")
    L += ["", "## Seeded rows into a level: fused against expand at the parent + restrict", "",
          "| n | k -> k' | elements | fused ms | composed ms | composed spread | fused / composed | wins by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    keep = True
    for r in rows:
        o, c, s = med(r["ms"]["fused"]), med(r["ms"]["composed"]), spread(r["ms"]["composed"])
        win = o < c * (1 - s)
        keep = keep and win
        L.append(f"| {r['n']} | {r['k']} -> {r['kept']} | {r['elements']} | {o:.3f} | {c:.3f} | {s:.1%} | {o / c:.2f} | {'yes' if win else 'NO'} |")
    L += ["", ("The fused form wins at every shape by more than the composition's own spread: it is the form `crc_seeded_keys_expand_level_dev` keeps."
               if keep else "The fused form does NOT win everywhere by more than the composition's spread: the entry point should compose the two steps there.")]
    os.makedirs(os.path.dirname(a.markdown), exist_ok=True)
    with open(a.markdown, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", a.markdown)
    return 0


if __name__ == "__main__":
    sys.exit(main())
