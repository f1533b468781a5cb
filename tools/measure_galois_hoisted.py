#!/usr/bin/env python3
"""Measure the hoisted rotations and the diagonal product on one GPU and write profiles/galois_hoisted.md.

    python tools/measure_galois_hoisted.py [--out profiles/galois_hoisted.md] [--calls 10] [--rounds 3]

Per parameter set ((4096, 2 moduli), (8192, 3 moduli)), count in (1, 1024), R in (1, 8, 32): HIP events around `calls` calls, the candidates alternating
`rounds` times in ONE process, median (min, max) per call.
  * one crc_rotate_hoisted_forms of R elements, with one key per digit load (hoist_rt = 1) and with two (hoist_rt = 2), against R calls of
    crc_apply_galois_forms with the direct keys of the same elements -- code the hoisted rotations do not touch
  * crc_diag_mac_forms against its composed form: crc_rotate_hoisted_forms, then crc_multiply_plain_ntt per element, then crc_add
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_galois import alternate, fmt  # noqa: E402


def measure(n, k, t, counts, Rs, calls, rounds):
    import crcnn_amd as ca
    q = ca.binding.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(1)
    Rmax = max(Rs)
    gs_all = [int(E.galois_elt_rows(s)) for s in range(1, Rmax + 1)]
    elts, gk = H.gen_galois_keys(2, sk, elts=gs_all)
    d_gk = E.upload(gk); d_cg = E.alloc(gk.nbytes)
    E.galois_conjugate_keys_dev(elts, d_gk, d_cg)
    rng = np.random.RandomState(n)
    cmax = max(counts)
    x = np.stack([(rng.randint(0, 1 << 62, size=(cmax, 2, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=2)
    p = np.stack([(rng.randint(0, 1 << 62, size=(Rmax, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=1)
    d_x = E.upload(x); d_p = E.upload(p)
    d_xn = E.upload(x); E.ntt_fwd(d_xn, cmax)
    ctb = 2 * k * n * 8
    d_rot = E.alloc(Rmax * cmax * ctb); d_y = E.alloc(cmax * ctb)
    d_w = E.alloc(max(E.apply_galois_work_bytes(cmax), max(E.rotate_hoisted_work_bytes(cmax, R) for R in Rs), max(E.diag_mac_work_bytes(cmax, R) for R in Rs)))
    lines = [f"## n = {n}, {k} moduli", "",
             "| count | R | R x apply_galois | hoisted, 1 key / load | hoisted, 2 keys / load | hoisted / sequential (1, 2) | NTT form: R x apply_galois | NTT form: hoisted | ratio | diag_mac | composed | diag_mac / composed |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for count in counts:
        for R in Rs:
            gs = gs_all[:R]

            def sequential():
                for g in gs:
                    E.apply_galois(d_x, count, g, d_gk, elts, d_y, d_w)

            def hoisted(rt):
                E.set_tuning("hoist_rt", rt)
                E.rotate_hoisted(d_x, count, gs, d_cg, elts, d_rot, d_w, out_form=ca.COEFF)
                E.set_tuning("hoist_rt", 0)

            def composed():
                E.rotate_hoisted(d_x, count, gs, d_cg, elts, d_rot, d_w, out_form=ca.NTT)
                for r in range(R):
                    E.multiply_plain_ntt(d_rot.ptr + r * count * ctb, d_p.ptr + r * k * n * 8, count, count)
                    if r:
                        E.add(d_rot, d_rot.ptr + r * count * ctb, count)
                E.ntt_inv(d_rot, count)

            def sequential_ntt():
                for g in gs:
                    E.apply_galois(d_xn, count, g, d_gk, elts, d_y, d_w, in_form=ca.NTT, out_form=ca.NTT)

            fns = {"seq_ntt": sequential_ntt,
                   "hoisted_ntt": lambda: E.rotate_hoisted(d_xn, count, gs, d_cg, elts, d_rot, d_w, in_form=ca.NTT, out_form=ca.NTT),
                   "seq": sequential, "rt1": lambda: hoisted(1), "rt2": lambda: hoisted(2),
                   "diag": lambda: E.diag_mac(d_x, count, gs, d_p, d_cg, elts, d_y, d_w), "composed": composed}
            r = alternate(E, fns, calls, rounds)
            med = {k_: statistics.median(v) for k_, v in r.items()}
            lines.append(f"| {count} | {R} | {fmt(r['seq'])} | {fmt(r['rt1'])} | {fmt(r['rt2'])} | {med['rt1'] / med['seq']:.3f}, {med['rt2'] / med['seq']:.3f} | "
                         f"{fmt(r['seq_ntt'])} | {fmt(r['hoisted_ntt'])} | {med['hoisted_ntt'] / med['seq_ntt']:.3f} | "
                         f"{fmt(r['diag'])} | {fmt(r['composed'])} | {med['diag'] / med['composed']:.3f} |")
            print(lines[-1], flush=True)
    E.close(); H.close()
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "galois_hoisted.md"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import crcnn_amd as ca
    out = ["# Hoisted rotations and the diagonal product: measurements", "",
           f"tools/measure_galois_hoisted.py on one GPU: HIP events around {a.calls} calls, candidates alternating {a.rounds} times in one process, median (min, max) "
           "per call.  Coefficient form in and out unless a column says NTT form (both sides, the default hoist_rt), dbc = 16.  `R x apply_galois`: R calls of crc_apply_galois_forms with direct keys (one step each); `hoisted`: one "
           "crc_rotate_hoisted_forms of the same R elements with the tuning key hoist_rt = 1 / 2; `composed`: crc_rotate_hoisted_forms, crc_multiply_plain_ntt per "
           "element, crc_add.", ""]
    for n, k, t in ((4096, 2, 65537), (8192, 3, ca.Engine.slots_prime(8192, 30))):
        out += measure(n, k, t, (1, 1024), (1, 8, 32), a.calls, a.rounds)
    text = "\n".join(out)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
