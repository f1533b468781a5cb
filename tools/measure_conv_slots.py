#!/usr/bin/env python3
"""Measure the packed convolution over slots against its cheapest composition from the other entry points on one GPU and write profiles/conv_slots.md.

    python tools/measure_conv_slots.py [--out profiles/conv_slots.md] [--calls 3] [--rounds 3] [--sets 0,1] [--append]

Per parameter set and layer shape (Cin -> Cout, T taps), count in (1, 16): HIP events, the candidates alternating `rounds` times in ONE process, median
(min, max) per call.  Coefficient form in and out, dbc = 16.
  * fused: one crc_conv_slots_forms call, at every setting of the tuning key conv_jt (2, 4, 8 output channels per thread)
  * composed: per input channel one crc_rotate_hoisted_forms into NTT form (one digit decomposition and one key switch per tap, as in the fused call), then per
    (output channel, tap) a copy of the rotated ciphertexts, crc_multiply_plain_ntt on the copy (the entry point works in place) and crc_add, then one inverse
    transform: Cout Cin T products of a whole row each.  One call per round (it is thousands of launches), through the same Python binding as the fused call.
Shapes at (4096, 2 moduli): PlainModelTiny on a 28 x 28 plane with M = 1024 -- conv1 + pool1 as 1 -> 32 with the 36 taps of the planned 6 x 6 window, conv2 +
pool2 as 32 -> 64 with 36 taps at dilation 2 (the real element lists of conv_slots_plan).  At (8192, 3 moduli): ApproxPlainModel's channel and tap counts -- conv1
+ pool1 as 1 -> 20 with a 7 x 7 window (49 taps), conv2 as 20 -> 50 with 9 taps.  Its convolutions have stride 2, which the planner does not offer: those rows
time the operation at that size, not a plan of that network.
Times do not depend on the values of keys, weights or plaintext rows: the key blobs are device copies of ONE generated key, the composed form's plaintext rows
are T random rows used for every channel pair (Cout Cin T of them would be gigabytes).
The last table sets one whole packed image (upload of its one ciphertext, conv1 and conv2 fused at the default setting) beside the composed form of the same.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_galois import fmt, timed  # noqa: E402

COUNTS = (1, 16)
JTS = (2, 4, 8)


def shapes(n, which):
    """[(name, Cin, Cout, plan)]"""
    from crcnn_amd.binding import conv_slots_plan
    if which == 0:
        p1 = conv_slots_plan(n, 1024, 28, 28, 28, 5, 5, 1, 2)
        p2 = conv_slots_plan(n, 1024, 28, p1.out_h, p1.out_w, 5, 5, p1.out_dil, 2)
        return [("PlainModelTiny conv1 + pool1", 1, 32, p1), ("PlainModelTiny conv2 + pool2", 32, 64, p2)]
    return [("ApproxPlainModel conv1 + pool1 (size only)", 1, 20, conv_slots_plan(n, 1024, 28, 28, 28, 7, 7)),
            ("ApproxPlainModel conv2 (size only)", 20, 50, conv_slots_plan(n, 1024, 28, 28, 28, 3, 3))]


def measure(which, n, k, t, calls, rounds):
    import crcnn_amd as ca
    q = ca.binding.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(1)
    layers = shapes(n, which)
    all_elts = sorted({e for _, _, _, p in layers for e in p.elements} - {1})
    elts = np.array(all_elts, dtype=np.uint64)
    _, one = H.gen_galois_keys(2, sk, elts=[all_elts[0]])
    kb = one.nbytes
    d_cg = E.alloc(kb * elts.size); d_one = E.upload(one)
    for e in range(elts.size):
        E.copy_d2d(d_cg.ptr + e * kb, d_one, kb)
    cmax = max(COUNTS)
    cin_max = max(l[1] for l in layers); cout_max = max(l[2] for l in layers); t_max = max(len(l[3].steps) for l in layers)
    rng = np.random.RandomState(n)
    x = np.stack([(rng.randint(0, 1 << 62, size=(cin_max * cmax, 2, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=2)
    p = np.stack([(rng.randint(0, 1 << 62, size=(t_max, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=1)
    d_x = E.upload(x); d_p = E.upload(p)
    rowb = k * n * 8; ctb = 2 * rowb
    d_y = E.alloc(cout_max * cmax * ctb); d_rot = E.alloc(t_max * cmax * ctb); d_tmp = E.alloc(cmax * ctb)
    d_w = E.upload(H.conv_slots_pack_weights(rng.randint(-(t // 2), t // 2, size=(cout_max, cin_max, t_max))))
    d_work = E.alloc(max([E.conv_slots_work_bytes(cmax, ci, co, len(pl.steps)) for _, ci, co, pl in layers] + [E.rotate_hoisted_work_bytes(cmax, t_max)]))
    lines = [f"## n = {n}, {k} moduli (one key: {kb} bytes, one ciphertext: {ctb} bytes)", "",
             "| layer | Cin -> Cout, taps | count | composed | fused, conv_jt = 2 | conv_jt = 4 | conv_jt = 8 | fastest fused / composed |",
             "|---|---|---|---|---|---|---|---|"]
    image = {"fused": 0.0, "composed": 0.0}
    for name, Cin, Cout, plan in layers:
        gs, T = plan.elements, len(plan.steps)
        for count in COUNTS:
            def composed(count=count, Cin=Cin, Cout=Cout, gs=gs, T=T):
                for ci in range(Cin):
                    E.rotate_hoisted(d_x.ptr + ci * count * ctb, count, gs, d_cg, elts, d_rot, d_work, out_form=ca.NTT)
                    for co in range(Cout):
                        yo = d_y.ptr + co * count * ctb
                        for tau in range(T):
                            dst = yo if ci == 0 and tau == 0 else d_tmp.ptr
                            E.copy_d2d(dst, d_rot.ptr + tau * count * ctb, count * ctb)
                            E.multiply_plain_ntt(dst, d_p.ptr + tau * rowb, count, count)
                            if dst != yo:
                                E.add(yo, dst, count)
                E.ntt_inv(d_y, Cout * count)

            def fused(count=count, Cin=Cin, Cout=Cout, gs=gs):
                E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_y, d_work)
            r = {"composed": []}
            r.update({jt: [] for jt in JTS})
            for _ in range(rounds):
                r["composed"].append(timed(E, composed, 1))
                for jt in JTS:
                    E.set_tuning("conv_jt", jt)
                    r[jt].append(timed(E, fused, calls))
                    E.set_tuning("conv_jt", 0)
            med = {k_: statistics.median(v) for k_, v in r.items()}
            best = min(JTS, key=lambda jt: med[jt])
            lines.append(f"| {name} | {Cin} -> {Cout}, {T} | {count} | {fmt(r['composed'])} | {fmt(r[2])} | {fmt(r[4])} | {fmt(r[8])} | "
                         f"{med[best] / med['composed']:.4f} (conv_jt = {best}) |")
            print(lines[-1], flush=True)
            if count == 1:
                E.set_tuning("conv_jt", 0)
                image["fused"] += statistics.median([timed(E, fused, calls) for _ in range(rounds)])
                image["composed"] += med["composed"]
    ups = []
    for _ in range(5):
        E.sync(); t0 = time.perf_counter(); E.upload(x[:1]); E.sync(); ups.append((time.perf_counter() - t0) * 1e3)
    lines += ["", f"One packed image through both layers at count = 1 (default conv_jt): upload of its one ciphertext ({ctb} bytes; {ctb // 2} as a seeded c0 row) "
              f"{statistics.median(ups):.3f} ms (host clock, synchronised) + fused {image['fused']:.3f} ms = {statistics.median(ups) + image['fused']:.3f} ms; "
              f"the composed form of the same two layers {image['composed']:.3f} ms.", ""]
    print(lines[-2], flush=True)
    E.close(); H.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_slots.md"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="0,1")
    ap.add_argument("--append", action="store_true", help="add the chosen sets' tables to an existing file (a run per parameter set)")
    a = ap.parse_args()
    import crcnn_amd as ca
    out = [] if a.append else [
        "# Packed convolution over slots: measurements", "",
        f"tools/measure_conv_slots.py on one GPU: HIP events, candidates alternating {a.rounds} times in one process, median (min, max) per call ({a.calls} calls per "
        "timing of the fused form, 1 of the composed form).  Coefficient form in and out, dbc = 16.  `fused`: one crc_conv_slots_forms call at the tuning key "
        "conv_jt = 2 / 4 / 8; `composed`: crc_rotate_hoisted_forms per input channel into NTT form, then a copy, crc_multiply_plain_ntt and crc_add per (output "
        "channel, tap), one inverse transform -- entry points the parent commit has, driven through the same binding in the same run.  Key blobs are device "
        "copies of one generated key, weights and rows random: times do not depend on their values.", ""]
    sets = ((4096, 2, 65537), (8192, 3, ca.Engine.slots_prime(8192, 30)))
    for i in (int(v) for v in a.sets.split(",")):
        out += measure(i, *sets[i], a.calls, a.rounds)
    text = "\n".join(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
