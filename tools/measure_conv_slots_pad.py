#!/usr/bin/env python3
"""Measure the packed convolution with a bias and a mask against its composition and against the unmasked call on one GPU, and write profiles/conv_slots_pad.md.

    python tools/measure_conv_slots_pad.py [--out profiles/conv_slots_pad.md] [--calls 3] [--rounds 3] [--sets 0,1] [--append]

Per parameter set and layer shape (Cin -> Cout, T taps), count in (1, 16): HIP events, the candidates alternating `rounds` times in ONE process, median
(min, max) per call.  Coefficient form in and out, dbc = 16, the default conv_jt.
  * fused: one crc_conv_slots_bias_mask_forms call with a bias and a mask
  * composed: crc_conv_slots_forms into NTT form, crc_add_plain per output channel, crc_multiply_plain_ntt of all Cout count ciphertexts by the mask row, one
    inverse transform -- the definition of the fused call, from entry points the parent commit has
  * unmasked: crc_conv_slots_forms alone, which shows what the epilogue costs
Shapes at (8192, 3 moduli): ApproxPlainModel's real front on a 28 x 28 plane with M = 1024 -- conv1 (5 x 5, stride 2) + pool1 (window 2, stride 1) + bn1 as
1 -> 20 with the 49 taps of the planned 7 x 7 window and a bias, conv2 (3 x 3, stride 2) as 20 -> 50 with 9 taps at the dilation conv1 leaves.  At (4096, 2
moduli): a padded 3 x 3 'same' layer 32 -> 32 on a 28 x 28 plane with a margin of one.  The element lists are conv_slots_plan_geom's.
Times do not depend on the values of keys, weights, bias or mask: the key blobs are device copies of ONE generated key, the mask is the plan's own.
The last table is the noise budget of a 3 x 3 'same' layer 1 -> 2 (pad 1, real keys, a 12 x 12 image) at both parameter sets: after the layer with its bias,
and after the same layer with the mask.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_galois import fmt, timed  # noqa: E402

COUNTS = (1, 16)
SETS = ((8192, 3, 30), (4096, 2, 0))                                     # (n, moduli, bits of the slot prime; 0: 65537)


def shapes(n, which):
    """[(name, Cin, Cout, plan)]"""
    from crcnn_amd.binding import conv_slots_plan_geom
    if which == 0:
        p1 = conv_slots_plan_geom(n, 1024, 28, 0, 28, 28, 5, 5, 1, 0, 2, 2, 1)
        p2 = conv_slots_plan_geom(n, 1024, 28, 0, p1.out_h, p1.out_w, 3, 3, p1.out_dil, 0, 2)
        return [("ApproxPlainModel conv1 + pool1 + bn1", 1, 20, p1), ("ApproxPlainModel conv2", 20, 50, p2)]
    return [("3 x 3 'same' layer, pad 1, margin 1", 32, 32, conv_slots_plan_geom(n, 1024, 29, 30, 28, 28, 3, 3, 1, 1))]


def slot_prime(ca, n, bits):
    return ca.Engine.slots_prime(n, bits) if bits else 65537


def measure(which, n, k, bits, calls, rounds):
    import crcnn_amd as ca
    t = slot_prime(ca, n, bits)
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
    d_x = E.upload(x)
    rowb = k * n * 8; ctb = 2 * rowb
    d_y = E.alloc(cout_max * cmax * ctb)
    d_w = E.upload(H.conv_slots_pack_weights(rng.randint(-(t // 2), t // 2, size=(cout_max, cin_max, t_max))))
    bias = rng.randint(-(t // 2), t // 2, size=cout_max).astype(np.int64)
    consts = np.zeros((cout_max, n), dtype=np.uint64)
    consts[:, 0] = (bias % t).astype(np.uint64)
    d_delta = E.alloc(cout_max * rowb)
    E.plain_to_delta(E.upload(consts), cout_max, ca.NTT, d_delta)
    d_m = E.alloc(rowb)
    d_work = E.alloc(max(E.conv_slots_work_bytes(cmax, ci, co, len(pl.steps)) for _, ci, co, pl in layers))
    lines = [f"## n = {n}, {k} moduli, t = {t} (one key: {kb} bytes, one ciphertext: {ctb} bytes)", "",
             "| layer | Cin -> Cout, taps | count | composed | fused (bias + mask) | unmasked | fused / composed | fused / unmasked |",
             "|---|---|---|---|---|---|---|---|"]
    for name, Cin, Cout, plan in layers:
        gs, T = plan.elements, len(plan.steps)
        E.plain_to_ntt(E.upload(H.slots_compose(plan.mask_slots().reshape(1, n), 1, n, n, 1)), 1, d_m)
        d_b = E.upload(H.conv_slots_pack_bias(bias[:Cout]))
        for count in COUNTS:
            def unmasked(count=count, Cin=Cin, Cout=Cout, gs=gs):
                E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_y, d_work)

            def composed(count=count, Cin=Cin, Cout=Cout, gs=gs):
                E.conv_slots(d_x, count, Cin, gs, d_w, Cout, d_cg, elts, d_y, d_work, out_form=ca.NTT)
                for co in range(Cout):
                    E.add_plain(d_y.ptr + co * count * ctb, d_delta.ptr + co * rowb, count, count, 1)
                E.multiply_plain_ntt(d_y, d_m, Cout * count, Cout * count)
                E.ntt_inv(d_y, Cout * count)

            def fused(count=count, Cin=Cin, Cout=Cout, gs=gs, d_b=d_b):
                E.conv_slots_bias_mask(d_x, count, Cin, gs, d_w, Cout, d_b, d_m, d_cg, elts, d_y, d_work)
            r = {"composed": [], "fused": [], "unmasked": []}
            for _ in range(rounds):
                r["composed"].append(timed(E, composed, calls))
                r["fused"].append(timed(E, fused, calls))
                r["unmasked"].append(timed(E, unmasked, calls))
            med = {k_: statistics.median(v) for k_, v in r.items()}
            lines.append(f"| {name} | {Cin} -> {Cout}, {T} | {count} | {fmt(r['composed'])} | {fmt(r['fused'])} | {fmt(r['unmasked'])} | "
                         f"{med['fused'] / med['composed']:.4f} | {med['fused'] / med['unmasked']:.4f} |")
            print(lines[-1], flush=True)
    lines.append("")
    E.close(); H.close()
    return lines


def budgets(n, k, bits):
    """a 3 x 3 'same' layer 1 -> 2 with real keys on a 12 x 12 image (margin 1, M = 256): min budget of the fresh ciphertext, after the biased layer, after the
    biased and masked layer"""
    import crcnn_amd as ca
    from crcnn_amd.binding import conv_slots_plan_geom
    t = slot_prime(ca, n, bits)
    q = ca.binding.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    M = 256
    plan = conv_slots_plan_geom(n, M, 13, 14, 12, 12, 3, 3, 1, 1)
    sk, pk = H.keygen(5)
    elts, gk = H.gen_galois_keys(6, sk, elts=sorted(set(plan.elements) - {1}))
    d_cg = E.upload(H.galois_conjugate_keys(elts, gk)); d_sk = E.upload(sk)
    rng = np.random.RandomState(7)
    row = np.zeros(M, dtype=np.int64)
    row[plan.valid] = rng.randint(0, 4, size=144)                      # (a 'same' layer: the outputs sit where the pixels do)
    d_x = E.upload(H.encrypt(pk, H.slots_compose(np.tile(row, n // M).reshape(1, n), 1, n, n, 1), 8))
    w = rng.randint(-2, 3, size=(2, 1, 3, 3)).astype(np.int64)
    d_w = E.upload(H.conv_slots_pack_weights(plan.fold(w, t))); d_b = E.upload(H.conv_slots_pack_bias(np.array([3, -3])))
    d_m = E.alloc(k * n * 8)
    E.plain_to_ntt(E.upload(H.slots_compose(plan.mask_slots().reshape(1, n), 1, n, n, 1)), 1, d_m)
    d_y = E.alloc(2 * 2 * k * n * 8); d_work = E.alloc(E.conv_slots_work_bytes(1, 1, 2, 9))
    d_bits = E.alloc(2 * 4); d_bw = E.alloc(E.noise_budget_dev_work_bytes(2))

    def budget(d, count):
        E.noise_budget_dev(d_sk, d, count, d_bits, d_bw)
        return min(E.download(d_bits, (count,), dtype=np.int32).tolist())
    fresh = budget(d_x, 1)
    E.conv_slots_bias_mask(d_x, 1, 1, plan.elements, d_w, 2, d_b, None, d_cg, elts, d_y, d_work)
    biased = budget(d_y, 2)
    E.conv_slots_bias_mask(d_x, 1, 1, plan.elements, d_w, 2, d_b, d_m, d_cg, elts, d_y, d_work)
    masked = budget(d_y, 2)
    E.close(); H.close()
    line = f"| {n}, {k} moduli, t = {t} | {fresh} | {biased} | {masked} | {biased - masked} |"
    print(line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_slots_pad.md"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="0,1")
    ap.add_argument("--append", action="store_true", help="add the chosen sets' tables to an existing file (a run per parameter set)")
    a = ap.parse_args()
    out = [] if a.append else [
        "# Packed convolution with a bias and a mask: measurements", "",
        f"tools/measure_conv_slots_pad.py on one GPU: HIP events, candidates alternating {a.rounds} times in one process, median (min, max) per call ({a.calls} calls "
        "per timing).  Coefficient form in and out, dbc = 16, the default conv_jt.  `fused`: one crc_conv_slots_bias_mask_forms call with a bias and a mask; "
        "`composed`: crc_conv_slots_forms into NTT form, crc_add_plain per output channel, crc_multiply_plain_ntt by the mask row, one inverse transform -- the "
        "fused call's definition, driven through the same binding in the same run; `unmasked`: crc_conv_slots_forms alone.  Key blobs are device copies of one "
        "generated key, weights and bias random, the mask the plan's own: times do not depend on their values.", ""]
    which = [int(v) for v in a.sets.split(",")]
    for i in which:
        out += measure(i, *SETS[i], a.calls, a.rounds)
    out += ["## Noise budget before and after the mask", "",
            "A 3 x 3 'same' layer 1 -> 2 (pad 1) with real keys on a 12 x 12 image with a margin of one, M = 256; the smallest budget over the ciphertexts, in bits.", "",
            "| parameters | fresh | after the layer with its bias | after the same layer with the mask | the mask costs |", "|---|---|---|---|---|"]
    out += [budgets(*SETS[i]) for i in which] + [""]
    text = "\n".join(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
