#!/usr/bin/env python3
"""Measure the baby-step / giant-step diagonal product against the flat one on one GPU and write profiles/matvec_bsgs.md.

    python tools/measure_matvec_bsgs.py [--out profiles/matvec_bsgs.md] [--calls 3] [--rounds 3] [--sets 0,1] [--append]

Per parameter set ((4096, 2 moduli), (8192, 3 moduli)), M in (64, 256, 1024), count in (1, 64): HIP events around `calls` calls, the candidates alternating
`rounds` times in ONE process, median (min, max) per call.  Coefficient form in and out, dbc = 16, a dense M x M product: M plaintext rows either way.
  * crc_diag_mac_forms with its M - 1 keyed elements against crc_diag_mac_bsgs_forms at every power of two B from sqrt(M) / 2 to 2 sqrt(M), with the inner
    sums by galois_diag_mac_multi_kernel (bsgs_jt = 2) and, at the B nearest sqrt(M), by one galois_diag_mac_kernel launch per giant index (bsgs_jt = 1)
  * the inner sums alone: the same call on an NTT-form input with every element 1 in both lists -- no key switch, no digits, only the inner sums and the
    final sum kernel -- at bsgs_jt = 2 and 1; their difference is the multi kernel against G launches of the existing kernel on the same operands
Times do not depend on the values of keys or plaintext rows: the rows are random canonical residues and the key blobs are device copies of ONE generated key
(M - 1 real keys at (8192, 3) would take minutes to generate); the element lists are the real ones.
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

MS = (64, 256, 1024)
COUNTS = (1, 64)


def splits(M):
    r = 1 << ((M.bit_length() - 1) // 2)                              # sqrt(M): M is an even power of two here
    return [b for b in (r // 2, r, 2 * r) if 1 <= b <= M]


def alternate(E, cands, calls, rounds):
    """{name: [ms per round]}; a candidate is (tuning value of bsgs_jt, function).  The key is set outside the timed region (set_tuning synchronises)"""
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (jt, fn) in cands.items():
            E.set_tuning("bsgs_jt", jt)
            out[k].append(timed(E, fn, calls))
            E.set_tuning("bsgs_jt", 0)
    return out


def measure(n, k, t, calls, rounds):
    import crcnn_amd as ca
    q = ca.binding.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, _ = H.keygen(1)
    Mmax, cmax = max(MS), max(COUNTS)
    steps = [int(E.galois_elt_rows(s)) for s in range(Mmax)]           # steps[0] = 1
    elts = np.array(steps[1:], dtype=np.uint64)
    _, one = H.gen_galois_keys(2, sk, elts=[steps[1]])
    kb = one.nbytes
    d_cg = E.alloc(kb * elts.size)
    d_one = E.upload(one)
    for e in range(elts.size):
        E.copy_d2d(d_cg.ptr + e * kb, d_one, kb)
    rng = np.random.RandomState(n)
    x = np.stack([(rng.randint(0, 1 << 62, size=(cmax, 2, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=2)
    p = np.stack([(rng.randint(0, 1 << 62, size=(Mmax, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=1)
    d_x = E.upload(x); d_p = E.upload(p)
    d_xn = E.upload(x); E.ntt_fwd(d_xn, cmax)
    ctb = 2 * k * n * 8
    d_y = E.alloc(cmax * ctb)
    need = [E.diag_mac_work_bytes(cmax, M) for M in MS] + [E.diag_mac_bsgs_work_bytes(cmax, B, M // B) for M in MS for B in splits(M)]
    d_w = E.alloc(max(need))
    lines = [f"## n = {n}, {k} moduli (one key: {kb} bytes)", "",
             "| M | count | flat: keys, bytes | flat | B x G | BSGS: keys, bytes | BSGS | BSGS / flat | BSGS, one launch per giant index | inner sums alone: multi kernel | G launches | multi / launches |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for M in MS:
        for count in COUNTS:
            cands = {"flat": (0, lambda: E.diag_mac(d_x, count, steps[:M], d_p, d_cg, elts, d_y, d_w))}
            mid = splits(M)[len(splits(M)) // 2] if len(splits(M)) == 3 else splits(M)[0]
            for B in splits(M):
                G = M // B
                gb, gg = steps[:B], [steps[B * j] for j in range(G)]
                cands[f"bsgs{B}"] = (2, lambda gb=gb, gg=gg: E.diag_mac_bsgs(d_x, count, gb, gg, d_p, d_cg, elts, d_y, d_w))
                if B == mid:
                    cands["single"] = (1, lambda gb=gb, gg=gg: E.diag_mac_bsgs(d_x, count, gb, gg, d_p, d_cg, elts, d_y, d_w))
                    for name, jt in (("sums_multi", 2), ("sums_single", 1)):
                        cands[name] = (jt, lambda B=B, G=G: E.diag_mac_bsgs(d_xn, count, [1] * B, [1] * G, d_p, None, [], d_y, d_w, in_form=ca.NTT, out_form=ca.NTT))
            r = alternate(E, cands, calls, rounds)
            med = {k_: statistics.median(v) for k_, v in r.items()}
            for B in splits(M):
                G = M // B
                nk = B + G - 2
                at_mid = B == mid
                lines.append(f"| {M} | {count} | {M - 1}, {(M - 1) * kb} | {fmt(r['flat'])} | {B} x {G} | {nk}, {nk * kb} | {fmt(r[f'bsgs{B}'])} | "
                             f"{med[f'bsgs{B}'] / med['flat']:.3f} | {fmt(r['single']) if at_mid else ''} | {fmt(r['sums_multi']) if at_mid else ''} | "
                             f"{fmt(r['sums_single']) if at_mid else ''} | {'%.3f' % (med['sums_multi'] / med['sums_single']) if at_mid else ''} |")
                print(lines[-1], flush=True)
    E.close(); H.close()
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matvec_bsgs.md"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="0,1")
    ap.add_argument("--append", action="store_true", help="add the chosen sets' tables to an existing file (a run per parameter set)")
    a = ap.parse_args()
    import crcnn_amd as ca
    out = [] if a.append else [
        "# Baby-step / giant-step matrix-vector product over slots: measurements", "",
        f"tools/measure_matvec_bsgs.py on one GPU: HIP events around {a.calls} calls, candidates alternating {a.rounds} times in one process, median (min, max) per "
        "call.  Coefficient form in and out, dbc = 16, a dense M x M product.  `flat`: crc_diag_mac_forms with M - 1 keyed elements; `BSGS`: "
        "crc_diag_mac_bsgs_forms at the split B x G with B + G - 2 keyed elements (bsgs_jt = 2, galois_diag_mac_multi_kernel); `one launch per giant index`: "
        "the same call at bsgs_jt = 1 (G launches of galois_diag_mac_kernel), at the middle split only; `inner sums alone`: the call on an NTT-form input with "
        "every element 1 -- no key switch, only the inner sums and the final sum kernel -- at both settings.  Key blobs are device copies of one generated key "
        "and the rows random residues: times do not depend on their values.", ""]
    sets = ((4096, 2, 65537), (8192, 3, ca.Engine.slots_prime(8192, 30)))
    for i in (int(v) for v in a.sets.split(",")):
        out += measure(*sets[i], a.calls, a.rounds)
    text = "\n".join(out)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
