#!/usr/bin/env python3
"""Measure the Galois entry points on one GPU and write profiles/galois.md.

    python tools/measure_galois.py [--out profiles/galois.md] [--count 1024] [--calls 10] [--rounds 3]

Per parameter set ((4096, 2 moduli), (8192, 3 moduli)): HIP events around `calls` calls, the candidates alternating `rounds` times in ONE process, median and
spread of the per-call times over the rounds.
  * crc_apply_galois_forms (one step, g = 3) against crc_relinearize on the same size-3 tensor -- relinearisation's kernels are not changed by the Galois work,
    which makes it a baseline that is not the code under test; expected: relinearise plus one pass of 5 k n 8 bytes per ciphertext
  * galois_permute_kernel alone (crc_galois_permute_dev) in TB/s of algorithmic bytes (8 k n 5 per ciphertext), beside crc_pool (2 x 2 sum pooling: 4 ciphertexts
    read, one written) on a tensor of the same byte count in the same process -- the elementwise yardstick, measured, not assumed
  * crc_sum_slots_forms per ciphertext, and the fixed part of an apply_galois call (key preparation and launch latencies: the intercept of the times at count / 2
    and count, both one internal pass) as a share of a call at count = 1 and at `count`
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(E, fn, calls):
    """ms per call: events around `calls` calls on the engine's stream"""
    import crcnn_amd as ca
    L, VP = E.L, ctypes.c_void_p
    a, b = VP(), VP()
    ca.binding._chk(L.crc_event_create(E.c, ctypes.byref(a)), "crc_event_create"); ca.binding._chk(L.crc_event_create(E.c, ctypes.byref(b)), "crc_event_create")
    fn(); E.sync()                                                     # warm: code objects, LDS attributes, caches
    L.crc_event_record(E.c, a, E.stream)
    for _ in range(calls):
        fn()
    L.crc_event_record(E.c, b, E.stream)
    E.sync()
    ms = ctypes.c_float(0)
    ca.binding._chk(L.crc_event_elapsed_ms(E.c, a, b, ctypes.byref(ms)), "crc_event_elapsed_ms")
    L.crc_event_destroy(E.c, a); L.crc_event_destroy(E.c, b)
    return ms.value / calls


def alternate(E, fns, calls, rounds):
    """{name: [ms per round]}: the candidates one after the other, `rounds` times"""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(E, fn, calls))
    return out


def fmt(v):
    return f"{statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def measure(n, k, t, count, calls, rounds):
    import crcnn_amd as ca
    q = ca.binding.default_coeff_modulus_128(n)[:k]
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    sk, pk = H.keygen(1)
    elts, gk = H.gen_galois_keys(2, sk)
    evk = H.gen_evk(3, sk)
    rng = np.random.RandomState(n)
    x = np.stack([(rng.randint(0, 1 << 62, size=(count, 2, n)).astype(np.uint64) % np.uint64(qi)) for qi in q], axis=2)
    d_x = E.upload(x); d_y = E.alloc(x.nbytes); d_x3 = E.alloc(x.nbytes // 2 * 3); d_gk = E.upload(gk); d_evk = E.upload(evk)
    d_w = E.alloc(max(E.apply_galois_work_bytes(count), E.sum_slots_work_bytes(count), E.square_relin_work_bytes(count)))
    E.galois_permute_dev(d_x, count, 3, d_x3)                          # a size-3 tensor of canonical residues for crc_relinearize
    # the yardstick's own tensors, sized from ITS shape: zd planes of 2 x 2 ciphertexts in, one ciphertext per plane out
    zd = count // 2
    ct_bytes = 2 * k * n * 8
    pool_in, pool_out = zd * 4, zd                                     # ciphertexts read / written
    pool_bytes = float(pool_in + pool_out) * ct_bytes                  # = count 5 k n 8 for an even count: what the permute moves
    d_pin = E.alloc(pool_in * ct_bytes); d_p = E.alloc(pool_out * ct_bytes)
    E.copy_d2d(d_pin, d_x, x.nbytes); E.copy_d2d(d_pin.ptr + x.nbytes, d_x, (pool_in - count) * ct_bytes)      # canonical residues throughout
    fns = {
        "apply_galois": lambda: E.apply_galois(d_x, count, 3, d_gk, elts, d_y, d_w),
        "relinearize": lambda: E.relinearize(d_x3, count, d_evk, d_y, d_w),
        "permute": lambda: E.galois_permute_dev(d_x, count, 3, d_x3),
        "pool": lambda: E.pool(d_pin, 1, zd, 2, 2, 2, 2, 2, 2, None, ca.COEFF, d_p),
        "sum_slots": lambda: E.sum_slots(d_x, count, d_gk, elts, d_y, d_w),
        "apply_galois_half": lambda: E.apply_galois(d_x, count // 2, 3, d_gk, elts, d_y, d_w),
        "apply_galois_one": lambda: E.apply_galois(d_x, 1, 3, d_gk, elts, d_y, d_w),
    }
    r = alternate(E, fns, calls, rounds)
    E.close(); H.close()
    med = {k_: statistics.median(v) for k_, v in r.items()}
    bytes_moved = 8.0 * k * n * 5 * count
    fixed = max(0.0, 2 * med["apply_galois_half"] - med["apply_galois"])
    lines = [f"## n = {n}, {k} moduli, t = {t}, {count} ciphertexts per call", "",
             f"- crc_apply_galois_forms (one step, g = 3): {fmt(r['apply_galois'])}",
             f"- crc_relinearize on the same size-3 tensor: {fmt(r['relinearize'])}",
             f"- ratio apply_galois / relinearize (medians): {med['apply_galois'] / med['relinearize']:.3f}",
             f"- galois_permute_kernel alone: {fmt(r['permute'])} = {bytes_moved / med['permute'] / 1e9:.2f} TB/s of {bytes_moved / 1e6:.0f} MB",
             f"- crc_pool (2 x 2 sum, {pool_in} ciphertexts in, {pool_out} out): {fmt(r['pool'])} = {pool_bytes / med['pool'] / 1e9:.2f} TB/s of {pool_bytes / 1e6:.0f} MB",
             f"- permute / pool rate: {(bytes_moved / med['permute']) / (pool_bytes / med['pool']):.2f}",
             f"- crc_sum_slots_forms ({n.bit_length() - 1} key switches): {fmt(r['sum_slots'])} = {1e3 * med['sum_slots'] / count:.2f} us per ciphertext",
             f"- apply_galois at count / 2: {fmt(r['apply_galois_half'])}; at count = 1: {fmt(r['apply_galois_one'])}",
             f"- fixed part of a call (2 T(count / 2) - T(count): key preparation and launch latencies): {fixed:.3f} ms = "
             f"{100 * fixed / med['apply_galois']:.1f} % of a call at count = {count}, {100 * min(1.0, fixed / med['apply_galois_one']):.0f} % at count = 1", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "galois.md"))
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.count < 2 or a.count % 2:
        ap.error("--count must be even and at least 2 (the pool yardstick takes count / 2 windows)")
    import crcnn_amd as ca
    out = ["# Galois automorphisms: measurements", "",
           f"tools/measure_galois.py on one GPU: HIP events around {a.calls} calls, candidates alternating {a.rounds} times in one process, median (min, max) per call.", ""]
    for n, k, t in ((4096, 2, 65537), (8192, 3, ca.Engine.slots_prime(8192, 30))):
        out += measure(n, k, t, a.count, a.calls, a.rounds)
    text = "\n".join(out)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
