#!/usr/bin/env python3
"""Time crc_noise_budget_dev on a real layer tensor, beside the two figures it is judged by: crc_noise_budget on the host (the only way without the device path) and
crc_decrypt_dev on the same tensor (the same dot product and inverse transforms in front of a different per-coefficient kernel: the natural floor).

  tiny4096    PlainModelTiny  (4096, 2, t = 2^32): the tensor behind conv1 + pool1, 32 x 12 x 12 ciphertexts per image, batch 128
              (conv1's own output, 32 x 24 x 24 per image, is 155 GB at batch 128 before any work space: the pooled tensor stands in for it)
  approx8192  ApproxPlainModel (8192, 3, t = 2^42): the tensor behind pool2, 50 x 4 x 4 ciphertexts per image, batch 96

The tensor is what the network computes for 16 distinct seeded synthetic images (coefficient form between the layers), tiled on the device to the batch.  HIP events
around `--reps` calls after `--warmup` calls; both ciphertext forms (the coefficient-form call transforms the ciphertexts first; an NTT-resident network hands
over NTT form).  The host figure is wall time over 64 ciphertexts of the same tensor.

usage: measure_budget.py [--config tiny4096|approx8192|both] [--batch B] [--reps 20] [--warmup 5] [--markdown FILE]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import crcnn_amd as ca  # noqa: E402
from crcnn_amd import synth  # noqa: E402
from crcnn_amd.netrun import Network  # noqa: E402

CONFIGS = {
    "tiny4096": dict(model="PlainModelTiny", n=4096, k=2, t=1 << 32, layer="pool1", batch=128),
    "approx8192": dict(model="ApproxPlainModel", n=8192, k=3, t=1 << 42, layer="pool2", batch=96),
}
DISTINCT = 16


class _Grabbed(Exception):
    pass


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


def layer_tensor(E, cfg, sk, pk):
    """the tensor behind cfg['layer'] for DISTINCT images: device buffer (coefficient form) and ciphertexts per image"""
    evk = E.gen_evk(12, sk)
    net = Network(E, cfg["model"], h5_path=os.path.join(ROOT, "tests", "golden", "models", cfg["model"] + ".h5"), resident=False, d_evk=E.upload(evk))
    net.prepare(DISTINCT)
    idx = [i for i, pl in enumerate(net.plan) if pl[1] == cfg["layer"]][0]
    per_image = int(np.prod(net.plan[idx][5]))
    ct_bytes = 2 * E.k * E.n * 8
    grab = E.alloc(DISTINCT * per_image * ct_bytes)
    x = np.stack([E.encrypt(pk, E.encode(synth.normalize(synth.synth_image(i)).reshape(-1))[0], 5000 + 1000 * i).reshape(1, 28, 28, 2, E.k, E.n)
                  for i in range(DISTINCT)])

    def timer(i, name, kind, phase):
        if i == idx and phase == 1:
            E.L.crc_memcpy_d2d(E.c, E.p(grab), E.p(net.buf[net.slots[i]]), DISTINCT * per_image * ct_bytes, E.stream)
            E.sync()
            raise _Grabbed()

    try:
        net.forward(E.upload(x), DISTINCT, timer=timer)
    except _Grabbed:
        pass
    return grab, per_image


def measure(name, batch, reps, warmup):
    cfg = CONFIGS[name]
    batch = batch or cfg["batch"]
    q = ca.default_coeff_modulus_128(cfg["n"])[:cfg["k"]]
    E = ca.Engine(cfg["n"], q, cfg["t"], device=0)
    sk, pk = E.keygen(11)
    grab, per_image = layer_tensor(E, cfg, sk, pk)
    ct_bytes = 2 * E.k * E.n * 8
    count = batch * per_image
    d_ct = E.alloc(count * ct_bytes)
    for b0 in range(0, batch, DISTINCT):
        nb = min(DISTINCT, batch - b0)
        E.L.crc_memcpy_d2d(E.c, E.p(d_ct) + b0 * per_image * ct_bytes, E.p(grab), nb * per_image * ct_bytes, E.stream)
    E.sync()
    grab.free()
    # the host: 64 ciphertexts of the tensor
    sample = E.download(d_ct, (64, 2, E.k, E.n))
    t0 = time.perf_counter()
    host_bits = [E.noise_budget(sk, c) for c in sample]
    host_us = (time.perf_counter() - t0) / 64 * 1e6
    d_sk = E.upload(sk)
    d_bits, d_min = E.alloc(4 * count), E.alloc(8)
    d_plain = E.alloc(count * E.n * 8)
    rows = []
    for form, fname in ((ca.COEFF, "coefficient"), (ca.NTT, "NTT")):
        if form == ca.NTT:
            E.ntt_fwd(d_ct, count)
        d_work = E.alloc(max(E.noise_budget_dev_work_bytes(count, 2, form), E.decrypt_dev_work_bytes(count, 2, form)))
        bud_ms = events_ms(E, lambda: E.noise_budget_dev(d_sk, d_ct, count, d_bits, d_work, in_form=form, d_min=d_min), reps, warmup)
        bits = E.download(d_bits, (count,), dtype=np.int32)
        pair = E.download(d_min, (2,), dtype=np.int32)
        assert [int(b) for b in bits[:64]] == host_bits and int(pair[0]) == int(bits.min()) and int(pair[1]) == int(np.argmin(bits))
        dec_ms = events_ms(E, lambda: E.decrypt_dev(d_sk, d_ct, count, d_plain, d_work, in_form=form), reps, warmup)
        rows.append(dict(config=name, model=cfg["model"], n=cfg["n"], k=cfg["k"], layer=cfg["layer"], batch=batch, count=count, form=fname,
                         budget_ms=bud_ms, budget_us_per_ct=bud_ms * 1e3 / count, decrypt_ms=dec_ms, decrypt_us_per_ct=dec_ms * 1e3 / count,
                         host_us_per_ct=host_us, min_budget=int(pair[0]), max_budget=int(bits.max())))
        d_work.free()
    E.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=sorted(CONFIGS) + ["both"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--markdown", default=None, help="also write the table to this file")
    a = ap.parse_args()
    rows = []
    for name in (sorted(CONFIGS, reverse=True) if a.config == "both" else [a.config]):
        rows += measure(name, a.batch, a.reps, a.warmup)
    import torch
    pr = torch.cuda.get_device_properties(0)
    box = f"{pr.name} ({pr.gcnArchName}, {pr.multi_processor_count} CUs, {pr.total_memory >> 30} GiB), torch {torch.__version__}"
    lines = ["| tensor | ciphertexts | form | crc_noise_budget_dev | per ciphertext | crc_decrypt_dev | per ciphertext | budget / decrypt | crc_noise_budget (host) per ciphertext |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['model']} ({r['n']}, {r['k']}) behind {r['layer']}, batch {r['batch']} | {r['count']} | {r['form']} | {r['budget_ms']:.3f} ms | "
                     f"{r['budget_us_per_ct']:.3f} us | {r['decrypt_ms']:.3f} ms | {r['decrypt_us_per_ct']:.3f} us | {r['budget_ms'] / r['decrypt_ms']:.2f} | "
                     f"{r['host_us_per_ct']:.0f} us |")
    lines.append("")
    lines.append("budgets seen: " + "; ".join(f"{r['config']} {r['form']}: {r['min_budget']}..{r['max_budget']}" for r in rows))
    lines.append(f"box: {box}")
    lines.append(f"command: python tools/measure_budget.py --config {a.config} --reps {a.reps} --warmup {a.warmup}" + (f" --batch {a.batch}" if a.batch else ""))
    text = "\n".join(lines)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
