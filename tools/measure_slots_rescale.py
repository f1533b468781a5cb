#!/usr/bin/env python3
"""The slot-wise rescale priced on one MI355X -> profiles/slots_rescale.md.

(a) crc_slots_rescale_dev on `--rows` rows at n = 2048, 4096, 8192, 16384 (t = crc_slots_prime(n, 30), divisor 2^7, out of place: in place every repetition would divide the one before's output) against crc_slots_decompose_dev +
    crc_slots_compose_dev back to back on the same rows (item-major): the two existing kernels a user would otherwise chain, which do strictly more work (the
    permutation, 8 n more bytes each way).  HIP events around `--reps` calls, the two alternating in one process, `--rounds` rounds: median and spread in us per
    row.  The result of the fused kernel is checked against the host twin on the first rows before anything is timed.
(b) crc_slots_refresh_dev against crc_refresh_dev on `--cts` NTT-form ciphertexts at (4096, 2), the same way: us per ciphertext.
(c) PlainModelTiny with a `rescale` behind each pool (tests/golden/slots/tiny_rescale.net) at (4096, 2), t = crc_slots_prime(4096, 30), input_bits 4, weight_bits
    5: the 32 synthetic golden images in the slots of one tensor through `test_host slots_build`; how many keep the float model's argmax (recorded, not gated),
    whether the integers equal tests/slots_rescale_model.py's, and the noise budget left.

One process per step, each under its own `timeout`, run one after the other and stopped at the first that fails:
    measure_slots_rescale.py                 the driver
    measure_slots_rescale.py kernel N ROWS   one ring, in process; prints one JSON line
    measure_slots_rescale.py refresh CTS     the refresh at (4096, 2), in process; prints one JSON line
Options: --rounds (7), --reps (20), --rows (4096), --cts (2048), --markdown FILE."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
RINGS = [2048, 4096, 8192, 16384]
DIVISOR = 1 << 7


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


def kernel_step(n, rows, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    q = ca.default_coeff_modulus_128(n)[:1]
    t = ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    H = ca.Engine(n, q, t, device=-1)
    rng = np.random.RandomState(2)
    p = rng.randint(0, t, size=(rows, n)).astype(np.uint64)
    d_p, d_v, d_o = E.upload(p), E.alloc(rows * n * 8), E.alloc(rows * n * 8)
    E.slots_rescale_dev(d_p, rows, DIVISOR, d_o)
    equal = bool(np.array_equal(E.download(d_o, (rows, n))[:8], H.slots_rescale(p[:8], DIVISOR)))

    def pair():
        E.slots_decompose_dev(d_p, rows, n, d_v, n, 1)
        E.slots_compose_dev(d_v, rows, n, n, 1, d_o)
    calls = {"rescale": lambda: E.slots_rescale_dev(d_p, rows, DIVISOR, d_o), "decompose + compose": pair}
    for fn in calls.values():
        fn()
    E.sync()
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    print(json.dumps(dict(n=n, t=t, rows=rows, equal_host_twin=equal, ms=ms)), flush=True)
    return 0 if equal else 3


def refresh_step(cts, rounds, reps):
    import numpy as np
    import crcnn_amd as ca
    n, k = 4096, 2
    q = ca.default_coeff_modulus_128(n)[:k]
    t = ca.Engine.slots_prime(n, 30)
    E = ca.Engine(n, q, t, device=0)
    sk, pk = E.keygen(3)
    d_sk, d_pk = E.upload(sk), E.upload(pk)
    rng = np.random.RandomState(4)
    d_pl = E.upload(rng.randint(0, t, size=(cts, n)).astype(np.uint64))
    d_ct, d_out = E.alloc(cts * 2 * k * n * 8), E.alloc(cts * 2 * k * n * 8)
    E.encrypt_dev_forms(d_pk, d_pl, cts, 5, ca.NTT, d_ct, E.alloc(E.encrypt_dev_work_bytes(cts)))
    d_w = E.alloc(max(E.slots_refresh_dev_work_bytes(cts, ca.NTT), E.refresh_dev_work_bytes(cts, ca.NTT)))
    calls = {"crc_slots_refresh_dev": lambda: E.slots_refresh_dev(d_sk, d_pk, d_ct, cts, DIVISOR, 9, d_out, d_w, in_form=ca.NTT, out_form=ca.NTT),
             "crc_refresh_dev": lambda: E.refresh_dev(d_sk, d_pk, d_ct, cts, 9, d_out, d_w, in_form=ca.NTT, out_form=ca.NTT)}
    for fn in calls.values():
        fn()
    E.sync()
    ms = {nm: [] for nm in calls}
    for _ in range(rounds):
        for nm, fn in calls.items():
            ms[nm].append(events_ms(E, fn, reps))
    print(json.dumps(dict(n=n, k=k, t=t, cts=cts, ms=ms)), flush=True)
    return 0


def run(cmd, limit, log):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    log.append(f"$ {' '.join(cmd)}\n(exit {p.returncode})\n{p.stdout[-4000:]}\n{p.stderr[-3000:]}\n")
    print(f"[measure_slots_rescale] exit {p.returncode}: {' '.join(cmd[-6:])}", file=sys.stderr, flush=True)
    return p.stdout if p.returncode == 0 else None


def accuracy(log):
    """-> dict for the report, or None when the run failed"""
    import numpy as np
    import crcnn_amd as ca
    import slots_rescale_model as rm
    from benchkit.plain import plain_forward
    from crcnn_amd import netrun
    from crcnn_amd.synth import normalize, synth_image
    from netcommon import GOLD, model_weights
    n, k, S, in_bits, w_bits = 4096, 2, 32, 4, 5
    q = ca.default_coeff_modulus_128(n)[:k]
    t = ca.Engine.slots_prime(n, 30)
    desc = os.path.join(GOLD, "slots", "tiny_rescale.net")
    layers = netrun.load_description(desc)
    W = model_weights("PlainModelTiny")
    imgs = [normalize(synth_image(i)) for i in range(S)]
    images = np.stack([np.asarray(im, dtype=np.float32).reshape(layers.input_shape) for im in imgs])
    d = tempfile.mkdtemp()
    np.array([n, k, t] + q, dtype=np.uint64).tofile(os.path.join(d, "params.u64"))
    images.tofile(os.path.join(d, "images.f32"))
    out = run([os.path.join(ROOT, "crcnn_amd", "lib", "test_host"), "slots_build", desc, os.path.join(GOLD, "models", "PlainModelTiny.h5"), d, str(S), str(in_bits),
               str(w_bits)], 400, log)
    if out is None:
        return None
    lines = dict(l.split(" ", 1) for l in out.splitlines() if " " in l)
    got = np.fromfile(os.path.join(d, "slots_fused.i64"), dtype=np.int64).reshape(S, -1)
    want, scale = rm.network_forward(list(layers), W, images, t, in_bits, w_bits)
    keep = sum(int(np.argmax(got[i]) == np.argmax(plain_forward("PlainModelTiny", W, imgs[i]))) for i in range(S))
    err = max(float(np.abs(got[i] / float(scale) - plain_forward("PlainModelTiny", W, imgs[i])).max()) for i in range(S))
    return dict(n=n, k=k, t=t, S=S, input_bits=in_bits, weight_bits=w_bits, scale=float(scale), argmax_kept=keep, max_logit_abs_err=err, equal_model=got.tolist() == want,
                budget=int(lines["budget"].split()[3]), budget_unfused=int(lines["budget"].split()[1]))


def med_spread(vals, per):
    us = [1e3 * v / per for v in vals]
    return statistics.median(us), min(us), max(us)


def report(kern, refresh, acc, a):
    L = ["# The slot-wise rescale: one kernel against decompose + compose, the slot refresh, and a rescaled PlainModelTiny", "",
         f"One MI355X.  HIP events around {a.reps} calls, the compared calls alternating in one process, {a.rounds} rounds: median (min .. max).", "",
         "## slots_rescale_kernel against slots_decompose_kernel + slots_compose_kernel", "",
         f"{a.rows} rows per call, t = crc_slots_prime(n, 30), divisor 2^7; us per row.", "",
         "| n | rescale | min .. max | decompose + compose | min .. max | ratio | rescale equals the host twin |", "|---|---|---|---|---|---|---|"]
    slower = []
    for r in kern:
        m1, lo1, hi1 = med_spread(r["ms"]["rescale"], r["rows"]); m2, lo2, hi2 = med_spread(r["ms"]["decompose + compose"], r["rows"])
        L.append(f"| {r['n']} | {m1:.3f} | {lo1:.3f} .. {hi1:.3f} | {m2:.3f} | {lo2:.3f} .. {hi2:.3f} | {m1 / m2:.2f} | {r['equal_host_twin']} |")
        if m1 > m2 + max(hi1 - lo1, hi2 - lo2):
            slower.append(r["n"])
    L += ["", ("**The fused kernel is slower than the pair by more than the measured spread at n = " + ", ".join(map(str, slower)) + "**: reported, not tuned blind."
               if slower else "The fused kernel is not slower than the pair by more than the measured spread at any n."), ""]
    L += ["## crc_slots_refresh_dev against crc_refresh_dev at (4096, 2)", ""]
    if refresh is None:
        L += ["not measured (the step failed; see the log)", ""]
    else:
        L += [f"{refresh['cts']} NTT-form ciphertexts per call, NTT form out, public-key re-encryption in both; us per ciphertext.", "", "| call | us per ciphertext | min .. max |", "|---|---|---|"]
        for nm, vs in refresh["ms"].items():
            m, lo, hi = med_spread(vs, refresh["cts"])
            L.append(f"| {nm} | {m:.3f} | {lo:.3f} .. {hi:.3f} |")
        L.append("")
    L += ["## PlainModelTiny with a rescale behind each pool, 30-bit slot prime", ""]
    if acc is None:
        L += ["not measured (the run failed; see the log)", ""]
    else:
        L += [f"(n, k) = ({acc['n']}, {acc['k']}), t = {acc['t']}, input_bits {acc['input_bits']}, weight_bits {acc['weight_bits']}, final scale {acc['scale']:.0f}; the "
              f"{acc['S']} synthetic golden images in the slots of one tensor (`test_host slots_build`, tests/golden/slots/tiny_rescale.net).", "",
              f"* images that keep the float model's argmax: **{acc['argmax_kept']} of {acc['S']}** (recorded, not gated); largest |logit / scale - float logit| {acc['max_logit_abs_err']:.4f}",
              f"* integers equal tests/slots_rescale_model.py's in every slot: {acc['equal_model']}",
              f"* noise budget left: {acc['budget']} bits fused, {acc['budget_unfused']} unfused", ""]
    L += [f"command: python tools/measure_slots_rescale.py --rounds {a.rounds} --reps {a.reps} --rows {a.rows} --cts {a.cts}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all"); ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cts", type=int, default=2048)
    ap.add_argument("--out"); ap.add_argument("--markdown", default=os.path.join(ROOT, "profiles", "slots_rescale.md"))
    a = ap.parse_args()
    if a.mode == "kernel":
        return kernel_step(a.shape[0], a.shape[1], a.rounds, a.reps)
    if a.mode == "refresh":
        return refresh_step(a.shape[0], a.rounds, a.reps)
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    log, kern, refresh, acc = [], [], None, None
    me = [sys.executable, os.path.abspath(__file__)]
    opts = ["--rounds", str(a.rounds), "--reps", str(a.reps)]
    ok = True
    for n in RINGS:
        out = run(me + ["kernel", str(n), str(a.rows)] + opts, 180, log)
        if out is None:
            ok = False
            break
        kern.append(json.loads(out.strip().splitlines()[-1]))
    if ok:
        out = run(me + ["refresh", str(a.cts)] + opts, 180, log)
        ok = out is not None
        if ok:
            refresh = json.loads(out.strip().splitlines()[-1])
    if ok:
        acc = accuracy(log)
        ok = acc is not None
    open(os.path.join(out_dir, "measure_slots_rescale.log"), "w").write("\n".join(log))
    if not kern:
        print("\n".join(log)[-3000:])
        return 2
    text = report(kern, refresh, acc, a)
    print(text)
    if ok and a.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(a.markdown)), exist_ok=True)
        open(a.markdown, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
