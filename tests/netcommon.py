"""shared helpers for the whole-network parity tests (oracle side: input generation and the reference-order forward)"""
import hashlib
import json
import os

import numpy as np

from oracle import orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load_net_golden(name):
    return json.load(open(os.path.join(GOLD, f"net_{name}.json")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a)).hexdigest()          # (the array's own buffer: no second copy of a multi-GB tensor)


_M28 = (1 << 28) - 1


def limb_extreme(q):
    """the residue r < q with the largest (r mod 2^28) + (r >> 28): the largest Karatsuba middle term (x0 + x1)(w0 + w1)"""
    cands = []
    for x1 in range((q - 1) >> 28, max(((q - 1) >> 28) - 2, -1), -1):
        cands.append((x1 << 28) | min(_M28, q - 1 - (x1 << 28)))
    r = max(cands, key=lambda v: (v & _M28) + (v >> 28))
    # defining property, checked against the bound: no residue has a larger limb sum
    top = (q - 1) >> 28
    best = max(((q - 1) & _M28) + top, (_M28 + top - 1) if top else 0)
    assert r < q and (r & _M28) + (r >> 28) == best
    return r


_PIECES = []


def sha_device(E, buf, nbytes, offset=0, piece=64 << 20):
    """SHA-256 of nbytes of a device buffer, streamed through two reused 64-MiB host pieces: the next piece is copied down while the previous one is hashed
    (hashlib releases the GIL), and no multi-GB host tensor is allocated and page-faulted just to be hashed once (PlainModelWoPad's conv1 output at n = 16384
    is 11.5 GB: the layer-wise parity tests spent a third of their time there)"""
    from concurrent.futures import ThreadPoolExecutor
    if not _PIECES:
        _PIECES.extend(np.empty(piece, dtype=np.uint8) for _ in range(2))
    h = hashlib.sha256()
    base = E.p(buf) + offset
    E.sync()
    with ThreadPoolExecutor(1) as pool:
        pending = None
        for j, o in enumerate(range(0, nbytes, piece)):
            m = min(piece, nbytes - o)
            dst = _PIECES[j & 1]
            from crcnn_amd.binding import _chk
            _chk(E.L.crc_memcpy_d2h(E.c, dst.ctypes.data, base + o, m, E.stream), "crc_memcpy_d2h")
            E.sync()
            if pending is not None:
                pending.result()
            pending = pool.submit(h.update, dst[:m])
        if pending is not None:
            pending.result()
    return h.hexdigest()


_INPUTS = {}


def make_inputs(g):
    """regenerate keys + the encrypted synthetic image exactly as oracle/make_golden_nets.py did (cached per golden input: the CPU-side key generation and the 784
    encryptions take seconds at n = 16384, and every test of a parameter set -- layer-wise, NTT-resident, the C++ classes -- starts from the same input)"""
    key = (g["n"], tuple(g["q"]), g["t"], g["input_sha256"])
    if key not in _INPUTS:
        if len(_INPUTS) >= 6:
            _INPUTS.pop(next(iter(_INPUTS)))
        _INPUTS[key] = _make_inputs(g)
    return _INPUTS[key]


def _make_inputs(g):
    O = orc.Oracle(g["n"], g["q"], g["t"])
    img = orc.normalize(orc.synth_image(g["image_index"]))
    if g.get("input_gen") == "engine":
        # goldens at the parameter sets bench.py runs: keys and the encrypted image come from the ENGINE's seeded host-side client
        # (crc_keygen / crc_gen_evk / crc_encrypt; no GPU), so that bench.py can reproduce them without touching oracle/
        import crcnn_amd as ca
        E = ca.Engine(g["n"], g["q"], g["t"], device=-1)
        sk, pk = E.keygen(g["key_seed"]); evk = E.gen_evk(g["evk_seed"], sk)
        pl, _ = E.encode(img.reshape(-1))
        x = E.encrypt(pk, pl, g["enc_seed"]).reshape(1, 28, 28, 2, O.k, O.n)
        E.close()
    else:
        sk, pk = O.keygen(g["key_seed"]); evk = O.gen_evk(g["evk_seed"], sk)
        x = O.encrypt_many(pk, O.encode_many(img).reshape(1, 28, 28, O.n), g["enc_seed"])
    assert sha(x) == g["input_sha256"], "input generation drifted from the golden"
    return O, sk, pk, evk, img, x


def model_weights(model):
    import crcnn_amd as ca
    path = os.path.join(GOLD, "models", model + ".h5")
    return {nm: ca.h5_read(path, nm) for nm in ca.h5_list(path) if not nm.endswith("num_batches_tracked")}


def oracle_forward(O, model, W, x, evk, threads=8, fast=True):
    """Network::forward with the oracle's reference-order layer loops; yields (layer index, output tensor)"""
    from crcnn_amd.netrun import TOPOLOGIES
    enc = lambda a: O.encode_many(np.asarray(a, dtype=np.float32)).reshape(np.shape(a) + (O.n,))
    t = x
    for i, (kind, name, a) in enumerate(TOPOLOGIES[model]):
        if kind == "conv":
            w = O.plains_to_ntt(enc(W[name + ".weight"].reshape(a["nf"], a["zd"], a["xf"], a["yf"])))
            t = O.conv(t, w, enc(W[name + ".bias"]), a["xs"], a["ys"], threads=threads, fast=fast)
        elif kind == "fc":
            w = O.plains_to_ntt(enc(W[name + ".weight"].reshape(a["out_dim"], a["in_dim"], 1, 1)))
            flat = np.ascontiguousarray(t).reshape(a["in_dim"], 1, 1, 2, O.k, O.n)
            t = O.conv(flat, w, enc(W[name + ".bias"]), 1, 1, threads=threads, fast=fast).reshape(1, a["out_dim"], 1, 2, O.k, O.n)
        elif kind in ("pool", "avgpool"):
            div = O.encode(1.0 / (a["xf"] * a["yf"]))[0] if kind == "avgpool" else None
            t = O.pool(t, a["xs"], a["ys"], a["xf"], a["yf"], div_plain=div, threads=threads)
        elif kind == "bn":
            invstd = np.float32(1.0 / np.sqrt(W[name + ".running_var"].astype(np.float64) + 0.00001))
            t = O.bn(t, enc(W[name + ".running_mean"]), enc(invstd), threads=threads)
        elif kind == "square":
            t = O.square_layer(t, evk, threads=threads)
        yield i, t
