"""The packed convolution with strides, zero padding, a bias and a mask on the host: the general planner against a direct padded, strided, pooled integer
convolution over a grid of geometries, its mask, the clean-input contract, equality with the first planner at that one's parameters, the refusals (too little
margin among them), the bias packing against its definition, the C++ planner against the Python one, and the integer model through encryption at the small ring."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conv_slots_model as cm
import conv_slots_pad_model as pm
import galois_hoisted_model as hm
import galois_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ops_n256_k2_t20.npz")
T = 65537
# pad x stride x pool x pool_stride x dil x margin, each on a 7 x 6 and an 8 x 8 plane: 288 geometries (pool 1 at pool_stride 2: a subsampling, still a layer)
GRID = list(itertools.product((0, 1, 2), (1, 2), (1, 2), (1, 2), (1, 2), (0, 1, 2), ((7, 6), (8, 8))))
M_GRID = 512                                                           # dilation 2 of 8 rows at pitch 10 behind an origin of 22: 22 + 2 . 77 < 512


def geometry(margin, H, W):
    pitch = W + margin
    return pitch, margin * (pitch + 1)


def test_plan_against_the_direct_convolution_over_the_grid():
    """every geometry the planner admits: planes tiled with period M over both slot rows -- random junk at every non-pixel slot where pad = 0, zeros there where
    pad > 0 (the clean input the plan asks for) -- give, through the plan's taps with the folded weights, the padded, strided, pooled convolution at the valid
    slots of every period, mod t.  At this M the planner refuses exactly the geometries whose margin is below the pad: 96 of the 288"""
    import crcnn_amd as ca
    n = 2 * M_GRID
    seen = refused = 0
    for g, (pad, s, p, ps, dil, margin, (H, W)) in enumerate(GRID):
        pitch, origin = geometry(margin, H, W)
        try:
            plan = ca.binding.conv_slots_plan_geom(n, M_GRID, pitch, origin, H, W, 3, 3, dil, pad, s, p, ps)
        except ValueError:
            refused += 1
            assert pad > margin, (pad, s, p, ps, dil, margin, H, W)
            continue
        seen += 1
        assert plan.needs_clean_input == (pad > 0) and plan.out_dil == dil * s * ps and plan.origin == origin
        eh = 3 + s * (p - 1)
        assert plan.steps == [dil * ((a - pad) * pitch + (b - pad)) for a in range(eh) for b in range(eh)]
        assert plan.elements == [gm.elt_rows(n, st) for st in plan.steps] and 0 not in plan.elements
        rng = np.random.RandomState(1000 + g)
        img = rng.randint(0, T, size=(2, H, W)).astype(np.int64)
        w = rng.randint(-(T // 2), T // 2 + 1, size=(2, 2, 3, 3)).astype(np.int64)
        wf = plan.fold(w, T)
        assert wf.shape == (2, 2, eh * eh) and (wf >= 0).all() and (wf < T).all()
        planes = [pm.plane_slots_geom(img[ci], n, M_GRID, pitch, origin, dil, junk=None if pad else rng.randint(0, T, size=M_GRID)) for ci in range(2)]
        got = cm.conv_plan_slots(plan, wf, planes, T)
        want = pm.conv_direct_geom(img, w, pad, s, p, ps, t=T)
        assert want.shape == (2, plan.out_h, plan.out_w)
        for base in range(0, n, M_GRID):
            for co in range(2):
                assert [int(got[co][base + v]) for v in plan.valid] == [int(v) for v in want[co].reshape(-1)], (pad, s, p, ps, dil, margin, H, W, base, co)
    assert (seen, refused) == (192, 96)


@pytest.mark.parametrize("pad,s,p,ps,dil,margin", [(1, 1, 1, 1, 1, 1), (1, 2, 1, 1, 1, 1), (2, 1, 2, 1, 1, 2), (1, 2, 2, 2, 2, 2), (0, 2, 2, 1, 1, 0)])
def test_mask_and_the_composition_on_slots(pad, s, p, ps, dil, margin):
    """mask_slots is 1 exactly at the valid slots of every period; the composition's statement (taps, + bias, times mask) is the biased convolution there and
    exactly 0 at every other slot -- a clean plane for the next layer"""
    import crcnn_amd as ca
    H, W, M = 7, 6, 256
    n = 4 * M
    pitch, origin = geometry(margin, H, W)
    plan = ca.binding.conv_slots_plan_geom(n, M, pitch, origin, H, W, 3, 3, dil, pad, s, p, ps)
    mask = plan.mask_slots()
    assert mask.shape == (n,) and mask.dtype == np.int64 and set(np.flatnonzero(mask).tolist()) == {b + v for b in range(0, n, M) for v in plan.valid}
    assert np.array_equal(plan.mask_slots(2 * n), np.tile(mask, 2))
    with pytest.raises(ValueError):
        plan.mask_slots(M + 1)
    rng = np.random.RandomState(pad + 10 * s)
    img = rng.randint(0, T, size=(2, H, W)).astype(np.int64)
    w = rng.randint(-(T // 2), T // 2 + 1, size=(3, 2, 3, 3)).astype(np.int64)
    bias = np.array([T - 1, 0, -5], dtype=np.int64)
    planes = [pm.plane_slots_geom(img[ci], n, M, pitch, origin, dil, junk=None if pad else rng.randint(0, T, size=M)) for ci in range(2)]
    got = pm.conv_bias_mask_slots(plan, plan.fold(w, T), planes, T, bias, mask)
    want = pm.conv_direct_geom(img, w, pad, s, p, ps, bias=bias, t=T)
    for co in range(3):
        assert [int(got[co][v]) for v in plan.valid] == [int(v) for v in want[co].reshape(-1)]
        assert all(int(got[co][i]) == 0 for i in range(n) if not mask[i])
        assert [int(v) for v in got[co][:M]] * (n // M) == [int(v) for v in got[co]]


@pytest.mark.parametrize("pad,s,margin", [(1, 1, 1), (2, 1, 2), (1, 2, 1)])
def test_the_clean_input_contract_is_not_vacuous(pad, s, margin):
    """pad > 0: one junk value in a margin slot that a padding tap reads DOES change a valid output"""
    import crcnn_amd as ca
    H, W, M = 7, 6, 256
    n = 2 * M
    pitch, origin = geometry(margin, H, W)
    plan = ca.binding.conv_slots_plan_geom(n, M, pitch, origin, H, W, 3, 3, 1, pad, s)
    assert plan.needs_clean_input
    rng = np.random.RandomState(3)
    img = rng.randint(0, T, size=(1, H, W)).astype(np.int64)
    w = rng.randint(1, T // 2, size=(1, 1, 3, 3)).astype(np.int64)      # no zero weight: every tap counts
    wf = plan.fold(w, T)
    clean = pm.plane_slots_geom(img[0], n, M, pitch, origin, 1)
    dirty = clean.copy()
    slot = (origin - 1) % M                                             # the pixel left of (0, 0): a zero of the padding
    assert clean[slot] == 0 and (plan.valid[0] + plan.steps[pad * 3 + pad - 1]) % M == slot
    dirty[slot::M] = 12345
    a = cm.conv_plan_slots(plan, wf, [clean], T)
    b = cm.conv_plan_slots(plan, wf, [dirty], T)
    want = pm.conv_direct_geom(img, w, pad, s, t=T)
    assert [int(a[0][v]) for v in plan.valid] == [int(v) for v in want[0].reshape(-1)]
    assert any(int(a[0][v]) != int(b[0][v]) for v in plan.valid)


@pytest.mark.parametrize("args", [(256, 64, 8, 8, 8, 3, 3, 1, 1), (256, 64, 8, 8, 8, 3, 3, 1, 2), (512, 128, 8, 8, 8, 3, 3, 2, 2), (8192, 256, 14, 12, 12, 3, 3, 1, 2),
                                  (64, 32, 5, 6, 5, 6, 5, 1, 1), (4096, 1024, 28, 28, 28, 5, 5, 1, 2)])
def test_equals_the_first_planner_at_its_own_parameters(args):
    """pad = 0, stride = 1, pool_stride = pool (given, or left at 0), origin = 0: steps, elements, output geometry, valid list and fold are conv_slots_plan's"""
    import crcnn_amd as ca
    n, M, pitch, H, W, fh, fw, dil, pool = args
    old = ca.binding.conv_slots_plan(*args)
    w = np.random.RandomState(n).randint(-(1 << 40), 1 << 40, size=(2, 3, fh, fw)).astype(np.int64)
    for ps in (0, pool):
        new = ca.binding.conv_slots_plan_geom(n, M, pitch, 0, H, W, fh, fw, dil, 0, 1, pool, ps)
        assert (new.steps, new.elements, new.valid) == (old.steps, old.elements, old.valid)
        assert (new.out_h, new.out_w, new.out_dil, new.pitch, new.M, new.n) == (old.out_h, old.out_w, old.out_dil, old.pitch, old.M, old.n)
        assert not new.needs_clean_input and new.pool_stride == pool
        assert np.array_equal(new.fold(w, T), old.fold(w, T))


def test_refusals():
    import crcnn_amd as ca
    f = ca.binding.conv_slots_plan_geom
    base = dict(n=512, M=256, pitch=9, origin=10, H=8, W=8, fh=3, fw=3, dil=1, pad=1, stride=1, pool=1, pool_stride=0)
    assert f(**base).valid[0] == 10
    for bad in (dict(M=48), dict(M=0), dict(M=512), dict(M=64), dict(n=100),                    # not a power of two, none, above n/2, no room, n
                dict(pitch=8), dict(M=128, H=14, origin=0), dict(pad=2),                       # too little margin: right of a row, above the plane, both
                dict(pitch=7), dict(fh=11), dict(fw=11), dict(pool=9), dict(H=0), dict(W=0), dict(fh=0), dict(fw=0), dict(dil=0), dict(pool=0), dict(pitch=0),
                dict(stride=0), dict(pad=-1), dict(origin=-1), dict(pool_stride=-1), dict(dil=4), dict(origin=200)):
        a = dict(base)
        a.update(bad)
        with pytest.raises(ValueError):
            f(**a)
    assert f(**dict(base, pad=0, origin=0, pitch=8)).steps[0] == 0      # (without padding no margin is needed)
    assert f(**dict(base, M=128, H=13, origin=0)).steps[0] == -10       # (the empty tail of the period before is margin too: rows 0 .. 12 end at slot 115)
    assert f(**dict(base, pad=2, pitch=10, origin=22)).steps[0] == -22  # (and two pixels of it serve pad = 2)
    with pytest.raises(ValueError):                                     # |step| >= n/2: a tap two rows above at pitch 20 and dilation 4 in a ring of 128 slots a row
        f(256, 128, 20, 88, 1, 2, 5, 3, 4, 2)
    with pytest.raises(ValueError):                                     # outputs of a 1 x 1 window with pad 1 land one row below the plane: beyond the period
        f(256, 64, 8, 9, 6, 6, 1, 1, 1, 1)
    plan = f(**base)
    with pytest.raises(ValueError):
        plan.fold(np.zeros((2, 2, 3, 2), dtype=np.int64), T)
    E = ca.Engine(512, [0x3fffffff000001], T, device=-1)
    p2 = E.conv_slots_plan_geom(256, 9, 10, 8, 8, 3, 3, pad=1, stride=2)
    assert p2.steps == f(512, 256, 9, 10, 8, 8, 3, 3, 1, 1, 2).steps and p2.n == 512 and (p2.out_h, p2.out_w, p2.out_dil) == (4, 4, 2)
    E.close()


@pytest.mark.parametrize("q,t", [([0x7fffffff380001, 0x3fffffff000001], T), ([0x3fffffff000001], 12289), ([0xffffffffffc0001, 1073479681], (1 << 30) + 3)],
                         ids=["t65537_k2", "t12289_k1", "t_above_a_modulus"])
def test_pack_bias_is_the_constant_delta_rows_word(q, t):
    """b = 0, 1, (t - 1) / 2, (t + 1) / 2, t - 1, -1 and the int64 extremes: c = b mod t in [0, t), then floor(q / t) c (+ q mod t from (t + 1) / 2 on) mod q_i in
    Python integers -- and, where the oracle takes the parameters, what its add_plain adds to coefficient 0 of polynomial 0"""
    import crcnn_amd as ca
    n = 256
    E = ca.Engine(n, q, t, device=-1)
    bs = [0, 1, (t - 1) // 2, (t + 1) // 2, t - 1, -1, -t, t, t + 1, -(t // 2), np.iinfo(np.int64).max, np.iinfo(np.int64).min, 123456789012345]
    got = E.conv_slots_pack_bias(np.array(bs, dtype=np.int64).reshape(1, -1))
    assert got.shape == (len(q), 1, len(bs)) and got.dtype == np.uint64
    for i, qi in enumerate(q):
        assert [int(v) for v in got[i, 0]] == [pm.bias_word(b, t, q, i) for b in bs], i
        assert all(int(v) < qi for v in got[i, 0])
    if min(q) > t:
        from oracle import orc
        O = orc.Oracle(n, q, t)
        zero = np.zeros((2, len(q), n), dtype=np.uint64)
        for j, b in enumerate(bs):
            plain = np.zeros(n, dtype=np.uint64); plain[0] = int(b) % t
            r = O.add_plain(zero, plain)
            assert [int(r[0, i, 0]) for i in range(len(q))] == [int(got[i, 0, j]) for i in range(len(q))] and not r[1].any() and not r[0, :, 1:].any(), j
    assert E.conv_slots_pack_bias(np.zeros((0,), dtype=np.int64)).shape == (len(q), 0)
    E.close()


def test_cpp_planner_equals_the_python_planner():
    """tests/cpp/conv_slots_geom_plan_check.cpp (address and undefined-behaviour sanitizers) prints crc_conv_slots_plan_geom, crc_conv_slots_fold_geom and
    crc_conv_slots_mask_slots for the cases of a file; inside it checks that a refusal writes nothing"""
    import crcnn_amd as ca
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "conv_slots_geom_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "conv_slots_geom_plan_check.cpp"), "-o", exe])
    rng = np.random.RandomState(5)
    cases, bad = [], []
    for pad, s, p, ps, dil, margin, (H, W) in GRID[::7]:                # n M pitch origin H W fh fw dil pad stride pool pool_stride Cout Cin t
        pitch, origin = geometry(margin, H, W)
        c = (2 * M_GRID, M_GRID, pitch, origin, H, W, 3, 3, dil, pad, s, p, ps, 2, 2, T)
        try:
            ca.binding.conv_slots_plan_geom(*c[:13])
            cases.append(c)
        except ValueError:
            bad.append(c)
    cases += [(8192, 1024, 30, 31, 28, 28, 5, 5, 1, 0, 2, 2, 1, 2, 1, T), (8192, 256, 14, 15, 12, 12, 3, 3, 1, 1, 2, 1, 0, 2, 3, 12289),
              (64, 32, 5, 0, 6, 5, 6, 5, 1, 0, 1, 1, 1, 1, 1, 2), (4096, 1024, 29, 30, 28, 28, 3, 3, 1, 1, 1, 1, 1, 2, 1, (1 << 61) - 1)]
    bad += [(256, 48, 9, 10, 8, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, T), (512, 256, 8, 10, 8, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, T), (256, 128, 9, 0, 14, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, T),
            (512, 256, 9, 10, 8, 8, 3, 3, 1, 2, 1, 1, 1, 1, 1, T), (512, 256, 9, 10, 8, 8, 11, 3, 1, 1, 1, 1, 1, 1, 1, T), (512, 256, 9, 10, 8, 8, 3, 3, 1, 1, 0, 1, 1, 1, 1, T),
            (512, 256, 9, 10, 8, 8, 3, 3, 1, -1, 1, 1, 1, 1, 1, T), (256, 128, 20, 88, 1, 2, 5, 3, 4, 2, 1, 1, 1, 1, 1, T), (256, 64, 8, 9, 6, 6, 1, 1, 1, 1, 1, 1, 1, 1, 1, T)]
    assert len(cases) >= 30 and len(bad) >= 15
    ws = []
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for c in cases + bad:
            w = rng.randint(-(1 << 62), 1 << 62, size=(c[13], c[14], c[6], c[7])).astype(np.int64)
            w.reshape(-1)[0] = np.iinfo(np.int64).min; w.reshape(-1)[-1] = np.iinfo(np.int64).max
            ws.append(w)
            f.write(" ".join(str(v) for v in c) + "\n" + " ".join(str(int(v)) for v in w.reshape(-1)) + "\n")
    out = subprocess.check_output([exe, path], text=True).split("\n")
    at = 0
    for c, w in zip(cases, ws):
        plan = ca.binding.conv_slots_plan_geom(*c[:13])
        assert [out[at + i].split()[0] for i in range(6)] == ["steps", "elts", "geom", "valid", "fold", "mask"], (c, out[at])
        got = [[int(v) for v in out[at + i].split()[1:]] for i in range(6)]
        assert got[0] == plan.steps and got[1] == plan.elements and got[2] == [plan.out_h, plan.out_w, plan.out_dil, int(plan.needs_clean_input)], c
        assert got[3] == plan.valid and got[4] == plan.fold(w, c[15]).reshape(-1).tolist(), c
        assert got[5] == np.flatnonzero(plan.mask_slots()[:c[1]]).tolist() == sorted(plan.valid), c
        at += 6
    assert out[at:] == ["bad"] * len(bad) + [""]
    for c in bad:
        with pytest.raises(ValueError):
            ca.binding.conv_slots_plan_geom(*c[:13])


def test_model_decrypts_to_the_padded_convolution():
    """the golden set's ring (n = 256, two moduli) with a batching plaintext modulus: a 2 -> 2 channel 3 x 3 'same' layer (pad 1) on 4 x 4 planes with a margin of
    one (pitch 5, origin 6, M = 32), a bias and the mask, through conv_slots_model and the oracle's add_plain and multiply_plain -- the composition the entry
    point is defined as -- decrypts to the biased convolution at the valid slots of every period and to 0 at every other slot"""
    import crcnn_amd as ca
    from oracle import orc
    g0 = dict(np.load(GOLD))
    n, q = int(g0["n"]), [int(v) for v in g0["q"]]
    assert (n, len(q)) == (256, 2)
    t = ca.Engine.slots_prime(n, 20)
    M, half = 32, t // 2
    E = ca.Engine(n, q, t, device=-1)
    O = orc.Oracle(n, q, t)
    GM = gm.GaloisModel(O)
    rng = np.random.RandomState(23)
    img = rng.randint(0, 8, size=(2, 4, 4)).astype(np.int64)
    w = rng.randint(-4, 5, size=(2, 2, 3, 3)).astype(np.int64); w[1, 0, 0, 0] = -4
    bias = np.array([-7, 5], dtype=np.int64)
    plan = E.conv_slots_plan_geom(M, 5, 6, 4, 4, 3, 3, pad=1)
    assert plan.steps == [-6, -5, -4, -1, 0, 1, 4, 5, 6] and plan.valid == [6 + 5 * y + x for y in range(4) for x in range(4)] and plan.out_dil == 1
    keyed = sorted(set(plan.elements) - {1})
    sk, pk = E.keygen(41)
    elts, gk = E.gen_galois_keys(42, sk, elts=keyed)
    kc = {int(g): hm.conjugate_key_coeff(GM, GM.key_coeff(gk[e], 16), int(g)) for e, g in enumerate(elts)}
    planes = np.stack([pm.plane_slots_geom(img[ci], n, M, 5, 6, 1).astype(np.int64) for ci in range(2)])
    x = E.encrypt(pk, E.slots_compose(planes, 2, n, n, 1), 43)
    wl = E.conv_slots_pack_weights(plan.fold(w, t))
    bl = E.conv_slots_pack_bias(bias)
    mask_plain = E.slots_compose(plan.mask_slots().reshape(1, n), 1, n, n, 1).reshape(n)
    y = cm.conv_slots(GM, x, plan.elements, wl, kc)
    want = pm.conv_direct_geom(img, w, 1, bias=bias)
    assert int(np.abs(want).max()) < half
    for co in range(2):
        cplain = np.zeros(n, dtype=np.uint64); cplain[0] = int(bias[co]) % t
        yb = O.add_plain(y[co], cplain)
        assert [int(yb[0, i, 0]) for i in range(2)] == [(int(y[co][0, i, 0]) + int(bl[i, co])) % q[i] for i in range(2)]     # the packed word is what was added
        ym = O.multiply_plain(yb, mask_plain)
        assert O.noise_budget(sk, ym) >= 1
        got = E.slots_decompose(O.decrypt(sk, ym), n, n, 1).reshape(-1)
        for base in range(0, n, M):
            assert [int(got[base + s]) for s in plan.valid] == [int(v) for v in want[co].reshape(-1)], (co, base)
        assert all(int(got[i]) == 0 for i in range(n) if i % M not in plan.valid)
    E.close()
