"""Relations between the crc_*_work_bytes functions of the activation family that hold whatever their implementation (host-only contexts, no kernel is launched):
a pass holds at most `chunk` ciphertexts (tuning switch sq_chunk, else 1024 on these rings), so sizes grow with the count up to one pass's worth and stay there;
an entry point that delegates to another, or that adds regions to another's work space, needs at least as much; and every one of them holds the packed keys
and the size-3 products of a pass."""
import itertools

import pytest

Q256 = [0x7fffffff380001, 0x3fffffff000001]
FLAT = ["square_relin", "poly2_relin", "multiply_relin", "poly3_relin"]
POOLED = [((1, 2, 4, 4), (1, 1, 2, 2)), ((2, 3, 12, 12), (1, 1, 3, 3)), ((3, 1, 28, 28), (2, 2, 2, 2)), ((2, 5, 40, 40), (1, 1, 2, 2))]      # (B, zd, xd, yd), (xs, ys, xf, yf)


@pytest.fixture(scope="module", params=[256, 4096], ids=["n256", "n4096"])
def eng(request):
    import crcnn_amd as ca
    n = request.param
    E = ca.Engine(n, Q256 if n == 256 else ca.default_coeff_modulus_128(n), 1 << 20, device=-1)
    yield E
    E.L.crc_ctx_set_tuning(E.c, b"sq_chunk", 0)
    E.close()


def set_chunk(E, sq_chunk):
    """(Engine.set_tuning synchronises a stream, which a host-only context has not)"""
    assert E.L.crc_ctx_set_tuning(E.c, b"sq_chunk", sq_chunk) == 0
    return sq_chunk if sq_chunk else 1024


def flat(E, name, count, dbc):
    return getattr(E.L, f"crc_{name}_work_bytes")(E.c, count, dbc)


@pytest.mark.parametrize("sq_chunk", [0, 2, 16])
@pytest.mark.parametrize("dbc", [8, 16])
def test_flat_sizes(eng, sq_chunk, dbc):
    E = eng
    chunk = set_chunk(E, sq_chunk)
    counts = sorted(set(range(1, 20)) | {chunk - 1, chunk, chunk + 1, 2 * chunk, 3 * chunk + 7} - {0})
    sizes = {name: [flat(E, name, cnt, dbc) for cnt in counts] for name in FLAT}
    for name, s in sizes.items():
        assert all(a <= b for a, b in zip(s, s[1:])), (name, "decreases in count")
        at_chunk = s[counts.index(chunk)]
        assert all(v == at_chunk for cnt, v in zip(counts, s) if cnt >= chunk), (name, "changes beyond one pass")
        if chunk > 1: assert s[counts.index(chunk - 1)] < at_chunk, (name, "a partial pass takes as much as a whole one")
        for cnt, v in zip(counts, s):
            assert v >= 8 * (E.L.crc_evk_words(E.c, dbc) + min(cnt, chunk) * E.L.crc_ct_words(E.c, 3)), (name, cnt)
    for i, cnt in enumerate(counts):
        sq, p2, mu, p3 = (sizes[name][i] for name in FLAT)
        assert p3 >= mu >= sq and p2 >= sq, (cnt, sq, p2, mu, p3)
        # poly2 and poly3 hold their extra regions (the NTT copy of the input; that and relin(x^2)) on top of the delegate's work space
        slab = 8 * min(cnt, chunk) * E.L.crc_ct_words(E.c, 2)
        assert p2 >= sq + slab and p3 >= mu + 2 * slab, (cnt, sq, p2, mu, p3)


@pytest.mark.parametrize("sq_chunk", [0, 16, 200])
@pytest.mark.parametrize("dbc", [8, 16])
def test_pooled_sizes(eng, sq_chunk, dbc):
    E = eng
    chunk = set_chunk(E, sq_chunk)
    for (B, zd, xd, yd), (xs, ys, xf, yf) in POOLED:
        sq = E.L.crc_square_pool_relin_work_bytes(E.c, B, zd, xd, yd, xs, ys, xf, yf, dbc)
        p2 = E.L.crc_poly2_pool_relin_work_bytes(E.c, B, zd, xd, yd, xs, ys, xf, yf, dbc)
        # a pass takes whole planes: as many as fit into `chunk` ciphertexts, one at the least
        cin = min(B * zd, max(chunk // (xd * yd), 1)) * xd * yd
        assert sq >= 8 * (E.L.crc_evk_words(E.c, dbc) + cin * E.L.crc_ct_words(E.c, 3)), (B, zd, xd, yd)
        assert p2 >= sq + 8 * cin * E.L.crc_ct_words(E.c, 2), (B, zd, xd, yd)
        # more planes than a pass holds change nothing
        assert E.L.crc_square_pool_relin_work_bytes(E.c, B + 1, zd, xd, yd, xs, ys, xf, yf, dbc) >= sq
        if cin < B * zd * xd * yd:
            assert E.L.crc_square_pool_relin_work_bytes(E.c, B + 1, zd, xd, yd, xs, ys, xf, yf, dbc) == sq
            assert E.L.crc_poly2_pool_relin_work_bytes(E.c, B + 1, zd, xd, yd, xs, ys, xf, yf, dbc) == p2


def test_invalid_arguments_give_zero(eng):
    E = eng
    set_chunk(E, 0)
    for name, dbc in itertools.product(FLAT, [0, -1, 61]):
        assert flat(E, name, 5, dbc) == 0, (name, dbc)
    for name in FLAT:
        assert getattr(E.L, f"crc_{name}_work_bytes")(None, 5, 16) == 0, name
    for name in ("square_pool_relin", "poly2_pool_relin"):
        f = getattr(E.L, f"crc_{name}_work_bytes")
        assert f(None, 1, 2, 4, 4, 1, 1, 2, 2, 16) == 0 and f(E.c, 1, 2, 4, 4, 1, 1, 2, 2, 0) == 0, name
        assert f(E.c, 1, 2, 4, 4, 1, 1, 5, 2, 16) == 0 and f(E.c, 1, 2, 4, 4, 1, 1, 2, 5, 16) == 0, (name, "window larger than the plane")
        assert f(E.c, 1, 2, 4, 4, 0, 1, 2, 2, 16) == 0 and f(E.c, 1, 2, 4, 4, 1, 0, 2, 2, 16) == 0, (name, "stride 0")
