"""The work sizes of the client-side refreshes, the flood and the two device encryptors are a contract: callers allocate what crc_*_work_bytes returns.  Every
value of table() below, on host-only contexts (the size calls read n, k and the window; no kernel is launched), against tests/golden/refresh_work_bytes.json,
which `python tests/test_refresh_work_bytes_cpu.py` recorded from this same function before the refreshes were given one shared frame.  No GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refresh_work_bytes.json")
RINGS, KS, COUNTS = (256, 4096), (1, 3), (1, 3, 1025)
# the in-place case, a strided pool, overlapping windows, and a stride beyond the window (refused: 0 bytes)
WINDOWS = [(1, 1, 1, 1, 1, 1), (4, 4, 2, 2, 2, 2), (5, 5, 1, 1, 3, 3), (5, 4, 3, 3, 1, 1)]
REFUSED = WINDOWS[3]
CRT_R = (1, 2, 3, 4)
NO_BASE = (4096, 4)


def table():
    """{row name: bytes} over rings, modulus counts, counts, forms (CRC_NTTP: no ciphertext form), both encryptors, the act windows and the CRT bases"""
    import crcnn_amd as ca
    forms = {"COEFF": ca.COEFF, "NTT": ca.NTT, "NTTP": ca.NTTP}
    q3 = ca.default_coeff_modulus_128(8192)[:3]                   # primes that are 1 mod 2n on both rings
    out = {}
    for n in RINGS:
        # CRT members from crc_slots_crt_primes.  The four smallest primes that are 1 mod 8192 (40961, 65537, 114689, 147457) have a product above 2^63: n = 4096
        # has no base of four, and the r = 4 rows there pin the refusal (0 bytes) of a base that is not supported
        ts = ca.SlotsCrt.primes(n, 4, 15) if n == 256 else ca.SlotsCrt.primes(n, 3, 17) + ca.SlotsCrt.primes(n, 1, 18)
        for k in KS:
            E = [ca.Engine(n, q3[:k], t, device=-1) for t in ts]
            e, L = E[0], E[0].L
            for r in CRT_R:
                assert ca.SlotsCrt(E[:r]).supported == ((n, r) != NO_BASE), (n, k, r)
            for cnt in COUNTS:
                at = f"n{n}_k{k}_count{cnt}"
                out[f"encrypt_dev_{at}"] = L.crc_encrypt_dev_work_bytes(e.c, cnt)
                out[f"encrypt_sym_dev_{at}"] = L.crc_encrypt_sym_dev_work_bytes(e.c, cnt)
                for fname, f in forms.items():
                    out[f"flood_dev_{at}_{fname}"] = L.crc_flood_dev_work_bytes(e.c, cnt, f)
                    for fam in ("refresh", "refresh_sym", "slots_refresh", "slots_refresh_sym"):
                        out[f"{fam}_dev_{at}_{fname}"] = getattr(L, f"crc_{fam}_dev_work_bytes")(e.c, cnt, f)
                    for w in WINDOWS:
                        for fam in ("slots_refresh_act", "slots_refresh_act_sym"):
                            out[f"{fam}_dev_{at}_w{'x'.join(map(str, w))}_{fname}"] = getattr(L, f"crc_{fam}_dev_work_bytes")(e.c, cnt, *w, f)
                    for r in CRT_R:
                        out[f"slots_crt_refresh_dev_{at}_r{r}_{fname}"] = ca.SlotsCrt(E[:r]).refresh_dev_work_bytes(cnt, f)
            for x in E:
                x.close()
    return out


@pytest.fixture(scope="module")
def head():
    return table()


def test_every_size_is_the_recorded_one(head):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(head) == sorted(want), "the table's rows changed: the record must be made again from the commit that last changed a size on purpose"
    diff = {k: (head[k], want[k]) for k in want if head[k] != want[k]}
    assert not diff, diff


def test_what_the_sizes_must_say_whatever_was_recorded(head):
    """no ciphertext form, a refused window and the base that does not exist: 0; everything else: more than the arena's 256 bytes; a refresh holds at least its encryptor's work"""
    for name, v in head.items():
        if name.endswith("_NTTP") or "_w" + "x".join(map(str, REFUSED)) + "_" in name or (name.startswith("slots_crt_refresh_dev_n%d_" % NO_BASE[0]) and "_r%d_" % NO_BASE[1] in name):
            assert v == 0, name
        else:
            assert v > 256, name
    for n in RINGS:
        for k in KS:
            for cnt in COUNTS:
                at = f"n{n}_k{k}_count{cnt}"
                for f in ("COEFF", "NTT"):
                    for fam in ("refresh", "slots_refresh"):
                        assert head[f"{fam}_dev_{at}_{f}"] >= head[f"encrypt_dev_{at}"] and head[f"{fam}_sym_dev_{at}_{f}"] >= head[f"encrypt_sym_dev_{at}"], (fam, at, f)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    with open(GOLDEN, "w") as f:
        json.dump(table(), f, indent=0, sort_keys=True)
        f.write("\n")
