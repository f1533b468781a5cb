"""Which kernel a 64-bit row transform takes, without a GPU: the pure selector of crcnn_amd/csrc/ntt_select.h (ntt_launch in kernels.hip launches what it
chooses) walked by tests/cpp/ntt_select_check.cpp against expectations that program writes out itself -- the rows of the DESIGN.md table "Which kernel a transform
takes" under default tuning, the tuning switches ntt_wave (bit by bit), ntt_split = 0 and ntt_inv61_loose case by case, and the refusals.  The prefetch kernel, the
one-image kernel at n = 16384 and the loose 61-bit kernel are run by no GPU test: their selection is pinned here and nowhere else.  The program stands alone (the
header needs no HIP) and is built with the address and undefined-behaviour sanitizers; nothing sanitized is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ntt_select_check.cpp")


def test_the_selector_reproduces_the_table_the_switches_and_the_refusals(tmp_path):
    exe = str(tmp_path / "ntt_select_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "crcnn_amd", "csrc"), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok", r.stdout
    f = dict(zip(last[1::2], (int(v) for v in last[2::2])))
    # default tuning: 10 rings (64 .. 32768) x 10 classes (nine widths beside a 54-bit modulus, the 61-bit base) x 2 directions x 7 prologues x addend x 4 fused
    # products x box x offered post_mul
    assert f["cases"] == 10 * 10 * 2 * 7 * 2 * 4 * 2 * 2, r.stdout
    # the typed-out tuning cases: counted in the source, so that a row lost from the array fails here
    text = open(SRC).read()
    table = text[text.index("static const Case CASES[] = {"):text.index("static const Class &class_named")]
    typed = len(re.findall(r"^    \{\d+, \"", table, re.M))
    assert typed >= 90 and f["tuning"] == typed, (typed, r.stdout)
    # refusals: 10 classes x 9 rings x (2 addend x 4 products x (1 + 3 directions) + 2 empty launches) + 10 classes x 3 masks x 2 x 7 x 4 at n = 32768
    # + 4 rings x 3 products x 12 + 4 rings x 10 + 5 small rings x 7 x 2 + 4 rings x 4 strict classes x 7
    assert f["refusals"] == 10 * 9 * (2 * 4 * 4 + 2) + 10 * 3 * 2 * 7 * 4 + 4 * 3 * 12 + 4 * 10 + 5 * 7 * 2 + 4 * 4 * 7, r.stdout
    # distinct instantiations default tuning names: all 83 of the translation unit but the four prefetch kernels and ntt_rows_kernel<true, false, 0 / 4 / 6>
    # (ntt_inv61_loose only) -- 52 wave-local, 9 + 3 one-image, 12 split; the program checks that the 60 of profiles/ntt_paths_kernels.md are among them
    assert f["names"] == 52 + 9 + 3 + 12, r.stdout
