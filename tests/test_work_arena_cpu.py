"""CPU check of the work-space arena (crcnn_amd/csrc/work_arena.h) that every crc_*_work_bytes function and every entry point's carve-up run on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_counting_and_carving_runs_agree_under_sanitizers():
    """tests/cpp/work_arena_check.cpp, built with the address and undefined-behaviour sanitizers: for 400 random region lists and a base at every offset 0 .. 255
    from a 256-byte boundary, on a host buffer of exactly bytes(): the counting run covers the carving run, every region is 256-byte aligned, no two regions
    overlap, the last region ends inside base + bytes(), and every byte of every region is written and read back"""
    exe = os.path.join(tempfile.mkdtemp(), "work_arena_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crcnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "work_arena_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("ok "), out
    assert int(out.split()[1]) == 400 * 256
