"""The grow-only owner of the context's work spaces (kogarashi_amd/csrc/grow_buf.h) without a device: tests/host/grow_buf_test.cpp drives
it with a counting memory policy, as a stand-alone program, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "grow_buf_test.cpp")


def _build_and_run(tmp, san):
    exe = str(tmp / ("grow_buf_test_san" if san else "grow_buf_test"))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")


def test_grow_rule_failure_moves_and_release_counts(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined (leak detection included): nothing is loaded into Python, nothing is
    preloaded"""
    _build_and_run(tmp_path, san=True)
