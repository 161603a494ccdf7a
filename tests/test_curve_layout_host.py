"""kogarashi_amd/csrc/curve_layout.h without a device: which curve ids are accepted and every size of the three curves against the literal
values of the ABI, as a stand-alone program, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "curve_layout_host.cpp")


def _build_and_run(tmp, san):
    exe = str(tmp / ("curve_layout_host_san" if san else "curve_layout_host"))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")


def test_curve_ids_and_layout_sizes(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _build_and_run(tmp_path, san=True)
