"""The accumulation's ABI-form gather without a device: tests/host/acc_abi_bases_host.cpp compiles the unpack (fp29.h limbs_from_words_x32), the
conversion the exceptional branches do first (from_ref_x32) and add_mixed_signed(..., abi = true) (curve.h) for the host, on the plain types and on
the bound-tracking FpChecked types -- coordinates 0, 1 and p - 1, an accumulator at its documented maxima, every exceptional branch, real points
of G1 and Grumpkin -- and checks that unpack + conversion is from_ref limb for limb.  The program aborts on a bound violation."""
import os
import subprocess

import numpy as np
import pytest

import acc_abi_cases as AC
from helpers import CURVES, pt_to_np
from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "acc_abi_bases_host.cpp")
SEED = 0x4B6F676172617368


def _points_file(path):
    with open(path, "wb") as f:
        for name, field in (("g1", 0), ("gk", 1)):
            cur = CURVES[name][1]
            pts = [pt for _, pt in AC.special_points(name)] + [P.base_at(cur, SEED + 1200, i) for i in range(12)]
            pts.append(cur.neg(pts[0]))                       # the fold meets P ... -P apart from each other
            xy = np.stack([pt_to_np(cur, pt) for pt in pts])
            np.array([field, len(pts)], dtype=np.uint32).tofile(f)
            xy.astype(np.uint64).tofile(f)


def _build(tmp, flags):
    exe = str(tmp / "acc_abi_bases_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    return exe


def _run(exe, tmp):
    pts = str(tmp / "points.bin")
    _points_file(pts)
    r = subprocess.run([exe, pts], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok records=2"), (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_special_points_are_what_they_are_called():
    for name in ("g1", "gk"):
        cur = CURVES[name][1]
        sp = AC.special_points(name)
        assert all(cur.on_curve(pt) for _, pt in sp)
        assert sp[0][1][0] == 1
    assert AC.special_points("g1")[1][1][1] == P.Q_MOD - 1


def test_abi_gather_bounds_and_conversion(tmp_path):
    _run(_build(tmp_path, ["-O1"]), tmp_path)
