"""Point validation without a device: the per-point predicates of kg_points_check (kogarashi_amd/csrc/points_check.h, the header points.hip's
kernels are built from) compiled for the host as a stand-alone program and compared, status byte by status byte, with Python integers; the same
program once more under AddressSanitizer + UBSan; the generated psi constants; and the two new entries' argument checks."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import points_cases as PC
from helpers import CURVES, pt_to_np
from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "points_check_host.cpp")
SEED = 0x4B6F676172617368


def _valid(name, n):
    _, cur, _ = CURVES[name]
    if cur.ext:
        rnd = random.Random(41)
        return np.stack([pt_to_np(cur, cur.mul(cur.gen, rnd.randrange(1, cur.n))) for _ in range(n)])
    return np.stack([pt_to_np(cur, P.base_at(cur, SEED + 900, i)) for i in range(n)])


@pytest.fixture(scope="module")
def records():
    """[(curve name, checks, xy, inf or None)]: what the host program is asked, in file order"""
    recs = []
    for name in ("g1", "gk", "g2"):
        _, cur, _ = CURVES[name]
        valid = _valid(name, 130)
        for n in (1, 63, 65, 130):
            xy, inf = PC.curve_case(cur, valid, n)
            recs.append((name, PC.KG_CHECK_CURVE, xy, inf))
        xy, inf = PC.curve_case(cur, valid, 130, skip_first_group=True)
        recs.append((name, PC.KG_CHECK_CURVE | PC.KG_CHECK_SUBGROUP, xy, inf))       # G1 / Grumpkin: the subgroup bit does no work
        recs.append((name, PC.KG_CHECK_CURVE, valid[:70], None))                      # nothing to report
    valid = _valid("g2", 140)
    for n in (1, 140):
        xy, _ = PC.g2_subgroup_case(valid, n)
        recs.append(("g2", PC.KG_CHECK_SUBGROUP, xy, None))
        recs.append(("g2", PC.KG_CHECK_CURVE, xy, None))
    return recs


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("points_check_host"), san=False)


def _build(tmp, san):
    exe = str(tmp / ("points_check_host_san" if san else "points_check_host"))
    flags = ["-O1", "-DKG_POINTS_HOST_PLAIN_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    return exe


def _run(exe, tmp, records, mode=None):
    cases, out = str(tmp / "cases.bin"), str(tmp / "status.bin")
    with open(cases, "wb") as f:
        for name, checks, xy, inf in records:
            PC.write_record(f, CURVES[name][0], checks, xy, inf)
    r = subprocess.run([exe, cases, out] + ([mode] if mode else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint8)


def _compare(got, records):
    at = 0
    for name, checks, xy, inf in records:
        want, bad, first = PC.expected(CURVES[name][1], xy, inf, checks)
        g = got[at:at + len(xy)]
        assert (g == want).all(), (name, checks, len(xy), np.flatnonzero(g != want)[:8], g[g != want][:8], want[g != want][:8])
        at += len(xy)
    assert at == len(got)


def test_case_set_is_what_its_construction_promises():
    """the subgroup cases against [r]P = O: in the subgroup exactly where the construction says; both statuses occur; the criterion the kernel
    evaluates (tools/gen/psi_consts.py: criterion) agrees with [r]P = O on every one of them"""
    M = PC.psi_module()
    sp = PC.g2_special_points()
    assert len(sp) >= 38
    for name, pt, ok in sp:
        assert PC.in_subgroup(pt) == ok, name
        assert M.criterion(pt) == ok, name
    # the curve cases: every replacement kind yields the status it is meant to
    for name in ("g1", "gk", "g2"):
        _, cur, _ = CURVES[name]
        w = _valid(name, 1)[0]
        want = {"y+1": 2, "swap": 2, "zero": 2, "x+p": 1, "y=p": 1, "ones": 1, "c1": 2}
        for kind in PC.curve_kinds(cur):
            assert PC.expected_status(cur, PC.corrupt(cur, w, kind), False, 3) == want[kind], (name, kind)
        assert PC.expected_status(cur, PC.corrupt(cur, w, "ones"), True, 3) == 0


def test_host_predicates_match_python_integers(tmp_path, records, exe):
    _compare(_run(exe, tmp_path, records), records)


def test_host_predicates_stay_within_the_arithmetic_bounds(tmp_path, records, exe):
    """the same cases on the bound-tracking FpChecked type: the program aborts if a 64-bit column, a 32-bit limb or a Montgomery value bound of
    fp29.h could be exceeded anywhere in the curve equation, psi or the subgroup chain"""
    _compare(_run(exe, tmp_path, records, "checked"), records)


def test_host_predicates_under_address_and_ub_sanitizers(tmp_path, records):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _compare(_run(_build(tmp_path, san=True), tmp_path, records), records)


def test_psi_constants_are_generated_and_recomputed_from_xi():
    gen = os.path.join(ROOT, "tools", "gen", "psi_consts.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0, "run python tools/gen/psi_consts.py --write"
    hdr = open(os.path.join(ROOT, "kogarashi_amd", "csrc", "psi_consts.h")).read()
    arr = {m.group(1): [int(v[:-1], 16) for v in m.group(2).split(", ")] for m in re.finditer(r"uint32_t (G[XY]_C[01])\[9\] = \{([^}]*)\}", hdr)}
    q = P.Q_MOD
    val = lambda name: sum(l << (29 * i) for i, l in enumerate(arr[name])) * pow(1 << 261, -1, q) % q

    def fq2pow(a, e):
        r = P.Fq2(1, 0)
        for bit in bin(e)[2:]:
            r = r * r
            if bit == "1":
                r = r * a
        return r

    xi = P.Fq2(9, 1)
    gx, gy = fq2pow(xi, (q - 1) // 3), fq2pow(xi, (q - 1) // 2)
    assert all(l < 1 << 29 for v in arr.values() for l in v)
    assert (val("GX_C0"), val("GX_C1")) == (gx.a, gx.b) and (val("GY_C0"), val("GY_C1")) == (gy.a, gy.b)
    x = int(re.search(r"BN_X = (\d+)ull", hdr).group(1))
    assert x == 4965661367192848881 and x.bit_length() == 63 == int(re.search(r"BN_X_BITS = (\d+)", hdr).group(1))
    assert q == 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1 and P.R_MOD == q - 6 * x * x


def test_new_entries_refuse_a_null_context_without_a_device():
    from kogarashi_amd import build, lib as L
    import kogarashi_amd as K
    build.build()
    so = L.load()
    assert {"kg_points_check", "kg_groth16_crs_check"} <= set(L.EXPORTS)
    bad, first = C.c_size_t(7), C.c_size_t(7)
    xy = (C.c_uint64 * 8)()
    rc = so.kg_points_check(None, 0, xy, None, C.c_size_t(1), 1, None, C.byref(bad), C.byref(first))
    assert rc == -2
    crs, out = L.Groth16Crs(), (C.c_size_t * 10)()
    assert so.kg_groth16_crs_check(None, C.byref(crs), 1, out) == -2
    assert (K.KG_CHECK_CURVE, K.KG_CHECK_SUBGROUP, K.KG_PT_NON_CANONICAL, K.KG_PT_OFF_CURVE, K.KG_PT_NOT_IN_SUBGROUP) == (1, 2, 1, 2, 4)
