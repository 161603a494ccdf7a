"""R1CS satisfiability without a device: the row arithmetic of kg_r1cs_check (kogarashi_amd/csrc/vecops.h: the row sums, sat_residual_row,
is_zero_mod_p -- the lines vec.hip's kernels compile) built for the host as a stand-alone program and compared, status byte by status byte,
with Python integers; the same program on the bound-tracking type and under AddressSanitizer + UBSan; the case set itself; and the new
entry's argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import r1cs_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "r1cs_check_host.cpp")
SIZES = (1, 65, 300)


@pytest.fixture(scope="module")
def records(oracle):
    """[(shape, z, u or None, E or None, expected status)]: what the host program is asked, in file order"""
    recs = []
    for fd in (0, 1):
        for m in SIZES:
            sh = RC.Shape(oracle, fd, m)
            rows = RC.perturbed_rows(m)
            for name, u, ui in RC.u_values(oracle, fd):
                e = RC.satisfying_e(sh, ui)
                recs.append((sh, sh.z, u, RC.to_mont(e, sh.p), RC.expected(sh, ui, e)[0]))                 # every row holds
                pe = RC.perturb(sh, e, rows)
                recs.append((sh, sh.z, u, RC.to_mont(pe, sh.p), RC.expected(sh, ui, pe)[0]))
            recs.append((sh, sh.z, None, None, RC.expected(sh, 1, None)[0]))                                # the plain relation on random data
            if m > 12:
                ui = RC.u_values(oracle, fd)[-1]
                z2, prods2 = sh.flip_z()
                recs.append((sh, z2, ui[1], RC.to_mont(RC.satisfying_e(sh, ui[2]), sh.p), RC.expected(sh, ui[2], RC.satisfying_e(sh, ui[2]), prods2)[0]))
    return recs


def _build(tmp, san):
    exe = str(tmp / ("r1cs_check_host_san" if san else "r1cs_check_host"))
    flags = ["-O1", "-DKG_R1CS_HOST_PLAIN_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("r1cs_check_host"), san=False)


def _run(exe, tmp, records, mode=None):
    cases, out = str(tmp / "cases.bin"), str(tmp / "status.bin")
    with open(cases, "wb") as f:
        for sh, z, u, e, _ in records:
            RC.write_record(f, sh, z, u, e)
    r = subprocess.run([exe, cases, out] + ([mode] if mode else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.fromfile(out, dtype=np.uint8)


def _compare(got, records):
    at = 0
    for k, (sh, z, u, e, want) in enumerate(records):
        g = got[at:at + sh.m]
        assert (g == want).all(), (k, sh.fd, sh.m, u is None, e is None, np.flatnonzero(g != want)[:8])
        at += sh.m
    assert at == len(got)


def test_case_set_is_what_its_construction_promises(oracle):
    """the shapes hold the row classes they name; E := Az o Bz - u Cz satisfies every row; a perturbed E breaks exactly the perturbed rows, the
    all-empty one with E = 1; the flipped z entry breaks the long row and the short rows that read it"""
    for fd in (0, 1):
        sh = RC.Shape(oracle, fd, 300)
        ln = sh.row_lengths()
        assert ln[:, RC.EMPTY_A].tolist() == [0, 0, 0] == ln[:, RC.EMPTY_B].tolist()
        assert ln[:, RC.LONG_ROW].tolist() == [200, 200, 200]
        assert ln[0, RC.EDGE48] == 48 and ln[1:, RC.EDGE48].max() <= 6 and ln[2, RC.EDGE49] == 49 and ln[:2, RC.EDGE49].max() <= 6
        assert ln[1, RC.HUGE_ROW] == 5000 and (ln[0, 20:60:7] == 254).all() and (ln[1, 21:60:7] == 254).all() and (ln[2, 22:60:7] == 254).all()
        for t in sh.mats:                                                # repeated columns inside a row, coefficients +1 and -1
            assert len(set(t[1][int(t[0][RC.LONG_ROW]):int(t[0][RC.LONG_ROW + 1])].tolist())) < 200
            vals = RC.to_ints(t[2], sh.p)
            assert 1 in vals and sh.p - 1 in vals
        rows = RC.perturbed_rows(300)
        assert {0, 299, 63, 64, 255, 256, RC.EMPTY_A, RC.LONG_ROW, RC.LONG_ROW + 3} == set(rows)
        for name, u, ui in RC.u_values(oracle, fd):
            e = RC.satisfying_e(sh, ui)
            assert RC.expected(sh, ui, e)[1:] == (0, 300), name
            pe = RC.perturb(sh, e, rows)
            st, bad, first = RC.expected(sh, ui, pe)
            assert np.flatnonzero(st).tolist() == rows and (bad, first) == (len(rows), 0), name
            assert e[RC.EMPTY_A] == 0 == e[RC.EMPTY_B] and pe[RC.EMPTY_A] == 1 and pe[RC.EMPTY_B] == 0
            assert {(a - b) % sh.p for a, b in zip(pe, e) if a != b} >= {1, sh.p - 1} and any(a == 0 != b for a, b in zip(pe, e))
        name, u, ui = RC.u_values(oracle, fd)[-1]
        z2, prods2 = sh.flip_z()
        st = RC.expected(sh, ui, RC.satisfying_e(sh, ui), prods2)[0]
        assert st[RC.LONG_ROW] and st[RC.FLIP_SHORT_B] and st[RC.FLIP_SHORT_C] and not st[RC.EMPTY_A] and 3 <= st.sum() < 300
    sh = RC.Shape(oracle, 0, 1)
    assert sh.row_lengths().tolist() == [[0], [0], [0]] and RC.perturbed_rows(1) == [0]


def test_host_rows_match_python_integers(tmp_path, records, exe):
    _compare(_run(exe, tmp_path, records), records)


def test_host_rows_stay_within_the_arithmetic_bounds(tmp_path, records, exe):
    """the same cases on the bound-tracking FpChecked type: the program aborts if a 64-bit column, a 32-bit limb, a fat constant's domination
    or a Montgomery value bound of fp29.h could be exceeded in the row sums, the residual or the zero test"""
    _compare(_run(exe, tmp_path, records, "checked"), records)


def test_host_rows_under_address_and_ub_sanitizers(tmp_path, records):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _compare(_run(_build(tmp_path, san=True), tmp_path, records), records)


def test_new_entry_refuses_bad_arguments_without_a_device():
    from kogarashi_amd import build, lib as L
    import kogarashi_amd as K
    build.build()
    so = L.load()
    assert "kg_r1cs_check" in L.EXPORTS and K.KG_ROW_UNSAT == 1 and so.kg_version() == 6
    bad, first = C.c_size_t(7), C.c_size_t(7)
    csr = L.Csr()
    z = (C.c_uint64 * 4)()
    args = (C.byref(csr), C.byref(csr), C.byref(csr), C.c_size_t(1), z, None, None, None, C.byref(bad), C.byref(first))
    assert so.kg_r1cs_check(None, 0, *args) == -2                                   # no context
    fake = (C.c_uint64 * 64)()                                                      # never dereferenced: the field is looked at first
    assert so.kg_r1cs_check(C.cast(fake, C.c_void_p), 2, *args) == -2               # unknown field
    assert so.kg_r1cs_check(C.cast(fake, C.c_void_p), -1, *args) == -2
    assert (bad.value, first.value) == (7, 7)
    assert hasattr(K.Context, "r1cs_check") and all(hasattr(K.NovaProver, n) for n in ("check", "is_sat", "is_sat_relaxed")) and hasattr(K.Prover, "check_witness")
