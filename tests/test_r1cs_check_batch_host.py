"""The batched R1CS check without a device: tests/host/r1cs_check_batch_host.cpp (the argument checks of kg_r1cs_check_batch and
kg_groth16_witness_check_batch, the device-side scaling of u against the host's, the split source's index rule, the per-vector fold over a
simulated grid) as a stand-alone program, plain -- which includes the bound-checked type -- and under AddressSanitizer + UBSan; the case set
of tests/r1cs_check_batch_cases.py checked against its own promises from the case data alone; and the new entries' refusals that need no
device, through the built library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import r1cs_cases as RC
import r1cs_check_batch_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "r1cs_check_batch_host.cpp")
SECTIONS = ["args", "u Fr", "u Fq", "u Fr checked", "u Fq checked", "split", "fold", "r1cs check batch host"]


def _build(tmp, san):
    exe = str(tmp / ("r1cs_check_batch_host_san" if san else "r1cs_check_batch_host"))
    flags = ["-O1", "-DKG_R1CS_HOST_PLAIN_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ok: ")]


def test_host_program_plain_and_bound_checked(tmp_path):
    assert _run(_build(tmp_path, san=False)) == SECTIONS


def test_host_program_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    assert _run(_build(tmp_path, san=True)) == [s for s in SECTIONS if "checked" not in s]


def _is_long(sh):
    return sh.row_lengths().max(axis=0) > 48


@pytest.mark.parametrize("fd", [0, 1])
def test_case_set_is_what_its_construction_promises(oracle, fd):
    sh, vecs = BC.case300(oracle, fd)
    ln = sh.row_lengths()
    # every promised row class: the 48 / 49 edge, 200, 254 and 5000 entries, rows empty everywhere
    assert ln[0, RC.EDGE48] == 48 and ln[1:, RC.EDGE48].max() <= 6 and ln[2, RC.EDGE49] == 49 and ln[:2, RC.EDGE49].max() <= 6
    assert ln[:, RC.LONG_ROW].tolist() == [200, 200, 200] and ln[1, RC.HUGE_ROW] == 5000
    assert (ln[0, 20:60:7] == 254).all() and (ln[1, 21:60:7] == 254).all() and (ln[2, 22:60:7] == 254).all()
    assert ln[:, RC.EMPTY_A].tolist() == [0, 0, 0] == ln[:, RC.EMPTY_B].tolist()
    long_rows = _is_long(sh)
    assert not long_rows[RC.EDGE48] and long_rows[RC.EDGE49] and 10 < long_rows.sum() < 40
    assert [v.name for v in vecs] == ["satisfied", "E perturbed", "flip_z", "every row bad", "u = 0", "u = p - 1"]
    want = [v.want(sh) for v in vecs]
    assert want[0][1:] == (0, 300) and not want[0][0].any()                                     # at least one vector is fully satisfied
    assert np.flatnonzero(want[1][0]).tolist() == RC.perturbed_rows(300)
    st = want[2][0]
    assert st[RC.LONG_ROW] and st[RC.FLIP_SHORT_B] and st[RC.FLIP_SHORT_C] and not st[RC.EMPTY_A] and 3 <= st.sum() < 300
    assert want[3][1:] == (300, 0) and want[3][0].all()
    assert want[4][1:] == (4, RC.LONG_ROW + 3) and vecs[4].ui == 0 and want[5][1:] == (2, RC.EDGE48) and vecs[5].ui == sh.p - 1
    for v, w in zip(vecs, want):                                                                # a vector meant to have a bad long row has one
        assert bool(w[0][long_rows].any()) == v.long_bad, v.name
        assert set(np.unique(w[0]).tolist()) <= {0, RC.KG_ROW_UNSAT}
    # no two vectors share a summary -- with their u and E, and on the same z with u = 1 and E = 0
    assert BC.distinct_summaries(sh, vecs) and BC.distinct_summaries(sh, vecs, plain=True)
    plain = [v.want(sh, plain=True) for v in vecs]
    assert plain[5][1:] == (0, 300) and any(w[0][long_rows].any() for w in plain)               # z = 0 satisfies the plain relation
    # what pack() hands the entry: the vectors where the strides say, non-canonical words in the gaps
    z, u, e = BC.pack(sh, vecs, sh.nvars + 3, sh.m + 5)
    assert z.shape == (6, sh.nvars + 3, 4) and e.shape == (6, sh.m + 5, 4) and u.shape == (6, 4)
    assert (z[2, :sh.nvars] == vecs[2].z).all() and (z[:, sh.nvars:, 3] >> np.uint64(63)).all() and (e[:, sh.m:, 3] >> np.uint64(63)).all()
    assert RC.to_ints(e[4, :sh.m], sh.p) == vecs[4].e and RC.to_ints(u[3:4], sh.p) == [1]


@pytest.mark.parametrize("fd", [0, 1])
def test_small_cases_and_the_grid_limit_case(oracle, fd):
    for m in BC.SMALL_SIZES:
        sh, vecs = BC.small_case(oracle, fd, m)
        want = [v.want(sh) for v in vecs]
        rows = RC.perturbed_rows(m)
        assert want[0][1:] == (0, m) and want[1][1:] == (len(rows), 0) and want[2][1:] == (1, m - 1)
        if m == 1:
            assert {w[1:] for w in want} == {(0, 1), (1, 0)}                                    # a single row has no third summary
        else:
            assert BC.distinct_summaries(sh, vecs)
        long_rows = _is_long(sh)
        assert long_rows.any() == (m > 12)                                                      # m <= 12 has no work list
        for v, w in zip(vecs, want):
            assert bool(w[0][long_rows].any()) == v.long_bad, (m, v.name)
    if fd == 0:
        sh, base, special = BC.ymax_case(oracle)
        assert sh.row_lengths().tolist() == [[1, 49, 1], [1, 1, 1], [1, 1, 1]] and _is_long(sh).tolist() == [False, True, False]
        assert base.want(sh)[1:] == (0, 3) and sorted(special) == [65534, 65535, 65536] and BC.YMAX_COUNT == 65537
        assert [special[k].want(sh)[1:] for k in sorted(special)] == [(1, 2), (1, 0), (1, 1)]
        assert special[65536].long_bad and special[65536].want(sh)[0][1]                        # the second chunk's vector fails through the list


def test_new_entries_refuse_bad_arguments_without_a_device():
    from kogarashi_amd import build, lib as L
    import kogarashi_amd as K
    build.build()
    so = L.load()
    assert "kg_r1cs_check_batch" in L.EXPORTS and "kg_groth16_witness_check_batch" in L.EXPORTS
    csr = L.Csr()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)                                                     # never dereferenced: every call below is refused first
    ref = C.byref(csr)
    assert so.kg_r1cs_check_batch(None, 0, ref, ref, ref, 1, p, 1, 1, None, None, 0, None, 0, p) == -2            # no context
    assert so.kg_r1cs_check_batch(p, 2, ref, ref, ref, 1, p, 1, 1, None, None, 0, None, 0, p) == -2               # unknown field
    assert so.kg_r1cs_check_batch(p, 0, ref, ref, ref, 1 << 32, p, 1, 1, None, None, 0, None, 0, p) == -2         # m >= 2^32
    assert so.kg_r1cs_check_batch(p, 0, ref, ref, ref, 1, p, 1, 1, None, None, 0, None, 0, None) == -2            # no summary
    assert so.kg_r1cs_check_batch(p, 0, ref, ref, ref, 1, p, 1, 1, None, None, 0, None, 0, p) == -2               # null member arrays
    assert so.kg_r1cs_check_batch(p, 0, None, None, None, 1, None, 0, 0, None, None, 0, None, 0, None) == 0       # count == 0: nothing to do
    assert so.kg_groth16_witness_check_batch(None, ref, ref, ref, 1, 1, 1, p, 1, p, 1, 1, None, 0, p) == -2
    assert so.kg_groth16_witness_check_batch(p, ref, ref, ref, 1, 0, 1, p, 1, p, 1, 0, None, 0, p) == -2          # l < 1, even when empty
    assert so.kg_groth16_witness_check_batch(p, ref, ref, ref, 1, 2, 1, p, 1, p, 1, 1, None, 0, p) == -2          # x_stride < l
    assert so.kg_groth16_witness_check_batch(p, ref, ref, ref, 1, 1, 2, p, 1, p, 1, 1, None, 0, p) == -2          # w_stride < m_l_1
    assert so.kg_groth16_witness_check_batch(p, None, None, None, 1, 1, 1, None, 1, None, 1, 0, None, 0, None) == 0
    assert not any(buf)
    assert all(hasattr(K.Context, n) for n in ("r1cs_check_batch", "groth16_witness_check_batch"))
    assert hasattr(K.Prover, "check_witnesses") and hasattr(K.NovaProver, "check_batch")
    import inspect
    assert inspect.signature(K.Prover.create_proofs_batch_from_witness).parameters["check"].default is False
