"""The batched Groth16 prover (kg_groth16_prove_batch) without a device: the group rule, scratch layout and argument checks of
kogarashi_amd/csrc/groth16_batch.h and the chain and assembly formulas of groth16_assemble.h (over the device's field type, the
bound-tracking type and the host's type) as a stand-alone program, plain and under AddressSanitizer + UBSan; kg_groth16_prove_batch_plan
and the argument checks through the built library."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "g16_batch_host.cpp")

POINT_BYTES, CAP_MB = 1024, 256        # groth16_batch.h: G16_BATCH_POINT_BYTES; tuning.h: the default of KG_G16_BATCH_MB


def _build_and_run(tmp, san):
    exe = str(tmp / ("g16_batch_host_san" if san else "g16_batch_host"))
    # (shift-base: the binary GCD of fp_inv.h doubles negative update factors with <<, which C++20 defines and C++17 leaves to the
    # two's-complement machines the project builds for; every other check of -fsanitize=undefined stays on)
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")


def test_group_rule_argument_checks_chain_and_assembly(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _build_and_run(tmp_path, san=True)


@pytest.fixture(scope="module")
def lib():
    from kogarashi_amd import build, lib as L
    build.build()
    return L


def _plan(L, m, l, w, count):
    """the rule restated: per_group = min(count, cap / scratch bytes per proof), at least 1; no groups where kg_commit_batch would not run a
    length batched"""
    if count == 0 or m < 1 or l < 1:
        return 0, 0
    n = 2
    while n < m:
        n *= 2
    lens = [(0, l + w), (2, l + w), (0, w), (0, min(m - 1, n))]
    if any(ln and L.commit_batch_plan(curve, ln, count)[0] == 0 for curve, ln in lens):
        return 0, 0
    per = max(1, min(count, (CAP_MB << 20) // ((3 * n + l + w) * 32 + POINT_BYTES)))
    return (count + per - 1) // per, per


def test_batch_plan_through_the_library_without_a_device(lib):
    assert {"kg_groth16_prove_batch", "kg_groth16_prove_batch_plan"} <= set(lib.EXPORTS)
    so = lib.load()
    assert so.kg_version() == 6
    assert any(r["env"] == "KG_G16_BATCH_MB" and r["default"] == CAP_MB for r in lib.tuning_table())
    for m, l, w in ((1, 2, 1), (2, 2, 2), (5, 2, 5), (16, 2, 16), (100, 2, 100), (1024, 2, 1024), (2046, 2, 2046), (2047, 2, 2047), (7, 3, 0), (2049, 2, 16), (2050, 2, 16)):
        for count in (0, 1, 3, 1000, 100000):
            assert lib.groth16_prove_batch_plan(m, l, w, count) == _plan(lib, m, l, w, count), (m, l, w, count)
    assert lib.groth16_prove_batch_plan(2046, 2, 2046, 4) == (1, 4) and lib.groth16_prove_batch_plan(2047, 2, 2047, 4) == (0, 0)
    assert lib.groth16_prove_batch_plan(2049, 2, 16, 4) == (1, 4) and lib.groth16_prove_batch_plan(2050, 2, 16, 4) == (0, 0)      # h meets m - 1 coefficients
    assert lib.groth16_prove_batch_plan(1024, 2, 1024, 5000) == (3, (CAP_MB << 20) // 132160)
    assert lib.groth16_prove_batch_plan(0, 2, 5, 4) == (0, 0) and lib.groth16_prove_batch_plan(5, 0, 5, 4) == (0, 0)
    assert so.kg_groth16_prove_batch_plan(C.c_size_t(16), C.c_size_t(2), C.c_size_t(16), C.c_size_t(9), None) == 1       # the out-pointer is optional


def test_batched_entry_refuses_bad_arguments_without_a_device(lib):
    so = lib.load()
    fake = (C.c_uint64 * 64)()                      # never dereferenced: the arguments are looked at first
    p = C.cast(fake, C.c_void_p)
    crs = lib.Groth16Crs()
    crs.m, crs.l, crs.m_l_1 = 5, 2, 5

    def call(ctx=p, crs_=crs, a=p, b=p, c=p, es=5, x=p, xs=2, w=p, ws=5, r=p, s=p, count=3, out=p, inf=p):
        return so.kg_groth16_prove_batch(ctx, C.byref(crs_) if crs_ is not None else None, a, b, c, es, x, xs, w, ws, r, s, count, out, inf)

    bad = [dict(ctx=None), dict(crs_=None),
           dict(a=None), dict(b=None), dict(c=None), dict(x=None), dict(w=None), dict(r=None), dict(s=None), dict(out=None), dict(inf=None),
           dict(es=4), dict(xs=1), dict(ws=4), dict(es=4, count=0),                     # a stride shorter than its length
           dict(es=1 << 60, count=16), dict(xs=(1 << 58) + 1, count=2), dict(ws=(1 << 64) - 1, count=2), dict(count=(1 << 56) + 1)]       # products beyond size_t
    for kw in bad:
        assert call(**kw) == -2, kw
    for m, l in ((0, 2), (5, 0), ((1 << 28) + 1, 2)):
        c2 = lib.Groth16Crs()
        c2.m, c2.l, c2.m_l_1 = m, l, 5
        assert call(crs_=c2, es=1 << 29) == -2, (m, l)
    c3 = lib.Groth16Crs()
    c3.m, c3.l, c3.m_l_1 = 5, 2, (1 << 58) + 1
    assert call(crs_=c3, ws=(1 << 58) + 1, count=1) == -2
    import kogarashi_amd as K
    assert hasattr(K.Context, "groth16_prove_batch") and hasattr(K.Prover, "create_proofs_batch") and callable(lib.groth16_prove_batch_plan)
