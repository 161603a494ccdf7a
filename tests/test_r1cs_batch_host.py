"""The batched CSR product (kg_r1cs_prod_batch) and the batched prover's R1CS form (kg_groth16_prove_r1cs_batch) without a device: the
chunk rule and the argument checks of kogarashi_amd/csrc/r1cs_batch.h as a stand-alone program, plain and under AddressSanitizer + UBSan;
the same argument checks through the built library (nothing is dereferenced, so no device is needed)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "r1cs_batch_host.cpp")
KG_ERR_BAD_ARG = -2


def _build_and_run(tmp, san):
    exe = str(tmp / ("r1cs_batch_host_san" if san else "r1cs_batch_host"))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")


def test_chunk_rule_and_argument_checks(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _build_and_run(tmp_path, san=True)


@pytest.fixture(scope="module")
def lib():
    from kogarashi_amd import build, lib as L
    build.build()
    return L


def test_exports_and_python_entries(lib):
    import kogarashi_amd as K
    assert {"kg_r1cs_prod_batch", "kg_groth16_prove_r1cs_batch"} <= set(lib.EXPORTS)
    assert lib.load().kg_version() == 6
    assert hasattr(K.Context, "r1cs_prod_batch") and hasattr(K.Context, "groth16_prove_r1cs_batch")
    assert hasattr(K.Prover, "create_proofs_batch_from_witness")


def test_batched_product_refuses_bad_arguments_without_a_device(lib):
    so = lib.load()
    fake = (C.c_uint64 * 64)()                      # never dereferenced: the arguments are looked at first
    p = C.cast(fake, C.c_void_p)

    def call(ctx=p, field=0, rp=p, col=p, val=p, m=300, z=p, zs=155, count=5, out=p, os_=300):
        return so.kg_r1cs_prod_batch(ctx, field, rp, col, val, m, z, zs, count, out, os_)

    bad = [dict(ctx=None), dict(field=2), dict(field=-1), dict(rp=None), dict(col=None), dict(val=None), dict(z=None), dict(out=None),
           dict(os_=299), dict(os_=299, count=0), dict(ctx=None, count=0), dict(field=5, m=0, os_=0),
           dict(m=1 << 32, os_=1 << 32), dict(m=1 << 32, os_=1 << 32, count=0),
           dict(zs=1 << 60, count=16), dict(os_=1 << 60, count=16), dict(zs=(1 << 58) + 1, count=2), dict(os_=(1 << 64) - 1, count=2),
           dict(count=(1 << 64) - 1)]
    for kw in bad:
        assert call(**kw) == KG_ERR_BAD_ARG, kw


def test_batched_r1cs_prover_refuses_bad_arguments_without_a_device(lib):
    so = lib.load()
    fake = (C.c_uint64 * 64)()
    p = C.cast(fake, C.c_void_p)
    crs = lib.Groth16Crs()
    crs.m, crs.l, crs.m_l_1 = 5, 2, 5
    full = lib.Csr(p, p, p)

    def call(ctx=p, crs_=crs, a=full, b=full, c=full, x=p, xs=2, w=p, ws=5, r=p, s=p, count=3, out=p, inf=p):
        ref = lambda v: C.byref(v) if v is not None else None
        return so.kg_groth16_prove_r1cs_batch(ctx, ref(crs_), ref(a), ref(b), ref(c), x, xs, w, ws, r, s, count, out, inf)

    bad = [dict(ctx=None), dict(crs_=None), dict(a=None), dict(b=None), dict(c=None),
           dict(a=lib.Csr(None, p, p)), dict(b=lib.Csr(p, None, p)), dict(c=lib.Csr(p, p, None)),
           dict(x=None), dict(w=None), dict(r=None), dict(s=None), dict(out=None), dict(inf=None),
           dict(xs=1), dict(ws=4), dict(xs=1, count=0),
           dict(xs=(1 << 58) + 1, count=2), dict(ws=(1 << 64) - 1, count=2), dict(count=(1 << 56) + 1)]
    for kw in bad:
        assert call(**kw) == KG_ERR_BAD_ARG, kw
    for m, l in ((0, 2), (5, 0), ((1 << 28) + 1, 2)):
        c2 = lib.Groth16Crs()
        c2.m, c2.l, c2.m_l_1 = m, l, 5
        assert call(crs_=c2) == KG_ERR_BAD_ARG, (m, l)
