"""The batched transform without a device: the pure parts of kogarashi_amd/csrc/ntt_batch.h (launch-group rule, group boundaries, per-step
strides, argument checks) as a stand-alone program, plain and under AddressSanitizer + UBSan, and kg_ntt_batch_plan through the built
library."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ntt_batch_plan_host.cpp")


def _build_and_run(tmp, san):
    exe = str(tmp / ("ntt_batch_plan_host_san" if san else "ntt_batch_plan_host"))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 failures")


def test_group_rule_strides_and_argument_checks(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _build_and_run(tmp_path, san=True)


@pytest.fixture(scope="module")
def lib():
    from kogarashi_amd import build, lib as L
    build.build()
    return L


def test_batch_plan_through_the_library_without_a_device(lib):
    assert {"kg_ntt_bn254_fr_batch", "kg_fr_divide_by_z_on_coset_batch", "kg_ntt_batch_plan"} <= set(lib.EXPORTS)
    assert lib.load().kg_version() == 6
    # (groups, per_launch): the grid's y limit up to 2^11 (no scratch), then 2^23 scratch elements per group
    assert lib.ntt_batch_plan(11, 1) == (1, 65535) and lib.ntt_batch_plan(11, 65536) == (2, 65535)
    assert lib.ntt_batch_plan(12, 2048) == (1, 2048) and lib.ntt_batch_plan(12, 2049) == (2, 2048)
    assert lib.ntt_batch_plan(22, 2) == (1, 2) and lib.ntt_batch_plan(22, 5) == (3, 2)
    assert lib.ntt_batch_plan(23, 3) == (3, 1) and lib.ntt_batch_plan(28, 1) == (1, 1)
    assert lib.ntt_batch_plan(0, 4) == (0, 0) and lib.ntt_batch_plan(29, 4) == (0, 0)
    assert lib.ntt_batch_plan(10, 0) == (0, 65535)
    assert lib.load().kg_ntt_batch_plan(C.c_uint32(12), C.c_size_t(5000), None) == 3        # the out-pointer is optional


def test_batched_entries_refuse_bad_arguments_without_a_device(lib):
    so = lib.load()
    fake = (C.c_uint64 * 64)()                      # never dereferenced: the arguments are looked at first
    ctx, data = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    bad = [(None, data, 4, 1, 16), (ctx, None, 4, 1, 16), (ctx, data, 0, 1, 16), (ctx, data, 29, 1, 1 << 29), (ctx, data, 4, 1, 15),
           (ctx, data, 4, 1 << 60, 16), (ctx, data, 4, 2, (1 << 64) - 1)]
    for c, d, k, cnt, stride in bad:
        assert so.kg_ntt_bn254_fr_batch(c, d, k, cnt, stride, 0, 0) == -2, (k, cnt, stride)
        assert so.kg_fr_divide_by_z_on_coset_batch(c, d, k, cnt, stride) == -2, (k, cnt, stride)
    import kogarashi_amd as K
    assert all(hasattr(K.Context, n) for n in ("ntt_batch", "divide_by_z_on_coset_batch"))
    assert all(hasattr(K.Fft, n) for n in ("batch", "divide_by_z_on_coset_batch"))
