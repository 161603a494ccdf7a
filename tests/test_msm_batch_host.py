"""The batched short MSM (kg_commit_batch) without a device: the launch-group rule and argument checks of kogarashi_amd/csrc/msm_small_batch.h
and the finish chain of msm_small_finish.h (over the device's field type, the bound-tracking type and the host's type) as a stand-alone
program, plain and under AddressSanitizer + UBSan; kg_commit_batch_plan and the argument checks through the built library."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "msm_batch_host.cpp")

GRID_MAX, CAP, PLANES = 65535, 64 << 20, 8        # msm_small_batch.h: MSM_BATCH_GRID_MAX, MSM_BATCH_SCRATCH_CAP, MSM_BATCH_PLANES


def _build_and_run(tmp, san):
    exe = str(tmp / ("msm_batch_host_san" if san else "msm_batch_host"))
    # (shift-base: the binary GCD of fp_inv.h doubles negative update factors with <<, which C++20 defines and C++17 leaves to the
    # two's-complement machines the project builds for; every other check of -fsanitize=undefined stays on)
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")


def test_group_rule_argument_checks_and_finish_chain(tmp_path):
    _build_and_run(tmp_path, san=False)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    """a plain executable built with -fsanitize=address,undefined: nothing is loaded into Python, nothing is preloaded"""
    _build_and_run(tmp_path, san=True)


@pytest.fixture(scope="module")
def lib():
    from kogarashi_amd import build, lib as L
    build.build()
    return L


def _default_shape(curve, n):
    """(c, r) of msm_small_plan for an n-pair MSM with halved scalars (the default up to 2048 pairs): csrc/msm_small.hip"""
    if curve == 2:
        return (2, 1) if n <= 48 else ((2, 0) if n <= 160 else (4, 1))
    return (2, 1) if n <= 384 else (4, 1)


def _per_launch(curve, n):
    """min(65535, 64 MiB / scratch bytes per vector): W window sums of 4 coordinates in ABI words, and for split windows W x NB x 8 plane
    points of 36 (G2: 72) 32-bit words"""
    if n == 0:
        return GRID_MAX
    c, r = _default_shape(curve, n)
    W, NB = (128 + c - 1) // c, 1 << (c - 1 - r)
    e64, nw = (8, 72) if curve == 2 else (4, 36)
    vb = W * 4 * e64 * 8 + (W * NB * PLANES * nw * 4 if NB > 1 else 0)
    return min(GRID_MAX, CAP // vb)


def test_batch_plan_through_the_library_without_a_device(lib):
    assert {"kg_commit_batch", "kg_commit_batch_plan"} <= set(lib.EXPORTS)
    so = lib.load()
    assert so.kg_version() == 6
    for curve in (lib.KG_G1, lib.KG_G2):
        for n in (0, 1, 384, 385, 2048):
            per = _per_launch(curve, n)
            assert 1 <= per <= GRID_MAX
            for count in (1, per, per + 1, 3 * per + 2):
                assert lib.commit_batch_plan(curve, n, count) == ((count + per - 1) // per, per), (curve, n, count)
            assert lib.commit_batch_plan(curve, n, 0) == (0, 0)
        assert lib.commit_batch_plan(curve, 2049, 7) == (0, 0)           # the form with scalars converted once: single calls
    # the rows differ where the shape does: an unsplit window needs its sums alone, a split one its planes too
    assert _per_launch(0, 384) > _per_launch(0, 385) and _per_launch(2, 1) > _per_launch(2, 2048) and _per_launch(0, 1) == 2 * _per_launch(2, 1)
    assert lib.commit_batch_plan(3, 16, 4) == (0, 0) and lib.commit_batch_plan(-1, 16, 4) == (0, 0)
    assert so.kg_commit_batch_plan(0, C.c_size_t(1000), C.c_size_t(5000), None) == (5000 + _per_launch(0, 1000) - 1) // _per_launch(0, 1000)   # the out-pointer is optional


def test_batched_entry_refuses_bad_arguments_without_a_device(lib):
    so = lib.load()
    fake = (C.c_uint64 * 64)()                      # never dereferenced: the arguments are looked at first
    p = C.cast(fake, C.c_void_p)
    bad = [(None, 0, p, p, 4, 1, 4, p, p),                          # null context
           (p, 0, None, p, 4, 1, 4, p, p), (p, 0, p, None, 4, 1, 4, p, p),    # null bases / scalars with pairs to read
           (p, 0, p, p, 4, 1, 4, None, p), (p, 0, p, p, 4, 1, 4, p, None),    # null outputs
           (p, 0, None, None, 0, 2, 0, None, None),                # n == 0 still writes identities
           (p, 0, p, p, 4, 1, 3, p, p),                            # stride < n
           (p, 3, p, p, 4, 1, 4, p, p), (p, -1, p, p, 4, 1, 4, p, p),         # unknown curve
           (p, 0, p, p, 4, 1 << 60, 16, p, p), (p, 0, p, p, 4, 2, (1 << 64) - 1, p, p),      # count * stride * 32 beyond size_t
           (p, 2, p, p, 0, (1 << 57) + 1, 0, p, p)]                # count G2 points beyond size_t
    for ctx, curve, b, s, n, count, stride, oxy, oinf in bad:
        assert so.kg_commit_batch(ctx, curve, b, None, s, n, count, stride, oxy, oinf) == -2, (curve, n, count, stride)
    import kogarashi_amd as K
    assert hasattr(K.Context, "commit_batch") and hasattr(K.PedersenCommitment, "commit_batch") and callable(lib.commit_batch_plan)
