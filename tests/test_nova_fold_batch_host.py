"""The batched Nova fold without a device: tests/host/nova_fold_batch_host.cpp (the argument checks of kg_nova_cross_term_batch,
kg_field_vec_axpy_batch and kg_points_muladd_batch, the cross term's row with device-scaled u against the host-scaled one, the axpy step
on non-canonical words, the index rules, the P + k Q chain over three field types on both curves) as a stand-alone program, plain -- which
includes the bound-checked type -- and under AddressSanitizer + UBSan; and the new entries' refusals that need no device, through the built
library."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "nova_fold_batch_host.cpp")
SECTIONS = ["args", "cross Fr", "cross Fq", "axpy Fr", "axpy Fq", "cross Fr checked", "cross Fq checked", "axpy Fr checked", "axpy Fq checked", "index",
            "chain G1", "chain Grumpkin", "nova fold batch host"]


def _build(tmp, san):
    exe = str(tmp / ("nova_fold_batch_host_san" if san else "nova_fold_batch_host"))
    # (shift-base: the binary GCD of fp_inv.h doubles negative update factors with <<, which C++20 defines and C++17 leaves to the
    # two's-complement machines the project builds for; every other check of -fsanitize=undefined stays on)
    flags = ["-O1", "-DKG_NOVA_HOST_PLAIN_ONLY", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all"] if san else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
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


def test_new_entries_refuse_bad_arguments_without_a_device():
    from kogarashi_amd import build, lib as L
    import kogarashi_amd as K
    build.build()
    so = L.load()
    assert all(n in L.EXPORTS for n in ("kg_nova_cross_term_batch", "kg_field_vec_axpy_batch", "kg_points_muladd_batch"))
    csr = L.Csr()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)                                                     # never dereferenced: every call below is refused first
    ref = C.byref(csr)
    cross, axpy, pts = so.kg_nova_cross_term_batch, so.kg_field_vec_axpy_batch, so.kg_points_muladd_batch
    assert cross(None, 0, ref, ref, ref, 1, p, 1, p, 1, 1, None, None, p, 1) == -2                # no context
    assert cross(p, 2, ref, ref, ref, 1, p, 1, p, 1, 1, None, None, p, 1) == -2                   # unknown field
    assert cross(p, 0, ref, ref, ref, 1 << 32, p, 1, p, 1, 1, None, None, p, 1 << 32) == -2       # m >= 2^32
    assert cross(p, 0, ref, ref, ref, 2, p, 1, p, 1, 1, None, None, p, 1) == -2                   # out_stride < m
    assert cross(p, 0, ref, ref, ref, 2, p, 1, p, 1, 0, None, None, p, 1) == -2                   #   even for an empty call
    assert cross(p, 0, ref, ref, ref, 1, p, 1, p, 1, 1, None, None, p, 1) == -2                   # null member arrays
    assert cross(p, 0, None, None, None, 1, p, 1, p, 1, 1, None, None, p, 1) == -2                # null matrices
    assert cross(p, 0, None, None, None, 1, None, 0, None, 0, 0, None, None, None, 1) == 0        # count == 0: nothing to do
    assert cross(p, 1, None, None, None, 0, None, 0, None, 0, 3, None, None, None, 0) == 0        # m == 0
    assert axpy(None, 0, p, 1, p, p, 1, p, 1, 1, 1) == -2
    assert axpy(p, 2, p, 1, p, p, 1, p, 1, 1, 1) == -2
    assert axpy(p, 0, p, 1, p, p, 2, p, 2, 2, 1) == -2                                            # a stride below n
    assert axpy(p, 0, p, 2, p, p, 2, p, 1, 2, 0) == -2                                            #   even for an empty call
    assert axpy(p, 0, p, 1, None, p, 1, p, 1, 1, 1) == -2                                         # no scalars
    assert axpy(p, 0, None, 1, None, None, 1, None, 1, 1, 0) == 0 and axpy(p, 1, None, 0, None, None, 0, None, 0, 0, 5) == 0
    assert pts(None, 0, p, None, p, None, p, 1, 1, p, p) == -2
    assert pts(p, 2, p, None, p, None, p, 1, 1, p, p) == -2                                       # G2: Nova has none
    assert pts(p, 2, p, None, p, None, p, 1, 0, p, p) == -2                                       #   even for an empty call
    assert pts(p, 0, p, None, p, None, p, 0, 1, p, p) == -2                                       # per_scalar == 0
    assert pts(p, 1, p, None, p, None, None, 2, 2, p, p) == -2                                    # no scalars
    assert pts(p, 1, p, None, p, None, p, 2, 2, p, None) == -2                                    # no result flags
    assert pts(p, 0, None, None, None, None, None, 2, 0, None, None) == 0
    assert not any(buf)
    assert all(hasattr(K.Context, n) for n in ("nova_cross_term_batch", "field_vec_axpy_batch", "points_muladd_batch"))
    assert all(hasattr(K.NovaProver, n) for n in ("fold_begin", "fold_end", "prove_batch"))
