"""Fp2S<Fq>, the lane-pair Fq2 of csrc/fp2s.h, ON THE DEVICE one primitive at a time (tests/device/devprobe.hip: dp_fp2s_raw_ops, dp_fp2s_curve_ops).

The type exists only on the device (c0 on the even lane of a pair, c1 on the odd one, products through mul2pm after a __shfl_xor exchange, zero
tests as the AND of the two lanes' verdicts), so it has no host twin: the references are Python integers (primitive_cases.py) and, for the
canonical value, the one-lane Fp2<Fq> on the same operands.  The stream formulas run through the reduction's own accessors (AosSrc / AosDst /
SoaSrc / SoaDst<Fp2S>), so the half-offsets are checked against the one-lane PointAoS<Fp2> word order."""
import numpy as np
import pytest

import primitive_cases as PC
from test_gpu_primitives import devlib  # noqa: F401  (the probe library, built once per module)

pytestmark = pytest.mark.gpu


def test_lane_pair_raw_primitives(devlib):
    """mul, sqr, mul2sub, is_zero, is_zero_2p, one(): congruence, normalised limbs and the producing primitive's bound by exact integers; the
    canonical value of the one-lane Fp2<Fq> on the same operands (bit equality is counted, not required: the reduction sequences differ)"""
    rows = bit_equal = 0
    for prim, batches in PC.fp2s_batches().items():
        for b in batches:
            out = PC.dev_fp2s(devlib, prim, b)
            PC.check_fp2s_batch(prim, b, out)
            rows += len(b)
            if prim in ("mul", "sqr", "mul2sub"):
                one_lane = PC.dev_raw2(devlib, PC.FP2S_OPS[prim], b)
                assert PC.canonical_halves(out) == PC.canonical_halves(one_lane), (prim, b.name)
                eq = int((out == one_lane).all(axis=1).sum())
                bit_equal += eq
                print(f"fp2s {prim} '{b.name}': {len(b)} rows, {eq} bit-equal to Fp2<Fq>")
    print(f"fp2s raw primitives: {rows} operand rows, {bit_equal} product rows bit-equal to the one-lane type")


@pytest.fixture(scope="module")
def waves():
    p, q, flags, kinds, names = PC.fp2s_curve_waves()
    PC.assert_fp2s_waves_are_mixed(kinds, flags)
    return p, q, flags, kinds, names


def _check_all(op, p, q, flags, out, names, tag):
    for i in range(len(p)):
        if not flags[i] & PC.S_ACTIVE:
            assert (out[i] == PC.FILL).all(), (tag, i, "an idle pair wrote")
            continue
        try:
            PC.check_fp2s_curve(op, p[i], q[i], int(flags[i]), out[i])
        except AssertionError as e:
            raise AssertionError(f"{tag} pair {i} ({names[i]}): {e}; out {[hex(int(v)) for v in out[i]]}") from None


@pytest.mark.parametrize("route", list(PC.S_ROUTES))
def test_lane_pair_additions_through_the_accessors(devlib, waves, route):
    """add_xyzz_stream on XYZZ<Fp2S<Fq>> into a third slot and in place on its first operand, waves that hold every kind at once (the group cases
    of curve_case_arrays(G2) and the half-zero operand sets: a difference with exactly one half zero takes the generic branch, a zero difference
    with a half-zero R gives the identity, a half-zero ZZ is not the identity), one wave whose last pair alone is active, a partial workgroup"""
    p, q, flags, kinds, names = waves
    for inplace in (False, True):
        out = PC.dev_fp2s_curve(devlib, "add", PC.S_ROUTES[route], inplace, p, q, flags)
        _check_all("add", p, q, flags, out, names, (route, "in place" if inplace else "third slot"))
    print(f"fp2s additions, {route}: {len(p)} pairs x 2; per kind {dict((k, kinds.count(k)) for k in PC.S_KINDS)}, idle {kinds.count(None)}")


def test_the_group_cases_give_the_group_law(devlib, pyoracle):
    """the curve points among the cases once more against the big-integer group law (affine), through AosSrc -> SoaDst"""
    cur = pyoracle.G2
    ps, qs, want, names = PC.curve_case_arrays(cur, "add_xyzz_stream")
    raw = lambda rows: np.array([PC.pt_raw(tuple(PC._abi_f2(r[8 * j:8 * j + 8]) for j in range(4))) for r in rows], dtype=np.uint32)
    p, q = raw(ps), raw(qs)
    flags = np.full(len(want), PC.S_ACTIVE, dtype=np.uint8)
    for inplace in (False, True):
        out = PC.dev_fp2s_curve(devlib, "add", 1, inplace, p, q, flags)
        for k in range(len(want)):
            x, y, zz, zzz = PC.raw_pt([int(v) for v in out[k]])
            got = None if zz.is_zero() else (x * zz.inv(), y * zzz.inv())
            assert got == want[k], (names[k], k, inplace)


@pytest.mark.parametrize("route", list(PC.S_ROUTES))
def test_lane_pair_doubling_and_copy_through_the_accessors(devlib, waves, route):
    """double_xyzz_stream (third slot and in place; X or Y with one half zero among the operands) and copy_xyzz_stream (empty slots included)"""
    p, q, flags, kinds, names = waves
    dp, dq, dflags = PC.fp2s_double_waves()
    for inplace in (False, True):
        out = PC.dev_fp2s_curve(devlib, "double", PC.S_ROUTES[route], inplace, dp, dq, dflags)
        _check_all("double", dp, dq, dflags, out, names, (route, "double", inplace))
    out = PC.dev_fp2s_curve(devlib, "copy", PC.S_ROUTES[route], False, p, q, flags)
    _check_all("copy", p, q, flags, out, names, (route, "copy"))
