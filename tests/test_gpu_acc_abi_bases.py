"""The long pipeline's accumulation gathering an unregistered G1 / Grumpkin array as the caller holds it (csrc/msm_bases.h load_point_abi,
KG_ACC_ABI_BASES) against the oracle: 1, 2, 65, 1000 and 8193 pairs forced into the long pipeline (kg_msm_set_small(0)), blocking and with two
tickets in flight; bases that reach every changed branch -- one point under equal scalars (doubling), a point and its negative under equal
scalars (identity, then a first entry again), the generator (x = 1), y = p - 1 on G1 and the golden points with the largest coordinates on
Grumpkin -- under random scalars, all ones and all r - 1; the same arrays with an all-zero identity array and registered (both convert); one G2
call; and everything once more with KG_ACC_ABI_BASES=0 in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import acc_abi_cases as AC
from helpers import CURVES, pt_to_np
from test_gpu_parity import SEED, aff, gpu_aff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_DEFAULT = 32768       # KG_SMALL_MAX
LENGTHS = (1, 2, 65, 1000, 8193)
KINDS = ("random", "ones", "minus_one")
CURVE_IDS = {"g1": (0, 0, 1), "gk": (1, 1, 0)}      # name -> (curve id, scalar field id, base field id)


def make_case(O, cv, n, kind):
    """(bases, scalars) of n pairs: random bases with the special ones in front -- the layout starts at another special pair for n = 2, so that
    the two shortest lengths are a lone generator and P, -P"""
    curve, sfd, bfd = CURVE_IDS[cv]
    cur = CURVES[cv][1]
    bases = O.gen_bases(curve, SEED + 1300 + n, 0, max(n, 8)).copy()
    scal = O.gen_scalars(sfd, SEED + 1301 + n, 0, max(n, 8)).copy()
    sp = [pt_to_np(cur, pt) for _, pt in AC.special_points(cv)]
    neg = sp[1].copy(); neg[4:] = O.f_neg(bfd, sp[1][4:])
    front = [sp[0], sp[0], sp[1], neg, sp[-1], bases[5]]      # gen, gen | S, -S, then a first entry again | another special point
    same = [(1, 0), (3, 2), (5, 2)]                           # scalars made equal: (index, index it copies)
    if n == 2:
        front, same = front[2:4], [(1, 0)]
    for i, b in enumerate(front[:len(bases)]):
        bases[i] = b
    for i, j in same:
        scal[i] = scal[j]
    one = O.f_consts(sfd)["r"]
    if kind == "ones":
        scal[:] = one
    elif kind == "minus_one":
        scal[:] = O.f_neg(sfd, one)                           # r - 1: a negative digit in every window
    return np.ascontiguousarray(bases[:n]), np.ascontiguousarray(scal[:n])


_cases = {}


def case(O, cv, n, kind):
    """the case and the oracle's affine point for it, computed once and shared"""
    key = (cv, n, kind)
    if key not in _cases:
        bases, scal = make_case(O, cv, n, kind)
        _cases[key] = (bases, scal, aff(O, cv, O.msm(cv, bases, scal, None, threads=8)))
    return _cases[key]


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    c.set_msm_small(0)              # every length through the long pipeline
    yield c
    c.close()


def test_the_knob_is_on_by_default():
    from kogarashi_amd import lib as L
    row = [r for r in L.tuning_table() if r["env"] == "KG_ACC_ABI_BASES"]
    assert len(row) == 1 and row[0]["default"] == 1


@pytest.mark.parametrize("cv", ["g1", "gk"])
@pytest.mark.parametrize("n", LENGTHS)
def test_blocking_calls_match_the_oracle_and_the_converting_paths(ctx, oracle, cv, n):
    O, curve = oracle, CURVE_IDS[cv][0]
    zero_inf = ctx.upload(np.zeros(n, dtype=np.uint8))
    for kind in KINDS:
        bases, scal, want = case(O, cv, n, kind)
        db, ds = ctx.upload(bases), ctx.upload(scal)
        got = ctx.msm(curve, db.ptr, 0, ds.ptr, n)                      # gathered in the ABI form
        assert gpu_aff(got, 4) == want, (cv, n, kind)
        assert (ctx.msm(curve, db.ptr, zero_inf.ptr, ds.ptr, n) == got).all(), (cv, n, kind, "identity array: converted")
        ctx.bases_register(curve, db.ptr, 0, n)
        try:
            assert (ctx.msm(curve, db.ptr, 0, ds.ptr, n) == got).all(), (cv, n, kind, "registered")
        finally:
            ctx.bases_unregister(db.ptr)


@pytest.mark.parametrize("cv", ["g1", "gk"])
def test_two_tickets_in_flight(ctx, oracle, cv):
    O, curve = oracle, CURVE_IDS[cv][0]
    jobs = [(n, kind) for n in LENGTHS for kind in KINDS]
    keep, want = [], []
    for n, kind in jobs:
        bases, scal, w = case(O, cv, n, kind)
        keep.append((ctx.upload(bases), ctx.upload(scal)))
        want.append(w)
    for i, (n, _) in enumerate(jobs):
        ctx.msm_begin(curve, keep[i][0].ptr, 0, keep[i][1].ptr, n, i % 2)
        if i >= 1:
            assert gpu_aff(ctx.msm_end(curve, (i - 1) % 2), 4) == want[i - 1], (cv, jobs[i - 1])
    assert gpu_aff(ctx.msm_end(curve, (len(jobs) - 1) % 2), 4) == want[-1], (cv, jobs[-1])


def test_the_abi_form_launches_no_conversion(ctx, oracle):
    """the phase record: no prep_bases phase for a plain unregistered array, one with an identity array"""
    bases, scal, want = case(oracle, "g1", 1000, "random")
    db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(np.zeros(1000, dtype=np.uint8))
    ctx.profile_enable(True)
    try:
        assert gpu_aff(ctx.msm(0, db.ptr, 0, ds.ptr, 1000), 4) == want
        phases = ctx.profile_summary()
        assert "accumulate" in phases and "prep_bases" not in phases, phases
        ctx.profile_enable(True)
        assert gpu_aff(ctx.msm(0, db.ptr, di.ptr, ds.ptr, 1000), 4) == want
        phases = ctx.profile_summary()
        assert "accumulate" in phases and "prep_bases" in phases, phases
    finally:
        ctx.profile_enable(False)


def test_g2_is_untouched(ctx, oracle):
    from test_gpu_small import _g2_bases
    O, n = oracle, 65
    bases = _g2_bases(O, n, SEED + 1390)
    scal = O.gen_scalars(0, SEED + 1391, 0, n)
    bases[5] = bases[4]; scal[5] = scal[4]
    db, ds = ctx.upload(bases), ctx.upload(scal)
    assert gpu_aff(ctx.msm(2, db.ptr, 0, ds.ptr, n), 8) == aff(O, "g2", O.msm("g2", bases, scal, None, threads=8))


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import kogarashi_amd as K
from kogarashi_amd import lib as L
from oracle import oracle as O
import test_gpu_acc_abi_bases as T
from test_gpu_parity import gpu_aff
assert [r["value"] for r in L.tuning_table() if r["env"] == "KG_ACC_ABI_BASES"] == [0]
ctx = K.Context(0)
ctx.set_msm_small(0)
for cv in ("g1", "gk"):
    curve = T.CURVE_IDS[cv][0]
    for n in T.LENGTHS:
        for kind in T.KINDS:
            bases, scal, want = T.case(O, cv, n, kind)
            db, ds = ctx.upload(bases), ctx.upload(scal)
            assert gpu_aff(ctx.msm(curve, db.ptr, 0, ds.ptr, n), 4) == want, (cv, n, kind)
            ctx.msm_begin(curve, db.ptr, 0, ds.ptr, n, 0)
            ctx.msm_begin(curve, db.ptr, 0, ds.ptr, n, 1)
            assert gpu_aff(ctx.msm_end(curve, 0), 4) == want and gpu_aff(ctx.msm_end(curve, 1), 4) == want, (cv, n, kind)
ctx.profile_enable(True)          # the knob is really off: the last array once more, with the phase record
assert gpu_aff(ctx.msm(curve, db.ptr, 0, ds.ptr, n), 4) == want
assert "prep_bases" in ctx.profile_summary()
ctx.profile_enable(False)
print("ok")
"""


def test_knob_off_in_a_fresh_process_gives_the_same_points():
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, KG_ACC_ABI_BASES="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
