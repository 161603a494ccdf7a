"""kg_points_check / kg_groth16_crs_check on the device: every status byte, the count and the first bad index against Python integers
(tests/points_cases.py: word values against p, the curve equation, [r]P = O by double-and-add)."""
import os
import subprocess

import numpy as np
import pytest

import points_cases as PC
from helpers import CURVES, pt_to_np
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu
SEED = 0x4B6F676172617368
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 63, 64, 65, 257, 1000]


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def valid(oracle):
    """on-curve points of the three curves, made once: G1 / Grumpkin from the oracle's base generator, G2 as generator multiples"""
    O = oracle
    k = O.gen_scalars(0, SEED + 950, 0, 1000)
    g2, inf = O.fixed_base_mul(2, k)
    assert not inf.any()
    return {"g1": O.gen_bases(0, SEED + 951, 0, 1000), "gk": O.gen_bases(1, SEED + 952, 0, 1000), "g2": g2}


def run(ctx, cid, xy, inf, checks, with_status=True):
    n = len(xy)
    d = ctx.upload(xy)
    di = ctx.upload(inf) if inf is not None else None
    st = ctx.empty((n,), dtype=np.uint8) if with_status else None
    bad, first = ctx.points_check(cid, d.ptr, di.ptr if di else 0, n, checks, st.ptr if st else 0)
    return (st.numpy() if st else None), bad, first


def assert_matches(ctx, name, xy, inf, checks):
    cid, cur, _ = CURVES[name]
    want, wbad, wfirst = PC.expected(cur, xy, inf, checks)
    got, bad, first = run(ctx, cid, xy, inf, checks)
    assert (got == want).all(), (name, len(xy), checks, np.flatnonzero(got != want)[:8])
    assert (bad, first) == (wbad, wfirst), (name, len(xy), checks)
    _, bad2, first2 = run(ctx, cid, xy, inf, checks, with_status=False)         # d_status = NULL: the summary alone
    assert (bad2, first2) == (wbad, wfirst)
    return want


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["g1", "gk", "g2"])
def test_curve_check(ctx, valid, name, n):
    cur = CURVES[name][1]
    xy, inf = PC.curve_case(cur, valid[name], n)
    want = assert_matches(ctx, name, xy, inf, PC.KG_CHECK_CURVE)
    assert want[0] != 0 and want[n - 1] != 0                                      # index 0 and n - 1 are among the replaced
    if n == 1000:
        assert {int(q) // 64 for q in np.flatnonzero(want)} >= {0, 1, 2, 4, 10, 15}
        xy, inf = PC.curve_case(cur, valid[name], n, skip_first_group=True)       # the lowest bad index outside the first workgroup
        want = assert_matches(ctx, name, xy, inf, PC.KG_CHECK_CURVE | PC.KG_CHECK_SUBGROUP)
        assert int(np.flatnonzero(want)[0]) >= 64 and len({int(q) // 64 for q in np.flatnonzero(want)}) >= 3
    # the same coordinates without a flag array: the two flagged garbage points count
    if n >= 63:
        want2 = assert_matches(ctx, name, xy, None, PC.KG_CHECK_CURVE)
        assert want2.astype(bool).sum() == want.astype(bool).sum() + 2
    # and an array with nothing to report: first_bad = n
    got, bad, first = run(ctx, CURVES[name][0], valid[name][:n], None, PC.KG_CHECK_CURVE)
    assert not got.any() and (bad, first) == (0, n)


@pytest.mark.parametrize("n", [1, 65, 300])
def test_g2_subgroup_check(ctx, valid, n):
    xy, names = PC.g2_subgroup_case(valid["g2"], n)
    want = assert_matches(ctx, "g2", xy, None, PC.KG_CHECK_SUBGROUP)            # the subgroup bit implies the curve check
    assert (want == assert_matches(ctx, "g2", xy, None, PC.KG_CHECK_SUBGROUP | PC.KG_CHECK_CURVE)).all()
    sp = {nm: ok for nm, _, ok in PC.g2_special_points()}
    for i, nm in enumerate(names):
        assert want[i] == (0 if nm == "valid" or sp[nm] else PC.NOT_IN_SUBGROUP), nm
    if n >= 65:
        assert (want == PC.NOT_IN_SUBGROUP).sum() >= 10 and (want == 0).sum() >= 30
    if n == 300:
        assert set(names) >= {nm for nm, _, _ in PC.g2_special_points()}          # the whole case set is in the array
    # the curve check alone reports nothing: every point here is on the curve
    got, bad, first = run(ctx, 2, xy, None, PC.KG_CHECK_CURVE)
    assert not got.any() and (bad, first) == (0, n)
    # flagged as identities, the off-subgroup points are not examined
    got, bad, first = run(ctx, 2, xy, (want != 0).astype(np.uint8), PC.KG_CHECK_SUBGROUP)
    assert not got.any() and (bad, first) == (0, n)


def test_subgroup_chain_on_mixed_defects(ctx, valid):
    """one array with all three statuses: lanes that are non-canonical or off the curve skip the chain, their neighbours run it"""
    cur = P.G2
    xy, _ = PC.g2_subgroup_case(valid["g2"], 130)
    for q, kind in ((0, "ones"), (2, "y+1"), (64, "c1"), (66, "x+p"), (129, "swap")):
        xy[q] = PC.corrupt(cur, valid["g2"][q], kind)
    inf = np.zeros(130, dtype=np.uint8)
    inf[3] = 1
    want = assert_matches(ctx, "g2", xy, inf, PC.KG_CHECK_SUBGROUP)
    assert {1, 2, 4} <= set(int(v) for v in want)


def test_argument_checks_and_empty_input(ctx, valid):
    import kogarashi_amd as K
    d = ctx.upload(valid["g1"][:4])
    assert ctx.points_check(0, d.ptr, 0, 0, 1) == (0, 0)                           # n = 0: nothing read, 0 / 0
    assert ctx.points_check(0, 0, 0, 0, 3) == (0, 0)
    for args in ((0, d.ptr, 0, 4, 0), (0, d.ptr, 0, 4, 4), (0, d.ptr, 0, 4, 7), (3, d.ptr, 0, 4, 1), (-1, d.ptr, 0, 4, 1), (0, 0, 0, 4, 1)):
        with pytest.raises(K.KogarashiError, match="bad argument"):
            ctx.points_check(*args)
    assert ctx.points_check(0, d.ptr, 0, 4, 3) == (0, 4)                           # G1: the subgroup bit is accepted and does no work
    # a CRS of no points at all: the five arrays are skipped, the host points are (0, 0) -- off their curves unless flagged as identities
    from kogarashi_amd.lib import CRS_CHECK_MEMBERS, Groth16Crs
    crs = Groth16Crs()
    crs.delta_g1_inf, crs.delta_g2_inf = 1, 1
    assert ctx.groth16_crs_check(crs, 3) == {**{m: 0 for m in CRS_CHECK_MEMBERS}, "alpha_g1": 1, "beta_g1": 1, "beta_g2": 1}
    for checks in (0, 4):
        with pytest.raises(K.KogarashiError, match="bad argument"):
            ctx.groth16_crs_check(crs, checks)
    crs.m, crs.l, crs.m_l_1 = 2, 1, 1                                              # lengths without arrays
    with pytest.raises(K.KogarashiError, match="bad argument"):
        ctx.groth16_crs_check(crs, 1)


def test_check_points_flags_an_off_subgroup_g2_base(ctx, valid):
    """ADVICE r6 item 1 from the safe side: a G2 array with one on-curve base outside the r-torsion -- the input on which the endomorphism
    split of the short MSM and the long pipeline would disagree -- is caught before it is registered"""
    import kogarashi_amd as K
    T = next(pt for nm, pt, ok in PC.g2_special_points() if nm == "G + T")
    pts = valid["g2"][:40].copy()
    pts[17] = pt_to_np(P.G2, T)
    st = K.api.check_points(pts, curve="g2", ctx=ctx)
    assert st.dtype == np.uint8 and np.flatnonzero(st).tolist() == [17] and st[17] == K.KG_PT_NOT_IN_SUBGROUP
    assert not K.api.check_points(pts, curve="g2", subgroup=False, ctx=ctx).any()
    key = K.PedersenCommitment(pts, curve="g2", ctx=ctx)
    assert key.check() == (1, 17) and key.check(subgroup=False) == (0, 40)
    assert K.PedersenCommitment(valid["gk"][:100], curve="gk", ctx=ctx).check() == (0, 100)


def test_crs_check(ctx, oracle):
    import kogarashi_amd as K
    from kogarashi_amd.api import groth16_setup
    from kogarashi_amd.lib import CRS_CHECK_MEMBERS
    O = oracle
    cs = O.chain_r1cs(64, O.gen_scalars(0, SEED + 960, 0, 1)[0])
    params = groth16_setup(cs.a, cs.b, cs.c, cs.m, cs.l, cs.m_l_1, O.gen_scalars(0, SEED + 961, 0, 5), ctx=ctx)
    clean = K.Prover(params, cs.m, cs.l, cs.m_l_1, ctx=ctx).check_crs()
    assert list(clean) == list(CRS_CHECK_MEMBERS) and not any(clean.values()), clean
    sp = {nm: pt for nm, pt, _ in PC.g2_special_points()}
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in params.items()}
    j = next(i for i in range(len(bad["b_g2"])) if not bad["b_g2_inf"][i])
    bad["b_g2"][j] = pt_to_np(P.G2, sp["T1"])
    k = next(i for i in range(len(bad["l"]) - 1, -1, -1) if not bad["l_inf"][i])
    bad["l"][k] = PC.corrupt(P.G1, bad["l"][k], "y+1")
    bad["vk_g2"][0] = pt_to_np(P.G2, sp["order 10069"])
    prover = K.Prover(bad, cs.m, cs.l, cs.m_l_1, ctx=ctx)
    got = prover.check_crs()
    assert got == {**{m: 0 for m in CRS_CHECK_MEMBERS}, "b_g2": 1, "l": 1, "beta_g2": 1}, got
    got = prover.check_crs(subgroup=False)                                     # the curve check alone sees the off-curve l entry only
    assert got == {**{m: 0 for m in CRS_CHECK_MEMBERS}, "l": 1}, got


def test_cpp_wrappers(tmp_path, valid):
    """include/kogarashi_amd.hpp: check_points and Prover::check_crs from a C++ host (tests/host/points_check_cpp_test.cpp)"""
    exe, lib_dir = str(tmp_path / "points_check_cpp_test"), os.path.join(ROOT, "kogarashi_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "points_check_cpp_test.cpp"),
                           "-L" + lib_dir, "-lkogarashi_amd", "-Wl,-rpath," + lib_dir])
    sp = {nm: pt for nm, pt, _ in PC.g2_special_points()}
    g1 = valid["g1"][:10].copy()
    g1[4] = PC.corrupt(P.G1, g1[4], "y+1")                                         # b_g1[0] off the curve
    g2 = valid["g2"][:5].copy()
    g2[1] = pt_to_np(P.G2, sp["T0"])                                               # b_g2[1] off the subgroup
    g2[3] = pt_to_np(P.G2, sp["order 5864401"])                                    # delta_g2 of order 5864401
    path = str(tmp_path / "points.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(g1), len(g2)], dtype=np.uint64).tobytes() + g1.tobytes() + g2.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "g1: bad 1 first 4 status 0 0 0 0 2 0 0 0 0 0"
    assert lines[1] == "g2: bad 2 first 1 status 0 4 0 4 0"
    assert lines[2] == "g2 curve only: bad 0 first 5 status 0 0 0 0 0"
    assert lines[3] == "crs: 0 0 0 1 1 0 0 0 0 1"
