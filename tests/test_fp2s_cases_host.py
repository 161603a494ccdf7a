"""The cases and checkers of tests/test_gpu_fp2s.py, checked without a GPU: the case list really holds what it promises (every kind in every full
wave, one wave with a lone active pair, a partial workgroup), the checkers accept an output computed in Python integers and REJECT every mutated
one -- a half taken from the wrong coordinate, c0 and c1 exchanged, the identity where a doubling is due, a doubling where the identity is due,
the identity where the generic branch is due, one lane's verdict flipped."""
import primitive_cases as PC


def _rejects(f, *a):
    try:
        f(*a)
    except AssertionError:
        return True
    return False


def test_the_waves_hold_every_kind_at_once():
    p, q, flags, kinds, names = PC.fp2s_curve_waves()
    PC.assert_fp2s_waves_are_mixed(kinds, flags)
    assert len(p) % PC.S_PAIRS != 0
    per = {k: kinds.count(k) for k in PC.S_KINDS}
    assert all(v >= 2 for v in per.values()), per
    cases = PC.fp2s_curve_cases()
    present = {PC.s_kind(*PC._case_values(c)) for c in cases}
    assert present == set(PC.S_KINDS), present
    # the _2p forms are among the operands: a ZZ half written as the limbs of p, on a point that is the identity and on one that is not
    pl = PC.limbs(PC.Q)
    zz_p = [c for c in cases if list(c[1][36:45]) == pl or list(c[1][45:54]) == pl or list(c[2][36:45]) == pl or list(c[2][45:54]) == pl]
    assert {PC.s_kind(*PC._case_values(c)) for c in zz_p} >= {"ZZ half zero", "O+A", "A+O", "O+O"}
    # a mixed wave that FAILS the census is noticed
    bad = [("ordinary" if k == "P=(0,x)" else k) for k in kinds]
    assert _rejects(PC.assert_fp2s_waves_are_mixed, bad, flags)


def test_the_raw_checker_rejects_every_mutated_output():
    seen = {"exchanged": 0, "lane verdict": 0, "wrong verdict": 0, "off by p limbs": 0}
    for prim, batches in PC.fp2s_batches().items():
        for b in batches:
            for i in range(len(b)):
                good = PC.fp2s_expected(prim, b, i)
                PC.check_fp2s(prim, b, i, good)
                if prim in ("mul", "sqr", "mul2sub"):
                    swapped = good[9:] + good[:9]
                    if swapped != good:
                        assert _rejects(PC.check_fp2s, prim, b, i, swapped), (prim, b.name, i)
                        seen["exchanged"] += 1
                    off = list(good)
                    off[0] ^= 1
                    assert _rejects(PC.check_fp2s, prim, b, i, off), (prim, b.name, i)
                    seen["off by p limbs"] += 1
                elif prim in ("is_zero", "is_zero_2p"):
                    one_lane = list(good)
                    one_lane[9] ^= 1
                    assert _rejects(PC.check_fp2s, prim, b, i, one_lane), (prim, b.name, i)
                    both = list(good)
                    both[0] ^= 1
                    both[9] ^= 1
                    assert _rejects(PC.check_fp2s, prim, b, i, both), (prim, b.name, i)
                    seen["lane verdict"] += 1
                    seen["wrong verdict"] += 1
                else:
                    assert _rejects(PC.check_fp2s, prim, b, i, good[9:] + good[:9])
    assert all(v > 0 for v in seen.values()), seen
    # the zero tests see exactly-one-half-zero operands of both orders, as values 0, p and beyond
    zb = PC.fp2s_batches()["is_zero"][0].rows
    assert any(a % PC.Q == 0 and b % PC.Q for ((a, b),) in zb) and any(a % PC.Q and b % PC.Q == 0 for ((a, b),) in zb)


def test_the_curve_checker_rejects_every_mutated_output():
    p, q, flags, kinds, names = PC.fp2s_curve_waves()
    seen = {k: 0 for k in ("half from the wrong coordinate", "c0 and c1 exchanged", "identity for a doubling", "doubling for the identity",
                           "identity for the generic branch", "generic for a half-zero ZZ treated as the identity")}
    for i in range(len(p)):
        if kinds[i] is None:
            continue
        fl = int(flags[i])
        good = PC.fp2s_curve_good_output("add", p[i], q[i], fl)
        PC.check_fp2s_curve("add", p[i], q[i], fl, good)
        wrong_half = good[18:27] + good[9:18] + good[0:9] + good[27:]          # x.c0 <-> y.c0: one lane's coordinate offset off by one
        if wrong_half != good:
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, wrong_half), (i, names[i])
            seen["half from the wrong coordinate"] += 1
        exch = [w for k in range(4) for w in good[18 * k + 9:18 * k + 18] + good[18 * k:18 * k + 9]]
        if exch != good:
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, exch), (i, names[i])
            seen["c0 and c1 exchanged"] += 1
        pv, qv = PC._case_values((names[i], p[i], q[i], fl))
        if kinds[i] == "doubling":
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, [0] * 72), (i, names[i])
            seen["identity for a doubling"] += 1
        if kinds[i] in ("cancelling", "P=0 R=(0,x)", "P=0 R=(x,0)"):
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, PC.pt_raw(PC.xyzz_dbl_ref(pv))), (i, names[i])
            seen["doubling for the identity"] += 1
        if kinds[i] in ("P=(0,x)", "P=(x,0)"):
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, [0] * 72), (i, names[i])
            assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, PC.pt_raw(PC.xyzz_dbl_ref(pv))), (i, names[i])
            seen["identity for the generic branch"] += 1
        if kinds[i] == "ZZ half zero":
            for other in (p[i], q[i]):
                assert _rejects(PC.check_fp2s_curve, "add", p[i], q[i], fl, [int(v) for v in other]), (i, names[i])
            seen["generic for a half-zero ZZ treated as the identity"] += 1
    assert all(v > 0 for v in seen.values()), seen
    dp, dq, dflags = PC.fp2s_double_waves()
    for i in range(len(dp)):
        if dflags[i] & PC.S_ACTIVE:
            good = PC.fp2s_curve_good_output("double", dp[i], dq[i], int(dflags[i]))
            PC.check_fp2s_curve("double", dp[i], dq[i], int(dflags[i]), good)
            exch = [w for k in range(4) for w in good[18 * k + 9:18 * k + 18] + good[18 * k:18 * k + 9]]
            assert exch == good or _rejects(PC.check_fp2s_curve, "double", dp[i], dq[i], int(dflags[i]), exch), i
            assert not PC.raw_pt(dp[i])[2].is_zero()


def test_the_reference_formulas_are_the_group_law_on_curve_points(pyoracle):
    """xyzz_add_ref / xyzz_dbl_ref over Fq2 integers against Curve.add on the G2 group cases: the reference of the off-curve sets is sound"""
    cur = pyoracle.G2
    ps, qs, want, names = PC.curve_case_arrays(cur, "add_xyzz_stream")
    for k in range(len(want)):
        pt, qt = (tuple(PC._abi_f2(r[8 * j:8 * j + 8]) for j in range(4)) for r in (ps[k], qs[k]))
        (x, y, zz, zzz), _ = PC.xyzz_add_ref(pt, qt)
        assert (None if zz.is_zero() else (x * zz.inv(), y * zzz.inv())) == want[k], names[k]
