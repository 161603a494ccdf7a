"""kg_points_muladd_batch on the device: out_j = affine(P_j + k_{j // per_scalar} Q_j) for many points of G1 or Grumpkin in one launch.
Every word and flag must equal pyoracle's cur.add(P, cur.mul(Q, k)); ordinary and exceptional lanes (identities, P = Q, P = -Q, P = -k Q)
share their waves.  Nothing here has a tolerance."""
import numpy as np
import pytest

from helpers import CURVES, L, pt_to_np
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu
KG_ERR_BAD_ARG = -2
KINDS = ("ordinary", "P identity", "Q identity", "both identity", "P = Q", "P = -k Q", "P = -Q")


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


_TABLES = {}


def tables(cv):
    """per curve: sixteen P candidates, three Q candidates, the six scalars 0, 1, 2, n - 1, 2^127 and a random one, and k Q for each pair"""
    if cv not in _TABLES:
        cur = CURVES[cv][1]
        mult = [cur.gen]
        for _ in range(20):
            mult.append(cur.add(mult[-1], cur.gen))          # mult[i] = (i + 1) G
        ps, qs = mult[:16], [mult[6], mult[10], mult[12]]
        ks = [0, 1, 2, cur.n - 1, 1 << 127, P.scalar_at(P.SEED_BASE + 7700, 0, cur.n)]
        kq = {(qi, ki): cur.mul(q, k) for qi, q in enumerate(qs) for ki, k in enumerate(ks)}
        _TABLES[cv] = (cur, ps, qs, ks, kq)
    return _TABLES[cv]


def build(cv, count, per, identities=True):
    """(p_xy, p_inf, q_xy, q_inf, k, want_xy, want_inf): point j is of kind j % 7 (without identities: the four kinds that have none), its
    scalar the one of its group j // per -- the scalars walk through the six values, so every kind meets every scalar as count grows"""
    cur, ps, qs, ks, kq = tables(cv)
    kinds = KINDS if identities else tuple(k for k in KINDS if "identity" not in k)
    one = L(P.to_mont(1, cur.p))
    rng = np.random.default_rng(count * 16 + per)
    nk = (count + per - 1) // per
    k_arr = np.stack([L(P.to_mont(ks[(g + 3) % 6], cur.n)) for g in range(nk)])
    p_xy, q_xy = np.zeros((count, 8), dtype=np.uint64), np.zeros((count, 8), dtype=np.uint64)
    p_inf, q_inf, w_inf = (np.zeros(count, dtype=np.uint8) for _ in range(3))
    w_xy = np.zeros((count, 8), dtype=np.uint64)
    for j in range(count):
        kind, ki, qi = kinds[j % len(kinds)], (j // per + 3) % 6, j % 3
        pt, q = ps[(5 * j + 1) % 16], qs[qi]
        if kind in ("P identity", "both identity"):
            pt = None
        if kind in ("Q identity", "both identity"):
            q = None
        if kind == "P = Q":
            pt = q
        if kind == "P = -k Q":
            pt = cur.neg(kq[(qi, ki)]) if kq[(qi, ki)] is not None else None
        if kind == "P = -Q":
            pt = cur.neg(q)
        if pt is None and not identities:                    # -0 Q: no flag array to say so, an ordinary lane instead
            pt = ps[(5 * j + 1) % 16]
        want = cur.add(pt, kq[(qi, ki)] if q is not None else None)
        for arr, flags, v in ((p_xy, p_inf, pt), (q_xy, q_inf, q), (w_xy, w_inf, want)):
            flags[j] = v is None
            arr[j] = pt_to_np(cur, v)
        if want is None:
            w_xy[j, 4:] = one                                # the identity is written as (0, 1) with flag 1
        for arr, v in ((p_xy, pt), (q_xy, q)):               # an identity operand's words are never used: anything may lie there
            if v is None:
                arr[j] = rng.integers(0, 1 << 63, 8, dtype=np.uint64) | np.uint64(1 << 63)
    if not identities:
        assert not p_inf.any() and not q_inf.any()
    return p_xy, p_inf, q_xy, q_inf, k_arr, w_xy, w_inf


def run(ctx, cid, case, per, null_flags=False, in_place=False):
    p_xy, p_inf, q_xy, q_inf, k_arr, w_xy, w_inf = case
    count = len(p_xy)
    dp, dpi, dq, dqi, dk = ctx.upload(p_xy), ctx.upload(p_inf), ctx.upload(q_xy), ctx.upload(q_inf), ctx.upload(k_arr)
    guard_xy, guard_inf = np.full((count + 2, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(count + 16, 0xA5, dtype=np.uint8)
    if in_place:
        guard_xy[:count], guard_inf[:count] = p_xy, p_inf
        dp, dpi = ctx.upload(guard_xy), ctx.upload(guard_inf)
        out_xy, out_inf = dp, dpi
    else:
        out_xy, out_inf = ctx.upload(guard_xy), ctx.upload(guard_inf)
    ctx.points_muladd_batch(cid, dp.ptr, 0 if null_flags else dpi.ptr, dq.ptr, 0 if null_flags else dqi.ptr, dk.ptr, per, count, out_xy.ptr, out_inf.ptr)
    xy, inf = out_xy.numpy(), out_inf.numpy()
    assert (xy[count:] == guard_xy[count:]).all() and (inf[count:] == guard_inf[count:]).all(), "written behind the last point"
    assert (inf[:count] == w_inf).all(), (cid, count, per, np.flatnonzero(inf[:count] != w_inf)[:8])
    bad = np.flatnonzero((xy[:count] != w_xy).any(axis=1))
    assert len(bad) == 0, (cid, count, per, [(int(j), KINDS[j % 7]) for j in bad[:8]])
    assert dq.numpy().tobytes() == q_xy.tobytes() and dk.numpy().tobytes() == k_arr.tobytes(), "an input was modified"


@pytest.mark.parametrize("cv", ["g1", "gk"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_every_kind_and_scalar_in_one_launch(ctx, cv, count):
    cid = CURVES[cv][0]
    for per in (1, 2, 3):
        run(ctx, cid, build(cv, count, per), per)
    run(ctx, cid, build(cv, count, 2), 2, in_place=True)
    run(ctx, cid, build(cv, count, 2, identities=False), 2, null_flags=True)


@pytest.mark.parametrize("cv", ["g1", "gk"])
def test_the_case_set_is_what_it_promises(cv):
    """(no device) at 130 points every kind occurs, identity results occur with and without identity operands, every scalar is used"""
    p_xy, p_inf, q_xy, q_inf, k_arr, w_xy, w_inf = build(cv, 130, 2)
    assert p_inf.sum() >= 30 and q_inf.sum() >= 30 and w_inf.sum() >= 25 and (w_inf & ~p_inf & ~q_inf).sum() >= 15
    assert len({k.tobytes() for k in k_arr}) == 6 and len(k_arr) == 65


def test_status_codes(ctx):
    import kogarashi_amd.lib as Lb
    case = build("g1", 5, 2)
    dp, dq, dk = ctx.upload(case[0]), ctx.upload(case[2]), ctx.upload(case[4])
    guard_xy, guard_inf = np.full((5, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(5, 0xA5, dtype=np.uint8)
    ox, oi = ctx.upload(guard_xy), ctx.upload(guard_inf)
    with pytest.raises(Lb.KogarashiError):
        ctx.points_muladd_batch(2, dp.ptr, 0, dq.ptr, 0, dk.ptr, 2, 5, ox.ptr, oi.ptr)            # G2: Nova has none
    for kw in (dict(per=0), dict(p=0), dict(q=0), dict(k=0), dict(ox=0), dict(oi=0)):
        a = dict(p=dp.ptr, q=dq.ptr, k=dk.ptr, per=2, ox=ox.ptr, oi=oi.ptr)
        a.update(kw)
        with pytest.raises(Lb.KogarashiError):
            ctx.points_muladd_batch(0, a["p"], 0, a["q"], 0, a["k"], a["per"], 5, a["ox"], a["oi"])
    ctx.points_muladd_batch(0, 0, 0, 0, 0, 0, 2, 0, 0, 0)                                         # count == 0: nothing to do
    ctx.sync()
    assert (ox.numpy() == guard_xy).all() and (oi.numpy() == guard_inf).all()
