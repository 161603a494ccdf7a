"""The long pipeline at the edges of its bucket reduction, through the C ABI (kg_msm, kg_msm_begin / kg_msm_end) with the short kernel switched off
(kg_msm_set_small(0)): G2 (the lane-pair Fp2S kernels), G1 and Grumpkin, 600 pairs over a pool of a dozen subgroup points and their negatives
(tests/long_edge_cases.py; tests/test_long_edges_host.py shows that the inputs really put equal, opposite, empty and ordinary nodes into level 1 of
the halving tree at every width used here).

Widths: the two staircases at every c from 2 to 13, the other patterns at c = 2, 8, 9, 10, 11, 13 and the automatic width.  With B = 2^(c-1) buckets
against TailCfg::L (128 for the lane pair, 256 for one lane) these are: the unfused gather with the run-time-length tail (B < L), the unfused gather
with the len == L tail, k_gather_halve with no k_halve level (B = 2 L), with one level (B = 4 L) and with several.  Every cell runs as a blocking
call (the tail is k_reduce_tail_coop on one-lane arithmetic) and as one of two tickets in flight (k_reduce_tail<KF, ...>), and must give the C
oracle's affine point bit for bit; where the sum has a closed form, (sum k mod r) P from pyoracle as well.

A note on the task length: msm_sort_begin clamps T = 2 n / B + 16 to at least 32, so a bucket of all 600 pairs is cut into 19 partial sums at
c = 8 AND at c = 13 (k_gather_sum: at most GATHER_SUM_MAX = 32) and never counts as hot (more than 32 T = 1024 entries).  The hot-bucket tree
(k_hot_sum / k_hot_fold) and, with KG_HOT_SUM=0, the lane-by-lane rounds (k_sum_tasks) are therefore reached with the same one-bucket patterns
at HOT_N = 1100 pairs, where the phase record is asserted; the 600-pair cells run everywhere as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

import long_edge_cases as LE
from helpers import CURVES, pt_to_np
from test_gpu_parity import SEED, aff, gpu_aff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT_N = LE.HOT_N
NB = {"g1": 4, "gk": 4, "g2": 8}


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    c.set_msm_small(0)              # every length through the long pipeline
    yield c
    c.close()


_want = {}


def want_of(O, pat):
    """the C oracle's affine point of a pattern, once; equal to the closed form in big integers where there is one"""
    key = (pat.cv, pat.name, len(pat.ks))
    if key not in _want:
        cur = CURVES[pat.cv][1]
        w = aff(O, pat.cv, O.msm(pat.cv, pat.bases, pat.scalars, pat.inf, threads=8))
        if pat.closed is not None:
            pt = cur.mul(cur.gen, pat.closed)
            assert w == (None if pt is None else pt_to_np(cur, pt).tobytes()), (pat.cv, pat.name, "closed form")
        _want[key] = w
    return _want[key]


class Dev:
    """a pattern's arrays on the device"""

    def __init__(self, ctx, pat):
        self.n = len(pat.ks)
        self.b, self.s = ctx.upload(pat.bases), ctx.upload(pat.scalars)
        self.i = ctx.upload(pat.inf) if pat.inf is not None else None
        self.inf = self.i.ptr if self.i is not None else 0


def run_cells(ctx, O, cv, pats, widths):
    """every (pattern, width): blocking, then each pattern as ticket 0 and as ticket 1 of two calls in flight.  Returns the cells that ran."""
    curve, nb = CURVES[cv][0], NB[cv]
    dev = [Dev(ctx, p) for p in pats]
    want = [want_of(O, p) for p in pats]
    cells = 0
    for c in widths:
        ctx.set_msm_window(c)
        try:
            for j, p in enumerate(pats):
                d = dev[j]
                assert gpu_aff(ctx.msm(curve, d.b.ptr, d.inf, d.s.ptr, d.n), nb) == want[j], (cv, p.name, c, "blocking")
                k = (j + 1) % len(pats)
                e = dev[k]
                ctx.msm_begin(curve, d.b.ptr, d.inf, d.s.ptr, d.n, 0)
                ctx.msm_begin(curve, e.b.ptr, e.inf, e.s.ptr, e.n, 1)
                got0, got1 = ctx.msm_end(curve, 0), ctx.msm_end(curve, 1)
                assert gpu_aff(got0, nb) == want[j], (cv, p.name, c, "ticket 0")
                assert gpu_aff(got1, nb) == want[k], (cv, pats[k].name, c, "ticket 1")
                cells += 3
        finally:
            ctx.set_msm_window(0)
    return cells


def phases_of(ctx, curve, d):
    ctx.profile_enable(True)
    try:
        out = ctx.msm(curve, d.b.ptr, d.inf, d.s.ptr, d.n)
        return out, ctx.profile_summary()
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("cv", ["g2", "g1", "gk"])
def test_staircases_at_every_width(ctx, oracle, cv):
    """one base under scalars 1 .. 600 (level-1 nodes add equal points, higher levels equal points in non-trivial ZZ) and the same with P / -P by
    the scalar's parity, both ways (level-1 nodes cancel, later levels add identities), c = 2 .. 13.  No bucket is hot: neither the tree nor a
    partial-sum round may appear in the phase record."""
    pats = [p for p in LE.patterns(cv) if "staircase" in p.name]
    assert len(pats) == 3
    cells = run_cells(ctx, oracle, cv, pats, LE.STAIR_WIDTHS)
    curve = CURVES[cv][0]
    for c in (8, 13):
        ctx.set_msm_window(c)
        try:
            out, ph = phases_of(ctx, curve, Dev(ctx, pats[0]))
        finally:
            ctx.set_msm_window(0)
        assert gpu_aff(out, NB[cv]) == want_of(oracle, pats[0])
        assert "hot_sum" not in ph and "partial_round" not in ph and "gather" in ph and "reduce" in ph, (cv, c, ph)
    print(f"long edges {cv}: staircases, {cells} cells (3 patterns x {len(LE.STAIR_WIDTHS)} widths x blocking / ticket 0 / ticket 1)")


@pytest.mark.parametrize("cv", ["g2", "g1", "gk"])
def test_one_bucket_sparse_and_mixed_inputs(ctx, oracle, cv):
    """one base under one scalar (random, all ones, alternating +-P: a bucket's equal partial sums double in k_gather_sum), three non-zero scalars
    among zeros with identity flags (identities on one or both sides of almost every node), and the parity tests' edge mix over the pool"""
    pats = [p for p in LE.patterns(cv) if "staircase" not in p.name]
    assert len(pats) == 5
    cells = run_cells(ctx, oracle, cv, pats, LE.OTHER_WIDTHS)
    print(f"long edges {cv}: one bucket x 3, sparse, edge_mix: {cells} cells (5 patterns x {len(LE.OTHER_WIDTHS)} widths x 3 call forms)")


@pytest.mark.parametrize("cv", ["g2", "g1", "gk"])
def test_hot_bucket_tree_on_repeated_bases(ctx, oracle, cv):
    """one bucket per window with more partial sums than the gather takes: k_hot_sum / k_hot_fold fold EQUAL partial sums (doublings at every tree
    node) or alternating ones (identities); c = 13 and the automatic width, blocking and in flight; the phase record shows hot_sum.  The same at
    600 pairs, c = 13, is an ordinary k_gather_sum bucket of 19 partial sums: no hot_sum there (see the module's note)."""
    curve = CURVES[cv][0]
    pats = LE.hot_patterns(cv)
    cells = run_cells(ctx, oracle, cv, pats, (13, 0))
    ctx.set_msm_window(13)
    try:
        for p in pats:
            out, ph = phases_of(ctx, curve, Dev(ctx, p))
            assert gpu_aff(out, NB[cv]) == want_of(oracle, p), (cv, p.name)
            assert "hot_sum" in ph and "partial_round" not in ph, (cv, p.name, ph)
        small = LE.patterns(cv)[3]
        out, ph = phases_of(ctx, curve, Dev(ctx, small))
        assert gpu_aff(out, NB[cv]) == want_of(oracle, small)
        print(f"long edges {cv}: one bucket of 600 at c = 13: phases {sorted(ph)}")
        assert "hot_sum" not in ph and "partial_round" not in ph, (cv, ph)
    finally:
        ctx.set_msm_window(0)
    print(f"long edges {cv}: hot bucket of {HOT_N}: {cells} cells, hot_sum observed for {len(pats)} patterns at c = 13")


def test_degenerate_inputs_of_the_parity_test_through_the_long_pipeline(ctx, oracle):
    """the inputs of test_msm_degenerate_inputs_hit_the_exceptional_branches (6000 pairs, G1; that test runs the short kernel today): one base under
    one scalar, under scalar 1, alternating P / -P, and the same with an odd one out -- blocking and as two tickets"""
    O, n = oracle, 6000
    P_ = O.gen_bases(0, SEED + 95, 0, 1)[0]
    k = O.gen_scalars(0, SEED + 96, 0, 1)[0]
    one = O.f_consts(0)["r"]
    negP = P_.copy(); negP[4:] = O.f_neg(1, P_[4:])
    same = np.tile(P_, (n, 1))
    alt = same.copy(); alt[1::2] = negP
    odd = alt.copy(); odd[-1] = P_
    sk = np.tile(k, (n, 1))
    sk_odd = sk.copy(); sk_odd[-1] = one
    jobs = [(same, sk), (same, np.tile(one, (n, 1))), (alt, sk), (odd, sk_odd)]
    want = [aff(O, "g1", O.msm("g1", b, s, None, threads=8)) for b, s in jobs]
    assert want[2] is None and all(w is not None for w in (want[0], want[1], want[3]))
    dev = [(ctx.upload(b), ctx.upload(s)) for b, s in jobs]
    for j, (db, ds) in enumerate(dev):
        assert gpu_aff(ctx.msm(0, db.ptr, 0, ds.ptr, n), 4) == want[j], (j, "blocking")
        eb, es = dev[(j + 1) % len(dev)]
        ctx.msm_begin(0, db.ptr, 0, ds.ptr, n, 0)
        ctx.msm_begin(0, eb.ptr, 0, es.ptr, n, 1)
        assert gpu_aff(ctx.msm_end(0, 0), 4) == want[j], (j, "ticket 0")
        assert gpu_aff(ctx.msm_end(0, 1), 4) == want[(j + 1) % len(dev)], (j, "ticket 1")


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import kogarashi_amd as K
from kogarashi_amd import lib as L
from oracle import oracle as O
import long_edge_cases as LE
import test_gpu_long_edges as T
assert [r["value"] for r in L.tuning_table() if r["env"] == "KG_HOT_SUM"] == [0]
ctx = K.Context(0)
ctx.set_msm_small(0)
pats = [p for p in LE.patterns("g2") if p.name.startswith("one bucket")] + LE.hot_patterns("g2")
cells = T.run_cells(ctx, O, "g2", pats, (13, 0))
ctx.set_msm_window(13)
for p in LE.hot_patterns("g2"):
    out, ph = T.phases_of(ctx, 2, T.Dev(ctx, p))
    assert T.gpu_aff(out, 8) == T.want_of(O, p), p.name
    assert "partial_round" in ph and "hot_sum" not in ph, (p.name, ph)
ctx.set_msm_window(0)
print("ok", cells)
"""


def test_lane_by_lane_rounds_on_the_lane_pair_in_a_fresh_process():
    """k_sum_tasks<Fp2S> is reached by default only beyond 4096 hot buckets: the one-bucket patterns on G2 with KG_HOT_SUM=0 (600 pairs and the hot
    bucket of HOT_N), blocking and in flight; the phase record of the hot bucket shows partial_round and no hot_sum"""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, KG_HOT_SUM="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    print("long edges g2, KG_HOT_SUM=0:", r.stdout.strip().splitlines()[-1])
