"""tests/sort_cases.py without a GPU: a census of the case lists (every class of input the sort and task kernels branch on is present, computed
from the lists alone), and every checker fed a valid output built by the reference (accepted) and mutated outputs (each rejected)."""
import numpy as np
import pytest

import primitive_cases as PC
import sort_cases as SC


# ---- census ---------------------------------------------------------------------------------------------------------------------------------
def test_probe_entries_are_listed_for_the_export_test():
    assert set(SC.SORT_EXPORTS) <= set(PC.DEV_EXPORTS)


@pytest.mark.parametrize("c", [2, 5, 8, 12, 13, 15, 16, 17, 18, 19, 20])
@pytest.mark.parametrize("field", [0, 1])
def test_census_edge_scalars(field, c):
    """the edge list holds 0, 1, r - 1, powers of two at every window boundary, a sum that carries through every word, a scalar whose signed
    digits are all -2^(c-1) and one whose digits are all 0; every one of them recomposes from its digits (asserted by Digits)"""
    ks = SC.scalar_values(field, c)
    r, W, H = SC.MODULUS[field], SC.windows(c), SC.bias(c)
    dg = SC.Digits(ks, c)
    assert {0, 1, r - 1} <= set(ks)
    for w in range(1, W):
        assert (1 << (w * c)) in ks or (1 << (w * c)) >= r
        assert (1 << (w * c)) - 1 in ks or (1 << (w * c)) - 1 >= r
    carries = []
    for k in ks:
        cy, n = 0, 0
        for j in range(8):
            cy = (((k >> (32 * j)) & 0xFFFFFFFF) + ((H >> (32 * j)) & 0xFFFFFFFF) + cy) >> 32
            n += cy
        carries.append(n)
    assert max(carries) >= 7                                # a carry out of each of the seven lower words
    assert (dg.d[:W - 1] == -(1 << (c - 1))).all(axis=0).any()
    assert (dg.d == 0).all(axis=0).any()
    assert dg.m.max() <= (1 << (c - 1))                     # a bucket number never leaves the window's row


def test_census_scalar_cases():
    prep, pc, op, gs = SC.prep_cases(), SC.prep_count_cases(), SC.onepass_cases(), SC.group_scatter_cases()
    for field in (0, 1):
        assert {n for f, c, n, kind, seed in prep if f == field} >= set(SC.PREP_NS) == {1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5}
        assert {kind for f, c, n, kind, seed in prep if f == field} >= {"mix", "zero", "largest", "uniform"}
    assert {x[5] for x in pc} == {1, 2, 3, 8, 9} and all(x[4] % 4096 == 0 and x[3] % x[4] and x[4] * x[5] >= x[3] for x in pc)
    assert {(x[1], x[2]) for x in pc} >= {(12, 7), (16, 7), (17, 7), (18, 7), (19, 9), (20, 9)} and {x[0] for x in pc} == {0, 1}
    assert {x[1] for x in op} == {2, 5, 8, 13, 15, 16} and {x[3] for x in op} == {1, 2, 3, 8, 9} and {x[0] for x in op} == {0, 1}
    assert {(x[1], x[2], x[3]) for x in gs} == {(12, 7, 16), (16, 7, 256), (17, 7, 512), (18, 7, 1024), (19, 9, 512), (20, 9, 1024)}
    assert {(x[2], x[10], x[11]) for x in gs} == {(fb, t, nt) for fb in (7, 9) for t, nt in SC.GS_PAIRS}
    assert {x[1] for x in gs if x[7]} == {16, 17}                                       # merged
    assert any(x[8] > 0 and x[8] + x[9] < SC.windows(x[1]) for x in gs)                 # a window group: w0 > 0 and a grid narrower than W
    assert all(x[4] > x[10] or x[12] != "mix" or x[4] <= 4097 for x in gs)
    assert max(x[4] for x in gs) > 8192                                                  # more than one tile of the largest size


def test_census_group_sizes():
    for fb in (7, 9):
        S = SC.seg_len(fb)
        sizes = np.concatenate([fc.gsize.reshape(-1) for fc in SC.fine_cases() if fc.fb == fb])
        assert {0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 7} <= set(int(v) for v in sizes)
        multi = np.concatenate([fc.multi for fc in SC.fine_cases() if fc.fb == fb])
        assert multi.any() and not multi.all()                                           # a window with MULTI_SEG and one without
        scan = np.concatenate([g.gsize.reshape(-1) for g in SC.group_scan_cases() if g.seg == S])
        assert {0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 7} <= set(int(v) for v in scan)
    for fc in SC.fine_cases():
        assert fc.maxseg > fc.nseg.max()                                                 # workgroups past the last segment exist
    fc = SC.fine_cases()[0]
    nz = np.nonzero(fc.gsize[0])[0]
    assert nz[0] > 0 and nz[-1] < fc.G - 1 and (np.diff(nz) > 1).any()                   # empty groups before, between and after
    gsc = SC.group_scan_cases()
    assert any(g.nch % 8 for g in gsc) and {g.nt for g in gsc} == {256, 512} and any(g.multi.any() and not g.multi.all() for g in gsc)
    assert any(m.multi for m in SC.merge_cases()) and not all(m.multi for m in SC.merge_cases())
    assert any(SC.SEG in m.gsize_m and SC.SEG + 1 in m.gsize_m for m in SC.merge_cases())


def test_census_task_cases():
    tc = SC.task_cases()
    assert {t.T for t in tc} >= {32, 48, 2048} and {t.top_w >= 0 for t in tc} == {True, False}
    for shift in (0, 1, 2):
        for T in (32, 48):
            v = np.concatenate([t.bsize[0] for t in tc if t.shift == shift and t.T == T])
            assert {0, 1, T - 1, T, T + 1, 32 * T, 32 * T + 1, 17 * T + 1} <= set(int(x) for x in v)
        hot = [t for t in tc if t.shift == shift and t.maxv[1]]
        assert hot and any((t.bsize == 32 * t.t).any() for t in hot)
        assert any(((t.Tb == t.t >> shift) & t.hot).any() for t in hot)
    big_per_wg = []
    for t in tc:
        big = (t.ntask.reshape(-1) - 1 > SC.BIG).astype(np.int64)
        big = np.concatenate([big, np.zeros(-len(big) % 1024, dtype=np.int64)]).reshape(-1, 1024).sum(axis=1)
        big_per_wg.append(int(big.max()))
    assert any(0 < b <= SC.BIG_CAP for b in big_per_wg) and any(b > SC.BIG_CAP for b in big_per_wg)
    assert any((t.ntask - 1 == SC.BIG + 1).any() for t in tc)                            # exactly BIG + 1 full tasks
    rows = [t for t in tc if t.B <= 4096]
    per = {t.B: (t.B + 255) // 256 for t in rows}
    assert {2, 16, 256, 1024, 4096} <= set(per) and any(1000 < B < 1024 * 2 and p & 3 for B, p in per.items())
    assert any(p & 3 == 0 for p in per.values()) and any(p & 3 for p in per.values())    # vector and scalar paths
    assert {t.B for t in tc if t.nsplit} == {8192, 32768, 65536, 1 << 19}
    assert any(t.maxv[1] > t.hot_cap for t in tc) and all(t.hot_cap == 8 for t in tc)
    assert any(not t.bsize.any() for t in tc) and any((~t.bsize.any(axis=1)).any() and t.bsize.any() for t in tc)


# ---- the checkers accept what the reference builds and reject mutations ---------------------------------------------------------------------
def rejects(check, out):
    with pytest.raises(AssertionError):
        check(out)


@pytest.fixture(scope="module")
def onepass():
    dg = SC.Digits(SC.scalar_set(0, 8, 700, 1), 8)
    return SC.OnePass(dg, 3)


def onepass_out(op):
    return {"sorted": SC.OBuf(op.W * op.n, init=op.model_sorted())}


def test_onepass_checker(onepass):
    op = onepass
    op.check_scatter(onepass_out(op))
    w = 1
    b = int(np.nonzero((op.bsize[w][:-1] > 0) & (op.bsize[w][1:] > 0))[0][0])             # two neighbouring non-empty buckets
    o = onepass_out(op)
    row = o["sorted"].own.reshape(op.W, op.n)[w]
    p, q = int(op.bstart[w][b]), int(op.bstart[w][b + 1])
    row[p], row[q] = row[q], row[p]                                                       # two entries exchanged between neighbouring buckets
    rejects(op.check_scatter, o)
    o = onepass_out(op)
    o["sorted"].own[op.n * w + 3] ^= 0x80000000                                           # a sign flipped
    rejects(op.check_scatter, o)
    o = onepass_out(op)
    o["sorted"].own[op.n * w + int(op.bsize[w].sum())] = 7                                # a word behind the lists written
    rejects(op.check_scatter, o)
    o = onepass_out(op)
    o["sorted"].a[-1] ^= 1                                                                # a guard word touched
    rejects(op.check_scatter, o)
    o = {"cnt": SC.OBuf(op.hist.size, init=op.hist)}
    op.check_count(o)
    o["cnt"].own[5] += 1
    rejects(op.check_count, o)
    o = {"cnt": SC.OBuf(op.prefix.size, init=op.prefix), "bsize": SC.OBuf(op.bsize.size, init=op.bsize)}
    op.check_scan(o)
    o["bsize"].own[0] += 1
    rejects(op.check_scan, o)


def test_prep_checkers():
    dg = SC.Digits(SC.scalar_set(1, 12, 300, 2), 12)
    o = {"kt": SC.OBuf(8 * dg.n, init=dg.kt), "cnt": SC.OBuf(dg.W * 1 * 16, init=dg.hist(1, 4096, 7))}
    SC.check_prep(o, dg)
    SC.check_prep_count(o, dg, 7, 1, 4096)
    o["cnt"].own[3] += 1
    rejects(lambda x: SC.check_prep_count(x, dg, 7, 1, 4096), o)
    o["kt"].own[7 * dg.n] ^= 1
    rejects(lambda x: SC.check_prep(x, dg), o)


def test_group_scan_and_merge_checkers():
    for gc in SC.group_scan_cases():
        gc.check(gc.model())
    gc = SC.group_scan_cases()[0]
    o = gc.model()
    o["segbase"].own[gc.G] &= 0x7FFFFFFF                                                   # MULTI_SEG dropped
    rejects(gc.check, o)
    o = gc.model()
    o["segbase"].own[2 * (gc.G + 1) - 1] |= 0x80000000                                    # MULTI_SEG on a window without a larger group
    rejects(gc.check, o)
    o = gc.model()
    o["bsize"].own[gc.W * gc.B] = 0                                                       # a word behind the windows' sizes cleared
    rejects(gc.check, o)
    o = gc.model()
    o["zero"].own[gc.zwords - 1] = SC.FILL                                                # the last zero word not cleared
    rejects(gc.check, o)
    o = gc.model()
    o["gstart"].a[-3] = 0                                                                 # a guard word touched
    rejects(gc.check, o)
    for mc in SC.merge_cases():
        mc.check(mc.model())
    mc = SC.merge_cases()[0]
    o = mc.model()
    o["segbase_m"].own[mc.G] &= 0x7FFFFFFF
    rejects(mc.check, o)
    o = mc.model()
    o["woff"].own[mc.G + 8] += 1
    rejects(mc.check, o)


@pytest.mark.parametrize("merged", [False, True])
def test_group_scatter_checker(merged):
    dg = SC.Digits(SC.scalar_set(0, 16, 900, 3), 16)
    gs = SC.GroupScatter(dg, 7, 256, 2, 500, merged, 0, dg.W)
    gs.check(gs.model())
    o = gs.model()
    t = o["tmp"].own
    g = int(np.nonzero((gs.gsize[0][:-1] > 0) & (gs.gsize[0][1:] > 0))[0][0])
    if merged:
        p, q = int(gs.gstart[g]), int(gs.gstart[g + 1])
    else:
        p, q = int(gs.gstart[0][g]), int(gs.gstart[0][g + 1])
    t[p], t[q] = t[q], t[p]                                                               # exchanged between neighbouring groups
    rejects(gs.check, o)
    o = gs.model()
    o["tmp"].own[0] ^= 1 << 24                                                            # a fine bit wrong
    rejects(gs.check, o)
    if merged:
        o = gs.model()
        o["tmp"].own[0] ^= 1 << gs.mshift                                                 # the window tag wrong
        rejects(gs.check, o)
    part = SC.GroupScatter(dg, 7, 256, 2, 500, False, 2, 3)
    part.check(part.model())
    o = part.model()
    o["tmp"].own[0] = 5                                                                   # a window outside the grid written
    rejects(part.check, o)


@pytest.mark.parametrize("i", range(len(SC.fine_cases())))
def test_fine_checkers_accept_the_model(i):
    fc = SC.fine_cases()[i]
    fc.check_local(fc.model_local())
    fc.check_scatter(fc.model_scatter())


def test_fine_checkers_reject_mutations():
    fc = SC.fine_cases()[0]
    W, F, n = fc.Wg, fc.FINE, fc.n
    o = fc.model_local()
    g = 5                                                                                 # SEGN - 1 entries spread over the buckets: a single segment
    b = g * F + int(np.nonzero((fc.bsize[0, g * F:(g + 1) * F - 1] > 0) & (fc.bsize[0, g * F + 1:(g + 1) * F] > 0))[0][0])
    row = o["sorted"].own.reshape(W, n)[0]
    p, q = int(fc.bstart[0, b]), int(fc.bstart[0, b + 1])
    row[p], row[q] = row[q], row[p]                                                       # exchanged between neighbouring buckets
    rejects(fc.check_local, o)
    o = fc.model_local()
    o["sorted"].own[p] |= 3 << 24                                                         # a fine field left in an output entry
    rejects(fc.check_local, o)
    o = fc.model_local()
    o["sorted"].own[p] ^= 0x80000000                                                      # a sign flipped
    rejects(fc.check_local, o)
    # a segoff that overlaps: the second segment of a larger group takes the first one's place
    w, gbig = 0, 10                                                                       # SEGN + 1 entries in one bucket: two segments
    s0 = int(fc.segbase[w, gbig])
    o = fc.model_local()
    so = o["segoff"].own.reshape(W, fc.maxseg, F)
    f = F - 1
    assert fc.segcnt[w, s0, f] and fc.segcnt[w, s0 + 1, f]
    so[w, s0 + 1, f] = so[w, s0, f]
    rejects(fc.check_local, o)
    o = fc.model_local()
    o["segcnt"].own.reshape(W, fc.maxseg, F)[w, s0, f] -= 1
    rejects(fc.check_local, o)
    o = fc.model_local()
    o["segcnt"].own.reshape(W, fc.maxseg, F)[w, fc.maxseg - 1, 0] = 0                    # a workgroup past the last segment wrote
    rejects(fc.check_local, o)
    o = fc.model_local()
    o["bsize"].a[-1] = 0                                                                  # a guard word touched
    rejects(fc.check_local, o)
    # k_fine_scatter
    o = fc.model_scatter()
    lo = int(fc.bstart[w, gbig * F + f])
    o["sorted"].own.reshape(W, n)[w, lo] ^= 0x80000000
    rejects(fc.check_scatter, o)
    o = fc.model_scatter()
    o["sorted"].own.reshape(W, n)[1, 0] = 1                                               # a window without MULTI_SEG written
    rejects(fc.check_scatter, o)
    o = fc.model_scatter()
    o["sorted"].own.reshape(W, n)[0, int(fc.gstart[0, 9])] = 1                            # a group of one segment written
    rejects(fc.check_scatter, o)
    g2 = fc.G - 3                                                                         # 2 SEGN entries spread out
    b = g2 * F + 1
    o = fc.model_scatter()
    row = o["sorted"].own.reshape(W, n)[0]
    p, q = int(fc.bstart[0, b]), int(fc.bstart[0, b + 1])
    row[p], row[q] = row[q], row[p]
    rejects(fc.check_scatter, o)


@pytest.mark.parametrize("i", range(len(SC.task_cases())))
def test_task_checkers_accept_the_model(i):
    tc = SC.task_cases()[i]
    tc.check_tables(tc.model_tables())
    tc.check_bases(tc.model_bases())
    tc.check_scatter(tc.model_scatter())
    loc = tc.locate_expected()
    assert len(loc) == tc.ntasks
    if tc.ntasks:                                           # the reference's own tables locate every task where the enumeration put it
        w, b = loc[:, 0], loc[:, 1]
        assert (tc.base[w] + tc.rel[w, b] + loc[:, 2] == np.arange(tc.ntasks)).all() and (tc.ntask[w, b] > loc[:, 2]).all()


def test_task_checkers_reject_mutations():
    tc = SC.task_cases()[0]
    o = tc.model_scatter()
    o["task_id"].own[5] = o["task_id"].own[6]                                            # one task id duplicated
    rejects(tc.check_scatter, o)
    o = tc.model_scatter()
    nt = tc.ntasks
    for k in ("task_bkt", "task_id"):                                                     # two tasks of different length exchanged
        a = o[k].own
        a[0], a[nt - 1] = a[nt - 1], a[0]
    rejects(tc.check_scatter, o)
    o = tc.model_scatter()
    o["task_id"].own[nt] = 0                                                              # written behind the tasks
    rejects(tc.check_scatter, o)
    o = tc.model_scatter()
    o["task_bkt"].own[0], o["task_bkt"].own[1] = o["task_bkt"].own[1], o["task_bkt"].own[0]      # an id that is not its bucket's
    if o["task_bkt"].own[0] != o["task_bkt"].own[1]:
        rejects(tc.check_scatter, o)
    o = tc.model_scatter()
    o["task_id"].a[-1] += 1                                                               # a guard word touched
    rejects(tc.check_scatter, o)
    o = tc.model_tables()
    o["rel"].own[7] += 1
    rejects(tc.check_tables, o)
    o = tc.model_tables()
    assert o["ghist"].own[tc.T] != o["ghist"].own[1]
    o["ghist"].own[tc.T], o["ghist"].own[1] = o["ghist"].own[1], o["ghist"].own[tc.T]      # two bins of the length histogram exchanged
    rejects(tc.check_tables, o)
    hot = [t for t in SC.task_cases() if t.maxv[1] > t.hot_cap][0]
    o = hot.model_tables()
    o["hot_list"].own[1] = o["hot_list"].own[0]                                           # a hot bucket listed twice
    rejects(hot.check_tables, o)
    o = hot.model_tables()
    o["hot_list"].own[0] = int(np.nonzero(~hot.hot.reshape(-1))[0][0])                    # a bucket that is not hot
    rejects(hot.check_tables, o)
    o = hot.model_tables()
    o["maxv"].own[1] = hot.hot_cap                                                        # the count clipped to the cap
    rejects(hot.check_tables, o)
    o = tc.model_bases()
    o["host_info"].own[3] += 1
    rejects(tc.check_bases, o)
    o = tc.model_bases()
    o["cursor"].own[:] = o["cursor"].own[::-1].copy()                                     # ascending instead of descending keys
    rejects(tc.check_bases, o)
