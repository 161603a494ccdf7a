"""tests/reduce_cases.py without a GPU: the layout coders round-trip and agree with the coders the suite already has, the references composed
in the order msm_run.hip launches the kernels give pyoracle's MSM, a census of the case lists (every class of input the kernels branch on is
present, computed from the lists alone), and every checker fed a valid output built by the reference (accepted) and mutated outputs (each
rejected): the evidence that tests/test_gpu_reduce_kernels.py can fail."""
import random

import numpy as np
import pytest

import primitive_cases as PC
import reduce_cases as RC
import sort_cases as SC
from helpers import pt_to_np
from reduce_cases import KEEP, Level, cv


def test_probe_entries_are_listed_for_the_export_test():
    assert set(RC.REDUCE_EXPORTS) <= set(PC.DEV_EXPORTS)


# ---- coders ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_coders_round_trip_and_agree_with_the_existing_ones(name):
    c = cv(name)
    rnd = random.Random(5)
    for m in (0, c.pool[0], c.pool[13], (c.pool[1] + c.pool[2]) % c.n):
        for zi in range(RC.NZ):
            co = c.xyzz(m, zi)
            raw, abi = c.raw(co), c.abi(co)
            assert raw.shape == (c.NW,) and abi.shape == (4 * c.E64,) and (raw < (1 << 29)).all()
            assert all(c.eq(a, b) for a, b in zip(c.unraw(raw), co)) and all(c.eq(a, b) for a, b in zip(c.unabi(abi), co))
            assert c.same_point(c.affine(c.unraw(raw)), c.aff(m))
            # the ABI form of the curve-primitive tests (X | Y | ZZ | ZZZ over a chosen z), and for G2 their 72 raw limbs
            assert np.array_equal(abi, PC.xyzz_np(c.cur, c.aff(m), c.zs[zi]))
            if c.ext:
                assert list(raw) == PC.pt_raw(co)
    # extreme coordinates: 0, 1, p - 1 through both forms
    for v in (0, 1, c.p - 1, rnd.randrange(c.p)):
        co = tuple(c.el([v, c.p - 1 - v]) for _ in range(4))
        assert all(c.eq(a, b) for a, b in zip(c.unraw(c.raw(co)), co)) and all(c.eq(a, b) for a, b in zip(c.unabi(c.abi(co)), co))
    rows = RC.aos(c, [c.pool[i] for i in range(5)], [0, 1, 2, 3, 0])
    flat = RC.to_soa(rows, 7)
    assert flat[3 * 7 + 2] == rows[2, 3] and (flat.reshape(c.NW, 7)[:, 5:] == SC.FILL).all()       # word k of item i at [k * stride + i]
    assert np.array_equal(RC.from_soa(flat, c.NW, 7)[:5], rows)
    if c.ext:                                                                                      # the c0 planes of a coordinate before its c1 planes
        x = c.xyzz(c.pool[0], 0)[0]
        assert PC.val(flat.reshape(c.NW, 7)[0:9, 0]) == x.a * PC.R261 % c.p and PC.val(flat.reshape(c.NW, 7)[9:18, 0]) == x.b * PC.R261 % c.p


# ---- the references, composed as msm_run.hip launches the kernels ------------------------------------------------------------------------------
def compose(c, ks, ms, cw, T, mode):
    """the multiplier of the MSM's sum through acc -> (hot | sum_tasks) -> gather -> halve -> tail -> window values -> windows combined"""
    n = c.n
    dg = SC.Digits(ks, cw)
    W, B = dg.W, 1 << (cw - 1)
    cnt, part = np.zeros((W, B), dtype=np.int64), []
    for w in range(W):
        val, bk, _ = dg.entries(w)
        for b in range(B):
            ent = [int(e) for e in val[bk == b]]
            for lo in range(0, len(ent), T):                                   # the accumulation: one partial sum per task of T entries
                part.append(sum(-ms[e & 0x7FFFFFFF] if e >> 31 else ms[e & 0x7FFFFFFF] for e in ent[lo:lo + T]) % n)
                cnt[w, b] += 1
    L = Level(cnt)
    assert L.total == len(part)
    if mode == "hot":
        hot = [w * B + b for w in range(W) for b in range(B) if cnt[w, b] > RC.GATHER_SUM_MAX][::-1]
        assert hot
        part = RC.ref_hot_fold(part, L, hot, RC.ref_hot_sum(part, L, hot, 16, n), 16, n)
        items, narr, ln = RC.ref_gather_sum(part, L, n), 1, B
    elif mode == "rounds":
        rounds = 0
        while L.cnt.max() > 1:
            L, part = RC.ref_sum_tasks(part, L, 4, n)
            rounds += 1
        assert rounds >= 2
        items, narr, ln = RC.ref_gather_buckets(part, L), 1, B
    else:
        assert cnt.max() <= 1
        items, narr, ln = RC.ref_gather_halve(part, L, n), 2, B // 2
    if mode != "fused":
        items, narr, ln = RC.ref_halve(items, W, narr, ln // 2, n), narr + 1, ln // 2
    slot = RC.ref_tail(items, W, narr, ln, n)
    assert len(slot) == W * cw
    return sum(RC.window_value(slot[w * cw:(w + 1) * cw], n) << (w * cw) for w in range(W)) % n


@pytest.mark.parametrize("name", RC.NAMES)
def test_composed_references_give_the_oracles_msm(name):
    c = cv(name)
    rnd = random.Random(77 + c.id)
    k1 = rnd.randrange(c.n)
    ks = [k1] * 45 + [rnd.randrange(c.n) for _ in range(14)] + [0]                    # one bucket per window with 45 entries: hot at T = 1
    idx = [rnd.randrange(len(c.pool)) for _ in ks]
    ms = [c.pool[i] for i in idx]
    want = sum(k * m for k, m in zip(ks, ms)) % c.n
    assert compose(c, ks, ms, 4, 1, "hot") == want
    assert compose(c, ks, ms, 4, 1, "rounds") == want
    assert compose(c, ks, ms, 4, 64, "fused") == want
    assert c.same_point(c.aff(want), c.cur.msm([c.aff(m) for m in ms], ks))


# ---- census ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_census_gather(name):
    c = cv(name)
    gc = [g for g in RC.gather_cases() if g.c is c]
    assert {g.B for g in gc if g.which == 0} == {2, 64, 512} and all(g.W == 3 and set(np.unique(g.L.cnt)) <= {0, 1} for g in gc if g.which == 0)
    assert all({0, 1} == set(np.unique(g.L.cnt)) for g in gc if g.which == 0)
    fused = [g for g in gc if g.which == 1]
    assert {g.B for g in fused} == {2 * c.TL, 4 * c.TL} and all(g.W == 2 for g in fused)
    for g in fused:
        kinds = g.nodes()
        assert set(kinds) == set(RC.NODE_KINDS), set(RC.NODE_KINDS) - set(kinds)
    sums = [g for g in gc if g.which == 2]
    for g in sums:
        assert set(int(v) for v in g.L.cnt.reshape(-1)) == set(RC.GATHER_SUM_CNTS)
    eq = next(g for g in sums if "equal" in g.name)
    assert any(eq.part[eq.L.first(w, b)] == eq.part[eq.L.first(w, b) + 1] for w in range(3) for b in range(7) if eq.L.cnt[w, b] >= 2)       # the running sum doubles
    al = next(g for g in sums if "alternating" in g.name)
    assert any((al.part[al.L.first(w, b)] + al.part[al.L.first(w, b) + 1]) % c.n == 0 for w in range(3) for b in range(7) if al.L.cnt[w, b] >= 2)
    rn = next(g for g in sums if "random" in g.name)
    hot = [(w, b) for w in range(3) for b in range(7) if rn.L.cnt[w, b] > 32]
    assert hot and any(sum(rn.part[rn.L.first(w, b):rn.L.first(w, b) + int(rn.L.cnt[w, b])]) % c.n != rn.part[rn.L.first(w, b)] for w, b in hot)
    assert all(int(g.L.base[0]) > 0 for g in gc)                           # points in front of the first window's run that no bucket owns


@pytest.mark.parametrize("name", RC.NAMES)
def test_census_sum_tasks_and_halve(name):
    c = cv(name)
    st = [s for s in RC.sum_tasks_cases() if s.c is c]
    assert {s.T2 for s in st} == {2, 16}
    for s in st:
        assert {s.T2 - 1, s.T2, s.T2 + 1, 2 * s.T2, 0} <= set(int(v) for v in s.Lin.cnt.reshape(-1))
        assert s.bound > s.L.total and s.want.count(KEEP) == s.bound - s.L.total
    hc = [h for h in RC.halve_cases() if h.c is c]
    assert {(h.narr, h.n_out) for h in hc} == {(a, o) for a in (1, 2, 3) for o in (1, 2, 64, c.TL)} and all(h.W == 3 for h in hc)
    assert {h.name.split()[-1] for h in hc} == set(RC.PATTERNS)
    seen = set()
    for h in hc:
        kinds = set(h.nodes())
        seen |= kinds
        if h.name.endswith("equal"):
            assert kinds == {"doubling"}
        if h.name.endswith("alternating"):
            assert kinds == {"cancelling"}
    assert seen == set(RC.NODE_KINDS)


@pytest.mark.parametrize("name", RC.NAMES)
def test_census_tails(name):
    c = cv(name)
    tc = [t for t in RC.tail_cases() if t.c is c]
    assert {(t.narr, t.ln) for t in tc if t.form == 0} == {(1, c.TL), (2, c.TL), (3, c.TL)}
    assert {(t.narr, t.ln) for t in tc if t.form == 1} == {(1, ln) for ln in (2, 4, 8, c.TL // 4, c.TL // 2)}
    assert {(t.narr, t.ln) for t in tc if t.form == 2} == {(a, ln) for a in (1, 3) for ln in (2, 4, c.TL // 2, c.TL)}
    for t in tc:
        assert t.W == 3 and len(t.want) == t.W * t.wc and t.wc == t.narr + t.ln.bit_length() - 1       # the slot holds exactly W * c points
    for form in (0, 1, 2):
        kinds = {t.name.split()[-1] for t in tc if t.form == form}
        assert kinds == set(RC.PATTERNS), (form, kinds)
        eq = next(t for t in tc if t.form == form and t.name.endswith("equal") and t.ln >= c.TL // 2)
        assert set(eq.items) == {c.pool[0]} and len(set(eq.zis)) == RC.NZ                                # every level doubles, over different denominators
        al = next(t for t in tc if t.form == form and t.name.endswith("alternating"))
        assert 0 in al.want                                                                             # an identity is exported


@pytest.mark.parametrize("name", RC.NAMES)
def test_census_hot(name):
    c = cv(name)
    hc = RC.hot_cases()
    hc = [h for h in hc if h.c is c]
    for which in (0, 1):
        hs = [h for h in hc if h.which == which]
        shapes = {(h.cnts[0], h.split) for h in hs}
        sm = c.split_max
        assert shapes == {(33, 16), (47, 16), (48, 16), (49, 16), (40, 17), (300, 100), (40, sm), (2 * sm + 1, sm), (16 * c.NT + 16, 16)}
        assert {len(h.cnts) for h in hs} == {1, 3}
        by = {(h.cnts[0], h.split): h for h in hs}
        assert by[(33, 16)].empty_shares() == 5 and by[(48, 16)].empty_shares() == 0 and by[(40, 17)].empty_shares() > 0 and by[(40, sm)].empty_shares() > 0
        big = by[(16 * c.NT + 16, 16)]
        assert (big.cnts[0] + 15) // 16 > c.NT                              # a share longer than the task lanes: the strided loop
        for h in hs:
            assert all(k > RC.GATHER_SUM_MAX for k in h.cnts)
            if len(h.cnts) == 3:
                assert h.hot_list != sorted(h.hot_list) and len({t // h.B for t in h.hot_list}) == 3
            cold = [(w, b) for w in range(h.W) for b in range(h.B) if 0 < h.L.cnt[w, b] <= RC.GATHER_SUM_MAX]
            assert cold and min(h.hot_list) > 0                              # buckets that are not hot hold partial sums around the hot ones
            if which == 0:
                assert h.want.count(KEEP) == h.SLACK and len(h.want) == len(h.cnts) * h.split + h.SLACK
            else:
                assert len(h.want) - h.want.count(KEEP) == len(h.cnts)
        assert any(0 in h.scr for h in hs)                                  # an identity among the shares


# ---- the checkers reject wrong outputs ------------------------------------------------------------------------------------------------------
def _small(cases, per=2):
    """the first `per` cases of every (class, curve, kernel form) whose outputs stay small: enough for every mutation, quick on any machine"""
    out, seen = [], {}
    for x in cases:
        key = (type(x).__name__, x.c.name, getattr(x, "which", getattr(x, "form", 0)))
        if len(x.expected()[next(iter(x.expected()))][0]) <= 1100 and seen.get(key, 0) < per:
            seen[key] = seen.get(key, 0) + 1
            out.append(x)
    return out


ALL = _small([a for a in RC.acc_cases() if a.nsets == 1] + RC.gather_cases() + RC.sum_tasks_cases() + RC.halve_cases() + RC.tail_cases() + RC.hot_cases())


def _rejected(case, out, what):
    with pytest.raises(AssertionError):
        case.check(out)
        print(f"{case.name}: accepted an output with {what}")


@pytest.mark.parametrize("case", ALL, ids=[x.name for x in ALL])
def test_checker_accepts_the_model_and_rejects_mutations(case):
    c = case.c
    case.check(case.model())
    (k, (want, rows, decode, before)), = case.expected().items()
    live = [i for i, m in enumerate(want) if m is not KEEP]
    # a guard word changed
    out = case.model()
    out[k].a[out[k].words + 3] ^= 1
    _rejected(case, out, "a guard word changed")
    # two slots with different contents swapped
    pair = next(((i, j) for i in live for j in live if i < j and want[i] % c.n != want[j] % c.n), None)
    assert pair is not None or len({want[i] % c.n for i in live}) == 1
    if pair:
        out = case.model()
        r = rows(out[k].own)
        a, b = r[pair[0]].copy(), r[pair[1]].copy()
        r[pair[0]], r[pair[1]] = b, a
        _rejected(case, out, "two slots swapped")
    # a sum that misses one item: the slot holds (expected - P)
    out = case.model()
    r = rows(out[k].own)
    m = (want[live[-1]] - c.pool[0]) % c.n
    r[live[-1]] = c.abi(c.xyzz(m, 1)) if decode is not None else c.enc(m, 1 if m else 0)
    _rejected(case, out, "a sum that misses one item")
    # a point whose zz and zzz do not belong together
    i = next((i for i in live if want[i] % c.n), None)
    if i is not None:
        out = case.model()
        r = rows(out[k].own)
        good = r[i].copy()
        third = len(good) // 4
        good[3 * third:] = r[i][2 * third:3 * third]                       # zzz := zz
        r[i] = good
        with pytest.raises(AssertionError, match="zz\\^3"):
            case.check(out)
    # a slot that was not written
    out = case.model()
    rows(out[k].own)[live[0]] = SC.FILL if before is None else before[live[0]]
    if before is None or want[live[0]] % c.n != case.part[live[0]] % c.n:                  # (in place: the input may already be the total)
        _rejected(case, out, "a slot left unwritten")
    # a word that must stay as it was overwritten
    keep = [i for i, m in enumerate(want) if m is KEEP]
    if keep:
        out = case.model()
        rows(out[k].own)[keep[0]][5] ^= 0x10
        _rejected(case, out, "a must-stay word overwritten")
        out = case.model()
        rows(out[k].own)[keep[-1]] = rows(out[k].own)[live[0]]
        _rejected(case, out, "a point written into a slot that must stay")


def test_mutations_cover_every_kernel_and_the_must_stay_slots():
    kinds = {(type(x).__name__, getattr(x, "which", getattr(x, "form", 0))) for x in ALL}
    assert kinds == {("AccCase", 0), ("GatherCase", 0), ("GatherCase", 1), ("GatherCase", 2), ("SumTasksCase", 0), ("HalveCase", 0), ("TailCase", 0), ("TailCase", 1),
                     ("TailCase", 2), ("HotCase", 0), ("HotCase", 1)}
    assert any(KEEP in x.expected()[next(iter(x.expected()))][0] for x in ALL if isinstance(x, RC.SumTasksCase))
    assert any(KEEP in x.expected()[next(iter(x.expected()))][0] for x in ALL if isinstance(x, RC.HotCase) and x.which == 1)


@pytest.mark.parametrize("name", RC.NAMES)
def test_fused_checker_rejects_a_partial_sum_in_the_other_sets_buffer(name):
    for case in (a for a in RC.acc_cases() if a.c.name == name and a.nsets > 1 and a.order == 0):
        case.check(case.model())
        ks = list(case.expected())
        out = case.model()                                                  # whole buffers exchanged
        out[ks[0]], out[ks[1]] = out[ks[1]], out[ks[0]]
        _rejected(case, out, "the sets' buffers exchanged")
        t = next(t for t in range(case.tc.ntasks) if case.want[0][t] % case.c.n != case.want[1][t] % case.c.n)
        out = case.model()                                                  # one task's sum of set 0 written into set 1's slot as well
        r0, r1 = out[ks[0]].own.reshape(-1, case.c.NW), out[ks[1]].own.reshape(-1, case.c.NW)
        r1[t] = r0[t]
        _rejected(case, out, "a partial sum in the other set's buffer")
        out = case.model()                                                  # a slot behind ntasks written
        out[ks[-1]].own.reshape(-1, case.c.NW)[case.tc.ntasks] = r0[0]
        _rejected(case, out, "a slot behind ntasks written")


@pytest.mark.parametrize("case", [x for x in RC.prep_cases() + RC.table_cases() if x.n <= 65], ids=lambda x: x.name)
def test_word_checkers_reject_mutations(case):
    case.check(case.model())
    for at, what in ((0, "the first word"), (len(case.want) - 1, "the last word"), (7 if case.fmt else 8, "the word of the flag")):
        out = case.model()
        out["out"].own[at] ^= 0x80000000 if "flag" in what else 1
        _rejected(case, out, what + " changed")
    out = case.model()
    out["out"].a[out["out"].words] ^= 1
    _rejected(case, out, "a guard word changed")


# ---- bases and accumulation: coders and census ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_resident_packers_round_trip(name):
    c = cv(name)
    rnd = random.Random(9)
    for w in [0, 1, c.p - 1] + [rnd.randrange(c.p) for _ in range(40)]:
        v = RC.from_ref_val(c.p, w)
        assert v < 2 * c.p and (v - 32 * w) % c.p == 0                      # x * 2^256 -> x * 2^261, below 2p
    for m in c.pool[:4]:
        for fmt in (RC.BASES_72, RC.BASES_64):
            for inf in (False, True):
                vals = RC.internal_vals(c, c.aff(m))
                w = RC.pack_resident(vals, inf, fmt)
                assert len(w) == RC.resident_words(c, fmt) and RC.unpack_resident(c, w, fmt) == (vals, inf)
                assert bool(w[7 if fmt else 8] & RC.INF_BIT) == inf and (fmt or not any(int(x) & RC.INF_BIT for i, x in enumerate(w) if i != 8))
                pt = c.aff(m)
                assert all((v - x * PC.R261) % c.p == 0 for v, x in zip(vals, [v for e in pt for v in c.comps(e)]))
    assert RC.resident_words(c, RC.BASES_72) == 18 * c.NE and RC.resident_words(c, RC.BASES_64) == 16 * c.NE
    assert np.array_equal(RC.abi_point(c, c.aff(c.pool[0])), pt_to_np(c.cur, c.aff(c.pool[0])))       # the ABI form of the parity tests


@pytest.mark.parametrize("name", RC.NAMES)
def test_census_bases(name):
    c = cv(name)
    pc = [x for x in RC.prep_cases() if x.c is c]
    assert {x.n for x in pc} == {1, 255, 256, 257} and {x.fmt for x in pc} == {0, 1}
    assert {(x.fmt, x.inf is None) for x in pc} == {(0, True), (0, False), (1, True), (1, False)}
    big = next(x for x in pc if x.n == 257 and x.inf is not None)
    comps = {v for pt in big.pts for e in pt for v in c.comps(e)}
    assert {0, 1, c.p - 1} <= comps and big.inf[0] and big.inf[-1] and big.inf[128] and not big.inf[1]
    if not c.ext:
        import acc_abi_cases
        assert all(pt in big.pts for _, pt in acc_abi_cases.special_points(name))
    tc = [x for x in RC.table_cases() if x.c is c]
    assert {(x.cw, x.n) for x in tc} == {(cw, n) for cw in (1, 2, 13) for n in (1, 63, 64, 65)}
    for fmt in (0, 1):
        assert {x.cw for x in tc if x.fmt == fmt} == {1, 2, 13} and {x.n for x in tc if x.fmt == fmt} == {1, 63, 64, 65}
    assert all(any(x.inf) and not all(x.inf) for x in tc if x.n > 1)


@pytest.mark.parametrize("name", RC.NAMES)
def test_census_acc(name):
    c = cv(name)
    ac = [a for a in RC.acc_cases() if a.c is c]
    fm = {0, 1} if c.ext else {0, 1, 2}
    assert {a.tc.ntasks for a in ac if not a.merged} == {1, 63, 64, 65, 130}
    assert {a.fmts[0] for a in ac if a.nsets == 1 and not a.merged} == fm and {f for a in ac if a.nsets > 1 for f in a.fmts} == fm
    assert {a.nsets for a in ac} == {1, 2, 3} and {a.fmts[0] for a in ac if a.merged} == {0, 1} and all(a.tc.Wg == 1 and a.mshift > 0 for a in ac if a.merged)
    for order in (0, 1):
        sel = [a for a in ac if a.order == order]
        tot = lambda key: sum(a.stats[key] for a in sel)
        assert tot("doubling") and tot("identity mid-chain")
        for pos in ("first", "middle", "last"):
            assert sum(a.stats["flagged"][pos] for a in sel)
        fused = [a for a in sel if a.nsets > 1]
        assert all(a.stats["skipped"][0] == 0 and all(v > 0 for v in a.stats["skipped"][1:]) for a in fused)
        assert any(v > 0 for a in fused for v in a.stats["all skipped"][1:])                  # a task with nothing left in a set: the identity
        assert set(RC.CHAINS) <= {k for a in sel for k in a.chain_of.values()}
    for a in ac:
        tc = a.tc
        nt = tc.ntasks
        assert sorted(a.task_id) == list(range(nt)) and a.idx_off == sorted(a.idx_off) and a.idx_off[0] == 0
        first = tc.base[a.task_bkt // tc.B] + tc.rel.reshape(-1)[a.task_bkt]
        seg = a.task_id - first
        cnt = tc.ntask.reshape(-1)[a.task_bkt]
        assert ((seg >= 0) & (seg < cnt)).all()
        ln = np.where(seg < cnt - 1, tc.Tb.reshape(-1)[a.task_bkt], tc.rem.reshape(-1)[a.task_bkt])
        key = SC.len_key(ln)
        assert (key[1:] <= key[:-1]).all()                                   # check_scatter's rules: the keys of the lengths never rise
    a0, a1 = (next(a for a in ac if a.tc.ntasks == 65 and a.nsets == 1 and a.order == o) for o in (0, 1))
    assert not np.array_equal(a0.task_id, a1.task_id)
    t65, t130 = RC.acc_task_tables()[65], RC.acc_task_tables()[130]
    assert ((t65.ntask > 1) & (t65.rem == 1)).any() and t65.top_w == 2 and t65.ntask[2].max() == 3 and t65.bsize[2].max() == 4 * RC.ACC_T + 1
    assert t130.hot.any() and t130.Tb[t130.hot][0] == RC.ACC_T >> 2 and t130.ntask.max() == 129
