"""kg_groth16_witness_check_batch on the device -- R1cs::is_sat for many witnesses x_b || w_b of one circuit, read in place from the arrays
kg_groth16_prove_r1cs_batch takes -- and the api.py entries over both batched checks: Prover.check_witnesses,
Prover.create_proofs_batch_from_witness(check=True), NovaProver.check_batch.  Every status byte and summary word must equal what Python
integers give on the oracle's row sums and what kg_r1cs_check gives on the concatenated z."""
import numpy as np
import pytest

import r1cs_cases as RC
import r1cs_check_batch_cases as BC
from test_gpu_groth16_batch import SEED, assert_same, random_jobs
from test_gpu_groth16_r1cs_batch import chain_prover

pytestmark = pytest.mark.gpu
P = RC.MODULI[0]


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def upload_mats(ctx, mats):
    dev = [tuple(ctx.upload(np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], dtype=np.uint64))) for a in t) for t in mats]
    return dev, [tuple(d.ptr for d in t) for t in dev]


def want_plain(O, mats, m, z):
    """(status, bad, first) of the plain relation from Python integers on the oracle's row sums"""
    az, bz, cz = (RC.to_ints(O.matrix_prod(0, t, z), P) if len(z) else [0] * m for t in mats)
    st = np.array([RC.KG_ROW_UNSAT if (a * b - c) % P else 0 for a, b, c in zip(az, bz, cz)], dtype=np.uint8)
    bad = np.flatnonzero(st)
    return st, len(bad), int(bad[0]) if len(bad) else m


def check_split(ctx, O, mats, ptrs, m, l, m_l_1, witnesses, extra=(2, 3, 4)):
    """the split form on (x, w) pairs packed with gaps of non-canonical words, into guarded outputs; against Python integers and against
    kg_r1cs_check on the concatenated z"""
    count = len(witnesses)
    xs, ws, ss = l + extra[0], m_l_1 + extra[1], m + extra[2]
    rng = np.random.default_rng(7)
    x = rng.integers(0, 1 << 63, (count, xs, 4), dtype=np.uint64) | np.uint64(1 << 63)
    w = rng.integers(0, 1 << 63, (count, max(ws, 1), 4), dtype=np.uint64) | np.uint64(1 << 63)
    for b, (xb, wb) in enumerate(witnesses):
        x[b, :l], w[b, :m_l_1] = xb, wb
    dx, dw = ctx.upload(x), ctx.upload(w)
    d_status = ctx.upload(np.full(count * ss + 16, BC.GUARD8, dtype=np.uint8))
    d_sum = ctx.upload(np.full((count + 2, 2), BC.GUARD32, dtype=np.uint32))
    ctx.groth16_witness_check_batch(*ptrs, m, l, m_l_1, dx.ptr, xs, dw.ptr if m_l_1 else 0, ws, count, d_status.ptr, ss, summary=d_sum)
    st, sums = d_status.numpy(), d_sum.numpy()
    assert (sums[count:] == BC.GUARD32).all() and (st[count * ss:] == BC.GUARD8).all()
    rows = st[:count * ss].reshape(count, ss)
    assert (rows[:, m:] == BC.GUARD8).all()
    assert dx.numpy().tobytes() == x.tobytes() and dw.numpy().tobytes() == w.tobytes()
    no_status = ctx.groth16_witness_check_batch(*ptrs, m, l, m_l_1, dx.ptr, xs, dw.ptr if m_l_1 else 0, ws, count).numpy()       # d_status NULL
    assert no_status.shape == (count, 2) and (no_status == sums[:count]).all()
    wants = []
    for b, (xb, wb) in enumerate(witnesses):
        z = np.ascontiguousarray(np.concatenate([np.asarray(xb).reshape(-1, 4), np.asarray(wb).reshape(-1, 4)]))
        want = want_plain(O, mats, m, z)
        assert tuple(int(v) for v in sums[b]) == want[1:], (m, b, sums[b], want[1:])
        assert (rows[b, :m] == want[0]).all(), (m, b, np.flatnonzero(rows[b, :m] != want[0])[:8])
        one = ctx.upload(np.full(m, 0xAA, dtype=np.uint8))
        assert ctx.r1cs_check(0, *ptrs, m, ctx.upload(z).ptr, status=one.ptr) == want[1:] and (one.numpy() == want[0]).all(), (m, b, "kg_r1cs_check")
        wants.append(want)
    return wants


def chain_witnesses(O, m, seed):
    """7 witnesses of the m-constraint chain: valid; one entry of w changed; x[0] != 1; the last w entry changed; all zero; two more valid"""
    t0 = O.gen_scalars(0, seed, 0, 4)
    css = [O.chain_r1cs(m, t0[k]) for k in range(3)]
    valid = [(cs.x.copy(), cs.w.copy()) for cs in css]
    x, w = valid[0]
    bump = lambda e: RC.to_mont([RC.to_ints(e.reshape(1, 4), P)[0] + 1], P)[0]
    w_mid, w_last, x_one = w.copy(), w.copy(), x.copy()
    w_mid[(m - 1) // 2] = bump(w[(m - 1) // 2])
    w_last[m - 1] = bump(w[m - 1])
    x_one[0] = bump(x[0])
    return css[0], [valid[0], (x, w_mid), (x_one, w), (x, w_last), (np.zeros_like(x), np.zeros_like(w)), valid[1], valid[2]]


@pytest.mark.parametrize("m", [1, 5, 100, 2046, 2047])
def test_chain_witnesses_read_in_place(ctx, oracle, m):
    """2046: the longest circuit the batched prover takes; 2047: one more -- the check needs no CRS and is not bound to that limit"""
    cs, wit = chain_witnesses(oracle, m, SEED + 4800 + m)
    mats = (cs.a, cs.b, cs.c)
    dev, ptrs = upload_mats(ctx, mats)
    wants = check_split(ctx, oracle, mats, ptrs, m, cs.l, cs.m_l_1, wit)
    assert [w[1] for w in wants][0::4] == [0, 0] and wants[5][1:] == (0, m) == wants[6][1:]     # the valid ones and the all-zero one hold
    assert wants[1][1] >= 1 and wants[1][2] == (m - 1) // 2                                     # the constraint that produces the changed wire
    assert wants[2][1] >= 1 and wants[3][1:] == (1, m - 1)


def test_circuit_with_long_rows(ctx, oracle):
    """the m = 300 shape of tests/r1cs_cases.py over Fr as the circuit tests/test_gpu_groth16_r1cs_batch.py uses (l = 4): rows of 49 .. 5000
    entries go through the work list and the wave kernel with the split source; the six z vectors of the batched check's case, cut at l"""
    sh, vecs = BC.case300(oracle, 0)
    dev, ptrs = upload_mats(ctx, sh.mats)
    wants = check_split(ctx, oracle, sh.mats, ptrs, sh.m, 4, sh.nvars - 4, [(v.z[:4], v.z[4:]) for v in vecs])
    for v, want in zip(vecs, wants):
        st, bad, first = v.want(sh, plain=True)
        assert want[1:] == (bad, first) and (want[0] == st).all()
    assert len({w[1:] for w in wants}) == len(wants)


def test_one_instance_wire_and_no_witness_wire(ctx, oracle):
    """l = 1, m_l_1 = 0: z = x, d_w NULL.  Row 0: z0 * z0 = z0; row 1: z0 * z0 = 0."""
    one = oracle.f_consts(0)["r"]
    e1 = (np.array([0, 1, 2], dtype=np.uint64), np.array([0, 0], dtype=np.uint64), np.stack([one, one]))
    c = (np.array([0, 1, 1], dtype=np.uint64), np.array([0], dtype=np.uint64), np.stack([one]))
    mats = (e1, e1, c)
    dev, ptrs = upload_mats(ctx, mats)
    empty = np.zeros((0, 4), dtype=np.uint64)
    wants = check_split(ctx, oracle, mats, ptrs, 2, 1, 0, [(RC.to_mont([v], P), empty) for v in (1, 2, 0)], extra=(0, 0, 0))
    assert [w[1:] for w in wants] == [(1, 1), (2, 0), (0, 2)]
    check_split(ctx, oracle, mats, ptrs, 2, 1, 0, [(RC.to_mont([v], P), empty) for v in (1, 2, 0)], extra=(3, 0, 1))


def test_prover_entries(ctx, oracle):
    """Prover.check_witnesses against check_witness; create_proofs_batch_from_witness(check=True): the proofs of check=False bit for bit, the
    summary flags exactly the invalid witnesses"""
    O, m = oracle, 5
    _, prover = chain_prover(O, ctx, m)
    jobs = [list(j[3:]) for _, j in random_jobs(O, m, 5, SEED + 4900)]
    jobs[1][1] = jobs[1][1].copy()
    jobs[1][1][2] = jobs[0][1][2]                                                  # witness 1: w[2] from another assignment
    jobs[3][0] = jobs[3][0].copy()
    jobs[3][0][1] = jobs[0][0][1]                                                  # witness 3: t_0 from another assignment
    singles = [prover.check_witness(j[0], j[1]) for j in jobs]
    assert [s[0] > 0 for s in singles] == [False, True, False, True, False] and singles[1][1] == 2 and singles[3][1] == 0
    got = prover.check_witnesses(jobs)
    assert got.shape == (5, 2) and got.dtype == np.uint32 and [tuple(int(v) for v in r) for r in got] == singles
    assert prover.check_witnesses([]).shape == (0, 2)
    plain = prover.create_proofs_batch_from_witness(jobs)
    checked = prover.create_proofs_batch_from_witness(jobs, check=True)
    assert len(plain) == 2 and len(checked) == 3
    for b in range(5):
        assert_same((checked[0][b], checked[1][b]), (plain[0][b], plain[1][b]), ("check=True", b))
    assert checked[0].tobytes() == plain[0].tobytes() and checked[1].tobytes() == plain[1].tobytes()
    assert [tuple(int(v) for v in r) for r in checked[2]] == singles
    out = prover.create_proofs_batch_from_witness([], check=True)
    assert out[0].shape == (0, 32) and out[1].shape == (0, 3) and out[2].shape == (0, 2)


@pytest.mark.parametrize("fd", [0, 1])
def test_nova_check_batch(ctx, oracle, fd):
    """NovaProver.check_batch over both scalar fields: z = (u | x | w), a u and an E per pair; row b is what NovaProver.check gives"""
    import kogarashi_amd as K
    O = oracle
    sh, vecs = BC.case300(O, fd)
    ck = K.PedersenCommitment(O.gen_bases(fd, SEED + 4950 + fd, 0, 8), curve=fd, ctx=ctx)
    prover = K.NovaProver(sh.mats, ck, ctx=ctx)
    assert prover.field == fd
    pairs, wants = [], []
    rows = [[], RC.perturbed_rows(sh.m), [RC.LONG_ROW], [RC.HUGE_ROW, sh.m - 1]]
    for v, sub in zip(vecs[:4], rows):
        z = v.z.copy()
        z[0] = v.u
        prods = sh.row_sums(z)
        e = RC.perturb(sh, RC.satisfying_e(sh, v.ui, prods), sub)
        pairs.append((v.u, z[1:4], z[4:], RC.to_mont(e, sh.p)))
        wants.append(RC.expected(sh, v.ui, e, prods)[1:])
    assert wants == [(0, sh.m), (len(rows[1]), 0), (1, RC.LONG_ROW), (2, RC.HUGE_ROW)]
    got = prover.check_batch(pairs)
    assert got.shape == (4, 2) and [tuple(int(x) for x in r) for r in got] == wants
    assert [prover.check(*p) for p in pairs] == wants
    # no E anywhere: d_e NULL
    plain = prover.check_batch([(u, x, w, None) for u, x, w, _ in pairs])
    assert [tuple(int(x) for x in r) for r in plain] == [prover.check(u, x, w) for u, x, w, _ in pairs]
    assert prover.check_batch([]).shape == (0, 2)
