"""kg_r1cs_check on the device: (A z)_i (B z)_i = u (C z)_i + E_i row by row, plain (R1cs::is_sat, zkstd/src/r1cs.rs:62-77) and relaxed
(is_sat_relaxed, nova/src/relaxed_r1cs.rs:81-114), over both scalar fields.  Every status byte, the count and the first index must equal what
Python integers give on the oracle's row sums (tests/r1cs_cases.py); nothing here has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import r1cs_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = RC.SEED
SIZES = [1, 5, 63, 64, 65, 255, 256, 257, 1000, 20000]     # wave and workgroup edges; from 13 rows the long rows appear, from 101 the 254- and 5000-entry rows


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


class Resident:
    """a shape of tests/r1cs_cases.py with its matrices on the device"""

    def __init__(self, ctx, sh):
        self.ctx, self.sh = ctx, sh
        self.dev = [tuple(ctx.upload(np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], dtype=np.uint64))) for a in t) for t in sh.mats]
        self.ptrs = [tuple(d.ptr for d in t) for t in self.dev]
        self.status = None

    def raw(self, z, u, e, status, want_bad=True, want_first=True):
        """the entry itself, so that each out-pointer can be NULL"""
        from kogarashi_amd import lib as L
        ca, cb, cc = (L.Csr(*p) for p in self.ptrs)
        hu = np.ascontiguousarray(u, dtype=np.uint64).ctypes.data_as(C.c_void_p) if u is not None else None
        bad, first = C.c_size_t(1 << 40), C.c_size_t(1 << 40)
        rc = self.ctx._lib.kg_r1cs_check(self.ctx._h, self.sh.fd, C.byref(ca), C.byref(cb), C.byref(cc), C.c_size_t(self.sh.m), C.c_void_p(z), hu,
                                         C.c_void_p(e) if e else None, C.c_void_p(status) if status else None,
                                         C.byref(bad) if want_bad else None, C.byref(first) if want_first else None)
        assert rc == 0, rc
        return bad.value, first.value

    def assert_matches(self, z, u, e, want, nulls=False):
        """status bytes, count and first index against `want`; with nulls=True also with d_status, out_bad and out_first_bad NULL in turn"""
        st, bad, first = want
        c, m = self.ctx, self.sh.m
        dz = z if hasattr(z, "ptr") else c.upload(z)
        de = c.upload(e) if e is not None else None
        ep = de.ptr if de is not None else 0
        self.status = c.upload(np.full(m, 0xAA, dtype=np.uint8))        # every byte must be written, the zeros too
        got = c.r1cs_check(self.sh.fd, *self.ptrs, m, dz.ptr, u, ep, self.status.ptr)
        g = self.status.numpy()
        assert (g == st).all(), (self.sh.fd, m, np.flatnonzero(g != st)[:8], g[g != st][:8])
        assert got == (bad, first), (self.sh.fd, m, got, (bad, first))
        if nulls:
            assert c.r1cs_check(self.sh.fd, *self.ptrs, m, dz.ptr, u, ep, 0) == (bad, first)
            assert self.raw(dz.ptr, u, ep, 0, want_bad=False) == (1 << 40, first)
            assert self.raw(dz.ptr, u, ep, self.status.ptr, want_first=False) == (bad, 1 << 40)
            assert self.raw(dz.ptr, u, ep, 0, want_bad=False, want_first=False) == (1 << 40, 1 << 40)
            assert (self.status.numpy() == st).all()


@pytest.fixture(scope="module")
def resident(ctx, oracle):
    cache = {}

    def get(fd, m):
        if (fd, m) not in cache:
            cache[(fd, m)] = Resident(ctx, RC.Shape(oracle, fd, m))
        return cache[(fd, m)]
    return get


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("m", SIZES)
def test_status_count_and_first_index(oracle, resident, fd, m):
    R = resident(fd, m)
    sh = R.sh
    dz = R.ctx.upload(sh.z)
    rows = RC.perturbed_rows(m)
    for name, u, ui in RC.u_values(oracle, fd):
        e = RC.satisfying_e(sh, ui)
        want = RC.expected(sh, ui, e)
        assert want[1:] == (0, m) and not want[0].any()
        R.assert_matches(dz, u, RC.to_mont(e, sh.p), want)                                      # every row holds
        pe = RC.perturb(sh, e, rows)
        want = RC.expected(sh, ui, pe)
        assert np.flatnonzero(want[0]).tolist() == rows
        R.assert_matches(dz, u, RC.to_mont(pe, sh.p), want, nulls=name in ("null", "random"))
    # the first index across the two kernels: a work-list row first with ordinary rows after it, an ordinary row first with work-list rows
    # after it, one row alone (a wave's last lane, the next wave's first, the 5000-entry row)
    name, u, ui = RC.u_values(oracle, fd)[-1]
    e = RC.satisfying_e(sh, ui)
    subsets = [[RC.LONG_ROW, RC.LONG_ROW + 3, m - 1], [RC.LONG_ROW + 3, 20, RC.HUGE_ROW, m - 1], [RC.EDGE49, RC.EDGE48], [RC.HUGE_ROW], [63], [64], [m - 1]]
    for sub in subsets:
        sub = sorted({r for r in sub if 0 <= r < m})
        if not sub:
            continue
        pe = RC.perturb(sh, e, sub)
        want = RC.expected(sh, ui, pe)
        assert (want[1], want[2]) == (len(sub), sub[0])
        R.assert_matches(dz, u, RC.to_mont(pe, sh.p), want)
    # the plain relation (no u, no E) on random data: nearly every row fails, the rows that are empty in every matrix hold
    want = RC.expected(sh, 1, None)
    assert not want[0][RC.EMPTY_A % m] and (m < 63 or want[1] > m // 2)
    R.assert_matches(dz, None, None, want, nulls=True)
    # one z entry changed under an E made for the old z: the long row and the short rows that read it fail
    if m > 12:
        z2, prods2 = sh.flip_z()
        want = RC.expected(sh, ui, e, prods2)
        assert want[0][RC.LONG_ROW] and want[0][RC.FLIP_SHORT_B] and want[0][RC.FLIP_SHORT_C] and 3 <= want[1] < m
        R.assert_matches(z2, u, RC.to_mont(e, sh.p), want)


@pytest.mark.parametrize("fd", [0, 1])
def test_summary_and_work_list_are_rebuilt_per_call(oracle, resident, fd):
    """two calls in a row on one context with different answers, a kg_r1cs_prod (same work space: its own work lists, the huge-row list too)
    between them, then the first answer again"""
    R = resident(fd, 1000)
    sh, c = R.sh, R.ctx
    dz = c.upload(sh.z)
    name, u, ui = RC.u_values(oracle, fd)[-1]
    e = RC.satisfying_e(sh, ui)
    pe = RC.perturb(sh, e, RC.perturbed_rows(sh.m))
    bad_case, good_case = (RC.to_mont(pe, sh.p), RC.expected(sh, ui, pe)), (RC.to_mont(e, sh.p), RC.expected(sh, ui, e))
    R.assert_matches(dz, u, *bad_case)
    R.assert_matches(dz, u, *good_case)
    out = c.empty((sh.m, 4))
    c.r1cs_prod(fd, *R.ptrs[1], sh.m, dz.ptr, out.ptr)
    assert (out.numpy() == oracle.matrix_prod(fd, sh.mats[1], sh.z)).all()
    R.assert_matches(dz, u, *bad_case)
    c.r1cs_prod(fd, *R.ptrs[1], sh.m, dz.ptr, out.ptr)
    R.assert_matches(dz, u, *good_case)


def test_argument_checks_and_empty_input(ctx, resident):
    from kogarashi_amd.lib import KogarashiError
    R = resident(0, 5)
    dz = ctx.upload(R.sh.z)
    assert ctx.r1cs_check(0, *R.ptrs, 0, dz.ptr) == (0, 0)                          # m = 0: nothing read, 0 / 0
    assert ctx.r1cs_check(0, *R.ptrs, 0, 0) == (0, 0)
    for args in ((0, *R.ptrs, 5, 0), (7, *R.ptrs, 5, dz.ptr), (0, (0, 0, 0), R.ptrs[1], R.ptrs[2], 5, dz.ptr), (0, *R.ptrs, 1 << 32, dz.ptr)):
        with pytest.raises(KogarashiError):
            ctx.r1cs_check(*args)
    assert ctx.r1cs_check(0, *R.ptrs, 5, dz.ptr)[0] > 0                             # and the context keeps working


def test_plain_relation_on_the_chain_circuit(ctx, oracle):
    """h_u = NULL, d_e = NULL is R1cs::is_sat: the chain circuit's own assignment holds; one witness entry changed breaks exactly the constraint
    that produces it and the one that consumes it"""
    O = oracle
    cs = O.chain_r1cs(512, O.gen_scalars(0, SEED + 4200, 0, 1)[0])
    dev = [tuple(ctx.upload(np.ascontiguousarray(a)) for a in t) for t in (cs.a, cs.b, cs.c)]
    ptrs = [tuple(d.ptr for d in t) for t in dev]
    z = np.concatenate([cs.x, cs.w])
    st = ctx.empty((cs.m,), dtype=np.uint8)
    assert ctx.r1cs_check(0, *ptrs, cs.m, ctx.upload(z).ptr, status=st.ptr) == (0, cs.m) and not st.numpy().any()
    p = RC.MODULI[0]
    z2 = z.copy()
    z2[2 + 100] = RC.to_mont([RC.to_ints(z[102:103], p)[0] + 5], p)[0]              # t_101: C of constraint 100, A and B of constraint 101
    az, bz, cz = (RC.to_ints(O.matrix_prod(0, t, z2), p) for t in (cs.a, cs.b, cs.c))
    want = np.array([1 if (a * b - c) % p else 0 for a, b, c in zip(az, bz, cz)], dtype=np.uint8)
    assert np.flatnonzero(want).tolist() == [100, 101]
    assert ctx.r1cs_check(0, *ptrs, cs.m, ctx.upload(z2).ptr, status=st.ptr) == (2, 100) and (st.numpy() == want).all()


def test_folded_pair_is_sat_relaxed(ctx, oracle):
    """after NovaProver.prove on two satisfied chain instances the folded pair satisfies the relaxed relation; one E entry changed and it does
    not, first_bad at that row; is_sat on a fresh pair, and with another commit_w (the constraints still hold: check reports no bad row); the
    check sees device-side folds enqueued just before it without a synchronisation in between"""
    import kogarashi_amd as K
    O, fd, m = oracle, 0, 300
    css = [O.chain_r1cs(m, O.gen_scalars(0, SEED + 4300 + j, 0, 1)[0]) for j in range(2)]
    one = O.f_consts(0)["r"]
    g = O.gen_bases(0, SEED + 4310, 0, m + 1)
    ck = K.PedersenCommitment(g, curve=0, ctx=ctx)
    prover = K.NovaProver((css[0].a, css[0].b, css[0].c), ck, ctx=ctx)
    xs, ws = [cs.x[1:] for cs in css], [cs.w for cs in css]             # chain_r1cs columns are (x | w) with x[0] = 1 = the one-wire u
    fresh = [({"commit_w": ck.commit(ws[j]), "x": xs[j]}, {"w": ws[j]}) for j in range(2)]
    for inst, wit in fresh:
        assert prover.is_sat(inst, wit)
        assert prover.check(one, inst["x"], wit["w"]) == (0, m)
    other = dict(fresh[0][0], commit_w=fresh[1][0]["commit_w"])
    assert not prover.is_sat(other, fresh[0][1]) and prover.check(one, other["x"], fresh[0][1]["w"]) == (0, m)
    broken = {"w": ws[0].copy()}
    broken["w"][17] = ws[1][17]
    assert not prover.is_sat(dict(fresh[0][0], commit_w=ck.commit(broken["w"])), broken)
    i1 = dict(fresh[0][0], commit_e=(np.zeros(8, dtype=np.uint64), 1), u=one)
    w1 = {"w": ws[0], "e": np.zeros((m, 4), dtype=np.uint64)}
    r = O.gen_scalars(0, SEED + 4320, 0, 1)[0]
    inst, wit, _ = prover.prove(i1, w1, fresh[1][0], fresh[1][1], r)
    assert prover.is_sat_relaxed(i1, w1) and prover.is_sat_relaxed(inst, wit)
    assert wit["e"].any() and (inst["u"] != one).any()                  # a relaxed pair in earnest
    assert not prover.is_sat(inst, wit)                                 # and no longer a plain one
    bad = {"w": wit["w"], "e": wit["e"].copy()}
    bad["e"][211, 0] ^= np.uint64(1)
    assert not prover.is_sat_relaxed(inst, bad)
    assert prover.check(inst["u"], inst["x"], bad["w"], bad["e"]) == (1, 211)
    # the same fold with device ops only, the check right behind them on the stream
    t = prover.compute_cross_term_device(one, xs[0], ws[0], one, xs[1], ws[1])
    z1, z2 = np.concatenate([css[0].x, css[0].w]), np.concatenate([css[1].x, css[1].w])
    dz1, dz2, de = ctx.upload(z1), ctx.upload(z2), ctx.upload(np.zeros((m, 4), dtype=np.uint64))
    ptrs = [tuple(d.ptr for d in trip) for trip in prover._dev]
    ctx.field_vec_axpy(fd, dz1.ptr, r, dz2.ptr, dz1.ptr, len(z1))                   # z = z1 + r z2: its first entry becomes u = 1 + r
    ctx.field_vec_axpy(fd, de.ptr, r, t.ptr, de.ptr, m)                             # E = 0 + r T
    assert ctx.r1cs_check(fd, *ptrs, m, dz1.ptr, O.f_add(0, one, r), de.ptr) == (0, m)
    ctx.field_vec_axpy(fd, de.ptr, r, t.ptr, de.ptr, m)                             # E = 2 r T: wrong wherever T != 0
    tz = RC.to_ints(t.numpy(), RC.MODULI[0])
    nz = [i for i, v in enumerate(tz) if v]
    assert len(nz) > m // 2
    assert ctx.r1cs_check(fd, *ptrs, m, dz1.ptr, O.f_add(0, one, r), de.ptr) == (len(nz), nz[0])


def test_relaxed_relation_over_fq(ctx, oracle):
    """the Grumpkin driver's field: NovaProver.check / is_sat_relaxed on a random shape with z = (u | x | w) and E made to fit"""
    import kogarashi_amd as K
    O, fd, m = oracle, 1, 300
    sh = RC.Shape(O, fd, m)
    name, u, ui = RC.u_values(O, fd)[-1]
    z = sh.z.copy()
    z[0] = u
    prods = sh.row_sums(z)
    e = RC.satisfying_e(sh, ui, prods)
    ck = K.PedersenCommitment(O.gen_bases(1, SEED + 4400, 0, 8), curve=1, ctx=ctx)
    prover = K.NovaProver(sh.mats, ck, ctx=ctx)
    assert prover.field == K.KG_FQ
    inst, wit = {"u": u, "x": z[1:4]}, {"w": z[4:], "e": RC.to_mont(e, sh.p)}
    assert prover.check(u, z[1:4], z[4:], wit["e"]) == (0, m) and prover.is_sat_relaxed(inst, wit)
    rows = RC.perturbed_rows(m)
    pe = RC.perturb(sh, e, rows)
    assert prover.check(u, z[1:4], z[4:], RC.to_mont(pe, sh.p)) == (len(rows), rows[0])
    assert not prover.is_sat_relaxed(inst, {"w": z[4:], "e": RC.to_mont(pe, sh.p)})
    assert prover.check(u, z[1:4], z[4:]) == RC.expected(sh, ui, None, prods)[1:]   # E = 0


def test_prover_check_witness(ctx, oracle):
    """Prover.check_witness on the chain circuit of tests/test_gpu_groth16.py: its assignment holds; with one wire changed the two constraints
    that touch it fail -- the case in which create_proof_from_witness returns a proof no verifier accepts"""
    import kogarashi_amd as K
    O = oracle
    cs = O.chain_r1cs(300, O.gen_scalars(0, SEED + 4500, 0, 1)[0])
    params = O.groth16_params(cs, O.gen_scalars(0, SEED + 4501, 0, 5), threads=8)
    params["vk_g2"] = params["vk_g2"][:2]
    prover = K.Prover(params, cs.m, cs.l, cs.m_l_1, ctx=ctx)
    prover.attach_constraint_system(cs.a, cs.b, cs.c)
    assert prover.check_witness(cs.x, cs.w) == (0, cs.m)
    w = cs.w.copy()
    w[40] = cs.w[41]
    assert prover.check_witness(cs.x, w) == (2, 40)
    x = cs.x.copy()
    x[1] = cs.w[7]                                                                  # t_0: constraint 0 alone reads it
    assert prover.check_witness(x, cs.w) == (1, 0)


def test_cpp_wrappers(tmp_path, oracle):
    """include/kogarashi_amd.hpp: R1csShape::is_sat / is_sat_relaxed from a C++ host (tests/host/r1cs_check_cpp_test.cpp)"""
    exe, lib_dir = str(tmp_path / "r1cs_check_cpp_test"), os.path.join(ROOT, "kogarashi_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "r1cs_check_cpp_test.cpp"),
                           "-L" + lib_dir, "-lkogarashi_amd", "-Wl,-rpath," + lib_dir])
    sh = RC.Shape(oracle, 1, 300)
    name, u, ui = RC.u_values(oracle, 1)[-1]
    rows = [RC.LONG_ROW, RC.LONG_ROW + 3, RC.HUGE_ROW, 299]
    pe = RC.perturb(sh, RC.satisfying_e(sh, ui), rows)
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:
        RC.write_record(f, sh, sh.z, u, RC.to_mont(pe, sh.p))
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok: r1cs check wrappers" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    fmt = lambda st: " ".join(str(int(v)) for v in st)
    st, bad, first = RC.expected(sh, ui, pe)
    assert (bad, first) == (4, RC.LONG_ROW)
    assert lines[0] == f"relaxed: sat 0 bad {bad} first {first} status {fmt(st)}"
    st, bad, first = RC.expected(sh, 1, None)
    assert lines[1] == f"plain: sat 0 bad {bad} first {first} status {fmt(st)}"
    assert lines[2] == f"plain, no status: bad {bad} first {first}"
