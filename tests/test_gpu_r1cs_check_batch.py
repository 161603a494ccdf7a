"""kg_r1cs_check_batch on the device: kg_r1cs_check for many vectors against one shape in one enqueue, results left in device memory.  Every
status byte and every summary word must equal what Python integers give (tests/r1cs_check_batch_cases.py on tests/r1cs_cases.py's expected())
and what kg_r1cs_check returns and writes for the same vector; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import r1cs_cases as RC
import r1cs_check_batch_cases as BC

pytestmark = pytest.mark.gpu
KG_ERR_BAD_ARG = -2


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def resident(ctx):
    """shape -> its matrices' device pointers, uploaded once"""
    cache = {}

    def get(sh):
        if id(sh) not in cache:
            cache[id(sh)] = (sh,) + BC.upload_shape(ctx, sh)
        return cache[id(sh)][2]
    return get


class Call:
    """one kg_r1cs_check_batch on packed uploads into guarded outputs; nothing is synchronised until collect()"""

    def __init__(self, ctx, ptrs, sh, vecs, given=True, status=True, extra=(0, 0, 0)):
        self.ctx, self.ptrs, self.sh, self.vecs, self.given, self.with_status = ctx, ptrs, sh, vecs, given, status
        self.count = len(vecs)
        self.z_stride, self.e_stride, self.st_stride = sh.nvars + extra[0], sh.m + extra[1], sh.m + extra[2]
        self.host = BC.pack(sh, vecs, self.z_stride, self.e_stride)
        self.dz, self.du, self.de = (ctx.upload(a) for a in self.host)
        self.d_status = ctx.upload(np.full(self.count * self.st_stride + 16, BC.GUARD8, dtype=np.uint8))
        self.d_sum = ctx.upload(np.full((self.count + 2, 2), BC.GUARD32, dtype=np.uint32))

    def enqueue(self):
        got = self.ctx.r1cs_check_batch(self.sh.fd, *self.ptrs, self.sh.m, self.dz.ptr, self.z_stride, self.count, self.du.ptr if self.given else 0,
                                        self.de.ptr if self.given else 0, self.e_stride, self.d_status.ptr if self.with_status else 0, self.st_stride,
                                        summary=self.d_sum)
        assert got is self.d_sum
        return self

    def collect(self):
        """(status[count, m] or None, summary[count, 2]) after the guards and the inputs have been looked at"""
        m, count = self.sh.m, self.count
        st, sums = self.d_status.numpy(), self.d_sum.numpy()
        assert (sums[count:] == BC.GUARD32).all(), "summary words written beyond count pairs"
        assert (st[count * self.st_stride:] == BC.GUARD8).all(), "status bytes written beyond the last vector"
        rows = st[:count * self.st_stride].reshape(count, self.st_stride)
        assert (rows[:, m:] == BC.GUARD8).all(), "status bytes written between two vectors' rows"
        if not self.with_status:
            assert (rows == BC.GUARD8).all(), "status bytes written though d_status was NULL"
        for host, dev in zip(self.host, (self.dz, self.du, self.de)):
            assert dev.numpy().tobytes() == host.tobytes(), "an input was modified"
        return (rows[:, :m] if self.with_status else None), sums[:count]

    def assert_matches(self, singles=True):
        """against Python integers, and against kg_r1cs_check run on each vector where it lies"""
        sh, ctx = self.sh, self.ctx
        st, sums = self.collect()
        for b, v in enumerate(self.vecs):
            want = v.want(sh, plain=not self.given)
            assert tuple(int(x) for x in sums[b]) == want[1:], (sh.fd, sh.m, b, v.name, sums[b], want[1:])
            if st is not None:
                assert (st[b] == want[0]).all(), (sh.fd, sh.m, b, v.name, np.flatnonzero(st[b] != want[0])[:8])
            if singles:
                one = ctx.upload(np.full(sh.m, 0xAA, dtype=np.uint8))
                got = ctx.r1cs_check(sh.fd, *self.ptrs, sh.m, self.dz.ptr + 32 * b * self.z_stride, v.u if self.given else None,
                                     self.de.ptr + 32 * b * self.e_stride if self.given else 0, one.ptr)
                assert got == want[1:] and (one.numpy() == want[0]).all(), (sh.fd, sh.m, b, v.name, "kg_r1cs_check")


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("given", [True, False], ids=["u and E given", "d_u and d_e NULL"])
def test_six_vectors_over_every_row_class(ctx, oracle, resident, fd, given):
    """m = 300: the 48 / 49 edge, rows of 200, 254 and 5000 entries, rows empty everywhere; a satisfied vector, E perturbed, flip_z(), every
    row bad, u = 0, u = p - 1 -- each with a summary of its own, also when the same z array is checked with u = 1 and E = 0"""
    sh, vecs = BC.case300(oracle, fd)
    Call(ctx, resident(sh), sh, vecs, given=given).enqueue().assert_matches()


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("m", BC.SMALL_SIZES)
def test_wave_and_workgroup_edges(ctx, oracle, resident, fd, m):
    sh, vecs = BC.small_case(oracle, fd, m)
    Call(ctx, resident(sh), sh, vecs).enqueue().assert_matches()


@pytest.mark.parametrize("fd", [0, 1])
def test_strides_with_garbage_and_guards(ctx, oracle, resident, fd):
    """z_stride, e_stride and status_stride all larger than needed, non-canonical words between the vectors and between the E vectors, 0xA5
    between the vectors' status rows and behind every output; the same once more with d_status NULL"""
    sh, vecs = BC.case300(oracle, fd)
    Call(ctx, resident(sh), sh, vecs, extra=(3, 5, 7)).enqueue().assert_matches()
    Call(ctx, resident(sh), sh, vecs, extra=(3, 5, 7), status=False).enqueue().assert_matches(singles=False)


def test_more_vectors_than_the_grid_has_rows(ctx, oracle, resident):
    """count = 65537: chunks of 65535 and 2 vectors.  Row 1 of the 3-row shape is on the work list, which only the first chunk builds: vector
    65536 fails through it.  Vectors 65534, 65535, 65536 are bad at rows 2, 0, 1; every other pair must be (0, 3) and every other byte 0."""
    sh, base, special = BC.ymax_case(oracle)
    ptrs, count, m = resident(sh), BC.YMAX_COUNT, 3
    z = np.ascontiguousarray(np.broadcast_to(base.z, (count, 8, 4)))
    want_st, want_sum = np.zeros((count, m), dtype=np.uint8), np.tile(np.array([0, m], dtype=np.uint32), (count, 1))
    assert base.want(sh)[1:] == (0, m)
    for b, v in special.items():
        z[b] = v.z
        st, bad, first = v.want(sh)
        want_st[b], want_sum[b] = st, (bad, first)
    dz = ctx.upload(z)
    d_status = ctx.upload(np.full(count * m + 16, BC.GUARD8, dtype=np.uint8))
    d_sum = ctx.upload(np.full((count + 2, 2), BC.GUARD32, dtype=np.uint32))
    ctx.r1cs_check_batch(0, *ptrs, m, dz.ptr, 8, count, 0, 0, 0, d_status.ptr, m, summary=d_sum)
    st, sums = d_status.numpy(), d_sum.numpy()
    assert (sums[count:] == BC.GUARD32).all() and (st[count * m:] == BC.GUARD8).all()
    bad_pairs = np.flatnonzero((sums[:count] != want_sum).any(axis=1))
    assert len(bad_pairs) == 0, (bad_pairs[:8], sums[bad_pairs[:8]])
    assert (st[:count * m].reshape(count, m) == want_st).all()
    for b in (0, 1, 32767, 65533, 65534, 65535, 65536):                              # kg_r1cs_check on a sample: the clean ones are clean
        one = ctx.upload(np.full(m, 0xAA, dtype=np.uint8))
        assert ctx.r1cs_check(0, *ptrs, m, dz.ptr + 32 * 8 * b, status=one.ptr) == tuple(int(x) for x in want_sum[b]) and (one.numpy() == want_st[b]).all(), b


def test_stream_order(ctx, oracle, resident):
    """two different shapes back to back without a sync between them (the work list and its counters are rebuilt per call); a
    kg_field_vec_axpy fold enqueued just before the check is seen by it; no worker thread is started"""
    sh1, vecs1 = BC.case300(oracle, 0)
    sh2, vecs2 = BC.small_case(oracle, 0, 65)
    c1, c2, c3 = Call(ctx, resident(sh1), sh1, vecs1), Call(ctx, resident(sh2), sh2, vecs2), Call(ctx, resident(sh1), sh1, vecs1)
    # vector 0 of the third call: its E starts as zero and is folded in on the stream, E = 0 + 1 * E
    v0 = vecs1[0]
    assert RC.expected(sh1, v0.ui, None, v0.prods)[1] > 0 and v0.want(sh1)[1] == 0           # without the fold it fails, with it it holds
    e_src = ctx.upload(c3.host[2][0, :sh1.m])
    ctx.write(c3.de.ptr, np.zeros((sh1.m, 4), dtype=np.uint64))
    one = oracle.f_consts(0)["r"]
    threads = ctx.worker_threads()
    ctx.sync()
    c1.enqueue()
    c2.enqueue()
    ctx.field_vec_axpy(0, c3.de.ptr, one, e_src.ptr, c3.de.ptr, sh1.m)
    c3.enqueue()
    assert ctx.worker_threads() == threads
    ctx.sync()
    c1.assert_matches(singles=False)
    c2.assert_matches(singles=False)
    c3.assert_matches(singles=False)
    assert ctx.worker_threads() == threads


@pytest.mark.parametrize("fd", [0, 1])
def test_single_and_batched_calls_share_one_work_space(ctx, oracle, resident, fd):
    """One context, m = 300, nothing synchronised in between: a single check, a batched check of 3, a single cross term, a batched product of
    2, a single product and a single check once more.  They share the launcher, the initialiser and the work space (the list, its two counters
    and the single check's summary pair; the product alone has a list's back, row 61 of matrix B), so each call must rebuild what it uses.
    Every word is compared with the oracle or with Python integers."""
    O = oracle
    sh, vecs = BC.case300(O, fd)
    ptrs, m, n = resident(sh), sh.m, sh.nvars
    first, last = vecs[1], vecs[4]                                                  # bad at perturbed_rows(m); the same z, plain, at the end
    batch = Call(ctx, ptrs, sh, [vecs[0], vecs[2], vecs[4]])
    dz, de = ctx.upload(first.z), ctx.upload(RC.to_mont(first.e, sh.p))
    d_st = ctx.upload(np.full(m, 0xAA, dtype=np.uint8))
    u1, u2 = vecs[0].u, vecs[5].u                                                   # random, p - 1
    dz1, dz2, d_t = ctx.upload(vecs[2].z), ctx.upload(vecs[3].z), ctx.upload(np.zeros((m, 4), dtype=np.uint64))
    zb = np.stack([vecs[3].z, last.z])
    dzb, d_pb, d_p = ctx.upload(zb), ctx.upload(np.zeros((2, m, 4), dtype=np.uint64)), ctx.upload(np.zeros((m, 4), dtype=np.uint64))
    assert sh.row_lengths()[1, RC.HUGE_ROW] == 5000
    ctx.sync()
    got_first = ctx.r1cs_check(fd, *ptrs, m, dz.ptr, first.u, de.ptr, d_st.ptr)     # (blocks, by its nature: the pair comes back)
    batch.enqueue()
    ctx.nova_cross_term(fd, *ptrs, m, dz1.ptr, dz2.ptr, u1, u2, d_t.ptr)
    ctx.r1cs_prod_batch(fd, *ptrs[1], m, dzb.ptr, n, 2, d_pb.ptr, m)
    ctx.r1cs_prod(fd, *ptrs[1], m, dz.ptr, d_p.ptr)
    got_last = ctx.r1cs_check(fd, *ptrs, m, dzb.ptr + 32 * n)
    ctx.sync()
    want = first.want(sh)
    assert got_first == want[1:] and want[1] == len(RC.perturbed_rows(m)) and (d_st.numpy() == want[0]).all()
    batch.assert_matches(singles=False)
    assert (d_t.numpy() == O.nova_cross_term(fd, *sh.mats, vecs[2].z, vecs[3].z, u1, u2)).all()
    for b in range(2):
        assert (d_pb.numpy()[b] == O.matrix_prod(fd, sh.mats[1], zb[b])).all(), b
    assert (d_p.numpy() == O.matrix_prod(fd, sh.mats[1], first.z)).all()
    assert got_last == last.want(sh, plain=True)[1:] and got_last != got_first


def test_status_codes(ctx, oracle, resident):
    """KG_ERR_BAD_ARG before anything is dereferenced or enqueued -- the pointers of the refused calls are poisoned --, the outputs untouched;
    count == 0 enqueues nothing; m == 0 writes (0, 0) into count pairs and nothing else"""
    import kogarashi_amd.lib as L
    sh, vecs = BC.small_case(oracle, 0, 13)
    ptrs = resident(sh)
    call = Call(ctx, ptrs, sh, vecs)
    full = [L.Csr(*t) for t in ptrs]
    poison = 0xDEAD0000BEEF0000
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    ref = lambda v: C.byref(v) if v is not None else None
    m, n, count = sh.m, sh.nvars, call.count

    def raw(h=ctx._h, field=0, mats=full, m=m, z=poison, zs=n, count=count, u=poison, e=poison, es=m, st=call.d_status.ptr, ss=m, sm=call.d_sum.ptr):
        return ctx._lib.kg_r1cs_check_batch(h, field, ref(mats[0]), ref(mats[1]), ref(mats[2]), C.c_size_t(m), vp(z), C.c_size_t(zs), C.c_size_t(count), vp(u), vp(e),
                                            C.c_size_t(es), vp(st), C.c_size_t(ss), vp(sm))

    def untouched():
        ctx.sync()
        return (call.d_status.numpy() == BC.GUARD8).all() and (call.d_sum.numpy() == BC.GUARD32).all()

    refused = [dict(h=None), dict(field=2), dict(field=-1), dict(m=1 << 32), dict(sm=0), dict(z=0), dict(es=m - 1), dict(ss=m - 1),
               dict(zs=(1 << 64) // 32 // count + 1), dict(es=(1 << 64) // 32 // count + 1), dict(ss=(1 << 64) // count + 1)]
    for which in range(3):
        mats = list(full)
        mats[which] = None
        refused.append(dict(mats=mats))
        for member in range(3):
            t = list(ptrs[which])
            t[member] = None
            mats = list(full)
            mats[which] = L.Csr(*t)
            refused.append(dict(mats=mats))
    for kw in refused:
        assert raw(**kw) == KG_ERR_BAD_ARG and untouched(), kw
    assert raw(count=0) == 0 and raw(count=0, mats=[None, None, None], sm=0, st=0) == 0 and untouched()
    assert raw(m=0, mats=[None, None, None], z=0, u=0, e=0, st=0) == 0                          # m == 0: the pairs alone
    ctx.sync()
    sums = call.d_sum.numpy()
    assert (sums[:count] == 0).all() and (sums[count:] == BC.GUARD32).all() and (call.d_status.numpy() == BC.GUARD8).all()
    with pytest.raises(L.KogarashiError):
        ctx.r1cs_check_batch(0, *ptrs, m, 0, n, count)
    call2 = Call(ctx, ptrs, sh, vecs)                                                            # and the context keeps working
    call2.enqueue().assert_matches()
