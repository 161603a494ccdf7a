"""kg_nova_cross_term_batch on the device: Nova's cross term for many pairs (z1_b, z2_b, u1_b, u2_b) against one shape in one enqueue.  Every
word of every T_b must equal the oracle's restatement (Prover::compute_cross_term) and what kg_nova_cross_term writes for the same pair;
nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import r1cs_cases as RC
import r1cs_check_batch_cases as BC

pytestmark = pytest.mark.gpu
KG_ERR_BAD_ARG = -2
SEED = RC.SEED + 7000


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


_SHAPES, _PAIRS = {}, {}


def shape(O, fd, m):
    if (fd, m) not in _SHAPES:
        _SHAPES[(fd, m)] = RC.Shape(O, fd, m)
    return _SHAPES[(fd, m)]


def pairs(O, sh, count):
    """count pairs (z1, z2, u1, u2, T) over the shape: random vectors, u1 and u2 walking through u_values' 1, 0, p - 1 and a random value at
    different phases; T from the oracle, computed once per (shape, count)"""
    key = (sh.fd, sh.m, count)
    if key not in _PAIRS:
        us = [u for name, u, _ in RC.u_values(O, sh.fd) if u is not None]
        one = O.f_consts(sh.fd)["r"]
        out = []
        for b in range(count):
            z1 = O.gen_scalars(sh.fd, SEED + 64 * sh.m + 2 * b, 0, sh.nvars)
            z2 = O.gen_scalars(sh.fd, SEED + 64 * sh.m + 2 * b + 1, 0, sh.nvars)
            u1, u2 = us[(b + 3) % 4], us[(b // 2 + 1) % 4]
            z1[0], z2[0] = u1, one                                  # z = (u | x | w), as a fold hands it in (the entry does not care)
            t_given = O.nova_cross_term(sh.fd, sh.mats[0], sh.mats[1], sh.mats[2], z1, z2, u1, u2)
            t_null = O.nova_cross_term(sh.fd, sh.mats[0], sh.mats[1], sh.mats[2], z1, z2, u1, one)
            out.append((z1, z2, u1, u2, t_given, t_null))
        _PAIRS[key] = out
    return _PAIRS[key]


def garbage(shape_, seed):
    """non-canonical words (bit 255 set): never to be read as field elements"""
    return np.random.default_rng(seed).integers(0, 1 << 63, shape_, dtype=np.uint64) | np.uint64(1 << 63)


class Call:
    """one kg_nova_cross_term_batch on packed uploads into a guarded output; nothing is synchronised until check()"""

    def __init__(self, ctx, ptrs, sh, prs, u2_given, extra=(0, 0, 0)):
        self.ctx, self.ptrs, self.sh, self.prs, self.u2_given = ctx, ptrs, sh, prs, u2_given
        count, m, n = len(prs), sh.m, sh.nvars
        self.count, self.s1, self.s2, self.so = count, n + extra[0], n + extra[1], m + extra[2]
        z1, z2 = garbage((count, self.s1, 4), 11), garbage((count, self.s2, 4), 12)
        for b, p in enumerate(prs):
            z1[b, :n], z2[b, :n] = p[0], p[1]
        self.host = (z1, z2, np.stack([p[2] for p in prs]), np.stack([p[3] for p in prs]))
        self.dz1, self.dz2, self.du1, self.du2 = (ctx.upload(a) for a in self.host)
        self.guard = garbage((count * self.so + 4, 4), 13)
        self.out = ctx.upload(self.guard)

    def enqueue(self):
        self.ctx.nova_cross_term_batch(self.sh.fd, *self.ptrs, self.sh.m, self.dz1.ptr, self.s1, self.dz2.ptr, self.s2, self.count, self.du1.ptr,
                                       self.du2.ptr if self.u2_given else 0, self.out.ptr, self.so)
        return self

    def check(self, singles=True):
        sh, ctx, m, count = self.sh, self.ctx, self.sh.m, self.count
        got = self.out.numpy()
        assert (got[count * self.so:] == self.guard[count * self.so:]).all(), "words written behind the last output"
        rows, keep = got[:count * self.so].reshape(count, self.so, 4), self.guard[:count * self.so].reshape(count, self.so, 4)
        assert (rows[:, m:] == keep[:, m:]).all(), "words written between two outputs"
        for host, dev in zip(self.host, (self.dz1, self.dz2, self.du1, self.du2)):
            assert dev.numpy().tobytes() == host.tobytes(), "an input was modified"
        one = sh.O.f_consts(sh.fd)["r"]
        for b, p in enumerate(self.prs):
            want = p[4] if self.u2_given else p[5]
            assert (rows[b, :m] == want).all(), (sh.fd, m, b, np.flatnonzero((rows[b, :m] != want).any(axis=1))[:8])
            if singles:
                t = ctx.empty((m, 4))
                ctx.nova_cross_term(sh.fd, *self.ptrs, m, self.dz1.ptr + 32 * b * self.s1, self.dz2.ptr + 32 * b * self.s2, p[2], p[3] if self.u2_given else one,
                                    t.ptr)
                assert (t.numpy() == want).all(), (sh.fd, m, b, "kg_nova_cross_term")


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("u2_given", [True, False], ids=["u2 given", "d_u2 NULL"])
def test_six_pairs_over_every_row_class(ctx, oracle, resident, fd, u2_given):
    """m = 300: the 48 / 49 edge in one matrix only, rows of 200, 254 and 5000 entries, rows empty everywhere; strides larger than needed
    with non-canonical words in the gaps, guard words behind the last output"""
    sh = shape(oracle, fd, 300)
    Call(ctx, resident(sh), sh, pairs(oracle, sh, 6), u2_given, extra=(3, 4, 5)).enqueue().check()
    Call(ctx, resident(sh), sh, pairs(oracle, sh, 6)[:1], u2_given).enqueue().check()             # count = 1, tight strides


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 12, 13, 65])
def test_small_shapes(ctx, oracle, resident, fd, m):
    """no work list up to m = 12, one from m = 13 on; a full wave and one row more; count 1 and 6"""
    sh = shape(oracle, fd, m)
    assert (sh.row_lengths().max() > 48) == (m > 12)
    prs = pairs(oracle, sh, 6)
    Call(ctx, resident(sh), sh, prs, True, extra=(1, 0, 2)).enqueue().check()
    Call(ctx, resident(sh), sh, prs[4:5], False).enqueue().check()


def test_two_shapes_back_to_back_and_stream_order(ctx, oracle, resident):
    """two different shapes on one context without a sync between them (the work list and its counters are rebuilt per call), a kernel
    enqueued behind the second call reads its T in stream order; no worker thread is started"""
    sh1, sh2 = shape(oracle, 0, 300), shape(oracle, 0, 65)
    c1 = Call(ctx, resident(sh1), sh1, pairs(oracle, sh1, 6), True)
    c2 = Call(ctx, resident(sh2), sh2, pairs(oracle, sh2, 6), True)
    c3 = Call(ctx, resident(sh1), sh1, pairs(oracle, sh1, 6), False)
    n = c2.count * c2.so
    behind = ctx.upload(np.zeros((n, 4), dtype=np.uint64))
    one = oracle.f_consts(0)["r"]
    threads = ctx.worker_threads()
    ctx.sync()
    c1.enqueue()
    c2.enqueue()
    ctx.field_vec_axpy(0, behind.ptr, one, c2.out.ptr, behind.ptr, n)                # 0 + 1 * T: reads T behind the call
    c3.enqueue()
    assert ctx.worker_threads() == threads
    ctx.sync()
    for c in (c1, c2, c3):
        c.check(singles=False)
    assert (behind.numpy() == c2.out.numpy()[:n]).all()
    assert ctx.worker_threads() == threads


def test_more_pairs_than_the_grid_has_rows(ctx, oracle, resident):
    """count = 65537: chunks of 65535 and 2 pairs over the 3-row shape whose middle row (49 entries) is on the work list, which only the
    first chunk builds.  A base pair repeated, three special pairs at 65534, 65535 and 65536; every output row of every pair is checked."""
    sh, base, special = BC.ymax_case(oracle)
    O, ptrs, count, m, n = oracle, resident(sh), BC.YMAX_COUNT, 3, 8
    one = O.f_consts(0)["r"]
    us = [u for name, u, _ in RC.u_values(O, 0) if u is not None]
    z2_base = O.gen_scalars(0, SEED + 1, 0, n)
    z1 = np.ascontiguousarray(np.broadcast_to(base.z, (count, n, 4)))
    z2 = np.ascontiguousarray(np.broadcast_to(z2_base, (count, n, 4)))
    u1 = np.ascontiguousarray(np.broadcast_to(one, (count, 4)))
    t_base = O.nova_cross_term(0, *sh.mats, base.z, z2_base, one, one)
    want = np.ascontiguousarray(np.broadcast_to(t_base, (count, m, 4)))
    for k, (b, v) in enumerate(sorted(special.items())):
        z1[b], u1[b] = v.z, us[1 + k]
        z2[b] = O.gen_scalars(0, SEED + 2 + k, 0, n)
        want[b] = O.nova_cross_term(0, *sh.mats, z1[b], z2[b], u1[b], one)
        assert (want[b] != t_base).any(axis=1).all(), "a special pair differs from the base in every row"
    guard = garbage((count * m + 4, 4), 14)
    dz1, dz2, du1, out = ctx.upload(z1), ctx.upload(z2), ctx.upload(u1), ctx.upload(guard)
    ctx.nova_cross_term_batch(0, *ptrs, m, dz1.ptr, n, dz2.ptr, n, count, du1.ptr, 0, out.ptr, m)
    got = out.numpy()
    assert (got[count * m:] == guard[count * m:]).all()
    bad = np.flatnonzero((got[:count * m].reshape(count, m, 4) != want).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:8]
    for b in (0, 65533, 65534, 65535, 65536):                                        # kg_nova_cross_term on a sample
        t = ctx.empty((m, 4))
        ctx.nova_cross_term(0, *ptrs, m, dz1.ptr + 32 * n * b, dz2.ptr + 32 * n * b, u1[b], one, t.ptr)
        assert (t.numpy() == want[b]).all(), b


def test_status_codes(ctx, oracle, resident):
    """KG_ERR_BAD_ARG before anything is dereferenced or enqueued -- the pointers of the refused calls are poisoned --, the output untouched;
    count == 0 and m == 0 enqueue nothing"""
    import kogarashi_amd.lib as L
    sh = shape(oracle, 0, 13)
    ptrs = resident(sh)
    call = Call(ctx, ptrs, sh, pairs(oracle, sh, 6), True)
    full = [L.Csr(*t) for t in ptrs]
    poison = 0xDEAD0000BEEF0000
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    ref = lambda v: C.byref(v) if v is not None else None
    m, n, count = sh.m, sh.nvars, call.count

    def raw(h=ctx._h, field=0, mats=full, m=m, z1=poison, s1=n, z2=poison, s2=n, count=count, u1=poison, u2=poison, out=call.out.ptr, so=m):
        return ctx._lib.kg_nova_cross_term_batch(h, field, ref(mats[0]), ref(mats[1]), ref(mats[2]), C.c_size_t(m), vp(z1), C.c_size_t(s1), vp(z2), C.c_size_t(s2),
                                                 C.c_size_t(count), vp(u1), vp(u2), vp(out), C.c_size_t(so))

    def untouched():
        ctx.sync()
        return (call.out.numpy() == call.guard).all()

    over = (1 << 64) // 32 // count + 1
    refused = [dict(h=None), dict(field=2), dict(field=-1), dict(m=1 << 32, so=1 << 32), dict(so=m - 1), dict(so=m - 1, count=0), dict(z1=0), dict(z2=0), dict(out=0),
               dict(s1=over), dict(s2=over), dict(so=over)]
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
    assert raw(count=0) == 0 and raw(count=0, mats=[None, None, None], out=0) == 0 and raw(m=0, so=0, mats=[None, None, None]) == 0 and untouched()
    with pytest.raises(L.KogarashiError):
        ctx.nova_cross_term_batch(0, *ptrs, m, 0, n, 0, n, count, 0, 0, call.out.ptr, m)
    call.enqueue().check()                                                           # and the context keeps working
