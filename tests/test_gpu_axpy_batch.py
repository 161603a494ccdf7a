"""kg_field_vec_axpy_batch on the device: out_b = a_b + s_b * b_b for many vectors, each with a scalar of its own read from device memory.
Every word must equal Python integers and what kg_field_vec_axpy writes for the same vector; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import r1cs_cases as RC

pytestmark = pytest.mark.gpu
KG_ERR_BAD_ARG = -2
SEED = RC.SEED + 7500


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def garbage(shape, seed):
    """non-canonical words (bit 255 set): never to be read as field elements"""
    return np.random.default_rng(seed).integers(0, 1 << 63, shape, dtype=np.uint64) | np.uint64(1 << 63)


_DATA = {}


def data(O, fd, n, count):
    """(a, b, s, want) as (count, n, 4), (count, n, 4), (count, 4) arrays and the big-integer result; s walks through 0, 1, p - 1, random"""
    if (fd, n, count) not in _DATA:
        p = RC.MODULI[fd]
        a = O.gen_scalars(fd, SEED + fd, 0, n * count).reshape(count, n, 4)
        b = O.gen_scalars(fd, SEED + 2 + fd, 0, n * count).reshape(count, n, 4)
        rnd = RC.to_ints(O.gen_scalars(fd, SEED + 4 + fd, 0, count), p)
        si = [(0, 1, p - 1, rnd[k])[(k + 3) % 4] for k in range(count)]          # count = 1: the random one
        ai, bi = RC.to_ints(a.reshape(-1, 4), p), RC.to_ints(b.reshape(-1, 4), p)
        want = RC.to_mont([x + si[k // n] * y for k, (x, y) in enumerate(zip(ai, bi))], p).reshape(count, n, 4)
        _DATA[(fd, n, count)] = (a, b, RC.to_mont(si, p), want)
    return _DATA[(fd, n, count)]


def run(ctx, fd, n, count, a, b, s, want, extra, in_place, singles=True):
    sa, sb, so = n + extra[0], n + extra[1], n + extra[2]
    if in_place:
        so = sa
    ha, hb = garbage((count * sa + 2, 4), 21), garbage((count * sb + 2, 4), 22)
    ha[:count * sa].reshape(count, sa, 4)[:, :n] = a
    hb[:count * sb].reshape(count, sb, 4)[:, :n] = b
    guard = ha if in_place else garbage((count * so + 2, 4), 23)
    da, db, ds = ctx.upload(ha), ctx.upload(hb), ctx.upload(s)
    out = da if in_place else ctx.upload(guard)
    ctx.field_vec_axpy_batch(fd, da.ptr, sa, ds.ptr, db.ptr, sb, out.ptr, so, n, count)
    got = out.numpy()
    assert (got[count * so:] == guard[count * so:]).all(), "words written behind the last vector"
    rows, keep = got[:count * so].reshape(count, so, 4), guard[:count * so].reshape(count, so, 4)
    assert (rows[:, n:] == keep[:, n:]).all(), "words written between two vectors"
    bad = np.flatnonzero((rows[:, :n] != want).any(axis=(1, 2)))
    assert len(bad) == 0, (fd, n, count, in_place, bad[:8])
    assert db.numpy().tobytes() == hb.tobytes() and ds.numpy().tobytes() == s.tobytes(), "an input was modified"
    if not in_place:
        assert da.numpy().tobytes() == ha.tobytes(), "an input was modified"
    if singles:
        src = ctx.upload(ha)
        for k in range(count):
            one = ctx.empty((n, 4))
            ctx.field_vec_axpy(fd, src.ptr + 32 * k * sa, s[k], db.ptr + 32 * k * sb, one.ptr, n)
            assert (one.numpy() == want[k]).all(), (fd, n, k, "kg_field_vec_axpy")


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_lengths_around_a_workgroup(ctx, oracle, fd, n):
    """n in {1, 255, 256, 257} x count in {1, 5}, s in {0, 1, p - 1, random}, out of place with three different strides and in place, with
    non-canonical words in the gaps and behind the arrays"""
    for count in (1, 5):
        a, b, s, want = data(oracle, fd, n, count)
        run(ctx, fd, n, count, a, b, s, want, (2, 3, 1), in_place=False)
        run(ctx, fd, n, count, a, b, s, want, (2, 0, 0), in_place=True, singles=False)
        run(ctx, fd, n, count, a, b, s, want, (0, 0, 0), in_place=False, singles=False)


@pytest.mark.parametrize("fd", [0, 1])
def test_more_vectors_than_a_grid_has_rows(ctx, oracle, fd):
    """65537 vectors of 2 elements: the count is not bound by a grid dimension"""
    a, b, s, want = data(oracle, fd, 2, 65537)
    run(ctx, fd, 2, 65537, a, b, s, want, (1, 0, 0), in_place=False, singles=False)
    run(ctx, fd, 2, 65537, a, b, s, want, (0, 0, 0), in_place=True, singles=False)


def test_stream_order_and_status_codes(ctx, oracle):
    """two folds in a row on the stream, the second reading the first's output, no sync between them; refusals leave the output alone"""
    import kogarashi_amd.lib as L
    fd, n, count = 0, 255, 5
    a, b, s, want = data(oracle, fd, n, count)
    p = RC.MODULI[fd]
    da, db, ds = ctx.upload(a), ctx.upload(b), ctx.upload(s)
    mid, out = ctx.empty((count, n, 4)), ctx.empty((count, n, 4))
    threads = ctx.worker_threads()
    ctx.field_vec_axpy_batch(fd, da.ptr, n, ds.ptr, db.ptr, n, mid.ptr, n, n, count)
    ctx.field_vec_axpy_batch(fd, mid.ptr, n, ds.ptr, db.ptr, n, out.ptr, n, n, count)           # (a + s b) + s b
    assert ctx.worker_threads() == threads
    si, ai, bi = RC.to_ints(s, p), RC.to_ints(a.reshape(-1, 4), p), RC.to_ints(b.reshape(-1, 4), p)
    twice = RC.to_mont([x + 2 * si[k // n] * y for k, (x, y) in enumerate(zip(ai, bi))], p).reshape(count, n, 4)
    assert (out.numpy() == twice).all() and (mid.numpy() == want).all()
    guard = garbage((count, n, 4), 24)
    dg = ctx.upload(guard)
    poison = 0xDEAD0000BEEF0000
    vp = lambda q: C.c_void_p(int(q) if q else 0)

    def raw(h=ctx._h, field=0, a=poison, sa=n, s=poison, b=poison, sb=n, out=dg.ptr, so=n, n=n, count=count):
        return ctx._lib.kg_field_vec_axpy_batch(h, field, vp(a), C.c_size_t(sa), vp(s), vp(b), C.c_size_t(sb), vp(out), C.c_size_t(so), C.c_size_t(n), C.c_size_t(count))

    over = (1 << 64) // 32 // count + 1
    for kw in (dict(h=None), dict(field=2), dict(field=-1), dict(sa=n - 1), dict(sb=n - 1), dict(so=n - 1), dict(so=n - 1, count=0), dict(a=0), dict(s=0), dict(b=0),
               dict(out=0), dict(sa=over), dict(sb=over), dict(so=over)):
        assert raw(**kw) == KG_ERR_BAD_ARG, kw
    assert raw(count=0) == 0 and raw(n=0, sa=0, sb=0, so=0) == 0 and raw(count=0, a=0, s=0, b=0, out=0) == 0
    ctx.sync()
    assert (dg.numpy() == guard).all()
    with pytest.raises(L.KogarashiError):
        ctx.field_vec_axpy_batch(fd, 0, n, ds.ptr, db.ptr, n, dg.ptr, n, n, count)
