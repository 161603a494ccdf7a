"""kg_r1cs_prod_batch (csrc/vec.hip): one CSR matrix against many vectors in one call -- the sparse-row walker over a grid whose y index is
the vector, the work list of long rows built once per call.  The product is exact, so every check is equality of all words: against the
oracle's SparseMatrix::prod per vector and against kg_r1cs_prod on the same vector.  Shapes are those of tests/r1cs_cases.py: m = 300 holds
every row class (empty rows, rows of exactly 48 and 49 entries, a row of 200, rows of 254, one row of 5000 entries: B only), m = 13 has the
wave rows without the huge one, m = 1 is the trivial edge."""
import ctypes as C

import numpy as np
import pytest

from r1cs_cases import MODULI, SEED, Shape, to_ints, to_mont

pytestmark = pytest.mark.gpu
GUARD64 = np.uint64(0xDEADBEEFCAFEF00D)
GARBAGE = np.uint64(0xFFFFFFFFFFFFFFFF)                  # non-canonical in every word
KG_ERR_BAD_ARG = -2
MAXCOUNT = 5


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


_CASES = {}


def case(O, ctx, fd, m):
    """(shape, the device triples of its three matrices, MAXCOUNT distinct z vectors [b, nvars, 4], the oracle's products [matrix][b] as
    (m, 4) arrays): computed once per (field, m) and left unchanged"""
    key = (id(ctx), fd, m)
    if key not in _CASES:
        sh = Shape(O, fd, m)
        zs = np.ascontiguousarray(O.gen_scalars(fd, SEED + 5000 + 16 * m + fd, 0, MAXCOUNT * sh.nvars)).reshape(MAXCOUNT, sh.nvars, 4)
        want = [[np.asarray(O.matrix_prod(fd, t, np.ascontiguousarray(zs[b])), dtype=np.uint64).reshape(m, 4) for b in range(MAXCOUNT)] for t in sh.mats]
        _CASES[key] = (sh, [upload_csr(ctx, t) for t in sh.mats], zs, want)
    return _CASES[key]


def upload_csr(ctx, t):
    rp, col, val = t
    col = np.ascontiguousarray(col, dtype=np.uint64)
    val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
    return (ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)), ctx.upload(col if len(col) else np.zeros(1, dtype=np.uint64)),
            ctx.upload(val if len(val) else np.zeros((1, 4), dtype=np.uint64)))


def strided(vecs, stride, fill):
    """[count, n, 4] -> [count, stride, 4] with `fill` in the gaps"""
    count, n = vecs.shape[0], vecs.shape[1]
    out = np.full((count, stride, 4), fill, dtype=np.uint64)
    out[:, :n] = vecs
    return out


@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("m", [1, 13, 300])
@pytest.mark.parametrize("fd", [0, 1])
def test_every_row_class_both_fields(ctx, oracle, fd, m, count):
    """all three matrices of the shape against `count` distinct vectors, dense strides: the oracle per vector, and kg_r1cs_prod bit for bit"""
    sh, dev, zs, want = case(oracle, ctx, fd, m)
    if m == 300:
        lens = sh.row_lengths()
        assert 48 in lens[0] and 49 in lens[2] and 200 in lens[0] and 254 in lens[1] and 5000 in lens[1] and (lens.sum(axis=0) == 0).any()
    dz = ctx.upload(np.ascontiguousarray(zs[:count]))
    for j, d in enumerate(dev):
        out = ctx.upload(np.full((count + 1, m, 4), GUARD64, dtype=np.uint64))
        ctx.r1cs_prod_batch(fd, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr, sh.nvars, count, out.ptr, m)
        got = out.numpy()
        assert (got[count] == GUARD64).all(), "written behind the last output"
        single = ctx.empty((m, 4))
        for b in range(count):
            assert (got[b] == want[j][b]).all(), (fd, m, count, j, b, "oracle")
            ctx.r1cs_prod(fd, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr + 32 * b * sh.nvars, single.ptr)
            assert got[b].tobytes() == single.numpy().tobytes(), (fd, m, count, j, b, "kg_r1cs_prod")


@pytest.mark.parametrize("fd", [0, 1])
def test_strides_with_garbage_and_guards(ctx, oracle, fd):
    """z_stride = nvars + 3 and out_stride = m + 5: garbage in the input gaps is never read into a sum, the guard values in the output gaps
    and behind the last output are untouched, the inputs are byte-identical after the call"""
    m, count = 300, 3
    sh, dev, zs, want = case(oracle, ctx, fd, m)
    zstride, ostride = sh.nvars + 3, m + 5
    hz = strided(zs[:count], zstride, GARBAGE)
    dz = ctx.upload(hz)
    for j, d in enumerate(dev):
        out = ctx.upload(np.full((count * ostride + 7, 4), GUARD64, dtype=np.uint64))
        ctx.r1cs_prod_batch(fd, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr, zstride, count, out.ptr, ostride)
        flat = out.numpy()
        got = flat[:count * ostride].reshape(count, ostride, 4)
        for b in range(count):
            assert (got[b, :m] == want[j][b]).all(), (fd, j, b)
        assert (got[:, m:] == GUARD64).all(), "an output gap was written"
        assert (flat[count * ostride:] == GUARD64).all(), "written behind the last output"
    assert dz.numpy().tobytes() == hz.tobytes()


def test_work_list_is_per_call_and_per_matrix(ctx, oracle):
    """two calls back to back on one context, different matrices (m = 300's B with its huge row, then m = 13's A) and different counts,
    then the first again with one vector: a list or counter that was not rebuilt, or a list that grew with count, shows in one of them"""
    s300, d300, z300, w300 = case(oracle, ctx, 0, 300)
    s13, d13, z13, w13 = case(oracle, ctx, 0, 13)
    dz300, dz13 = ctx.upload(np.ascontiguousarray(z300[:3])), ctx.upload(np.ascontiguousarray(z13))
    o1, o2, o3 = ctx.empty((3, 300, 4)), ctx.empty((5, 13, 4)), ctx.empty((1, 300, 4))
    ctx.sync()
    ctx.r1cs_prod_batch(0, d300[1][0].ptr, d300[1][1].ptr, d300[1][2].ptr, 300, dz300.ptr, s300.nvars, 3, o1.ptr, 300)
    ctx.r1cs_prod_batch(0, d13[0][0].ptr, d13[0][1].ptr, d13[0][2].ptr, 13, dz13.ptr, s13.nvars, 5, o2.ptr, 13)
    ctx.r1cs_prod_batch(0, d300[0][0].ptr, d300[0][1].ptr, d300[0][2].ptr, 300, dz300.ptr, s300.nvars, 1, o3.ptr, 300)
    ctx.sync()
    g1, g2, g3 = o1.numpy(), o2.numpy(), o3.numpy()
    for b in range(3):
        assert (g1[b] == w300[1][b]).all(), ("first call", b)
    for b in range(5):
        assert (g2[b] == w13[0][b]).all(), ("second call", b)
    assert (g3[0] == w300[0][0]).all(), "third call"


def test_chunk_edge_65537_vectors(ctx, oracle):
    """The vector index is the grid's y dimension, cut at 65535: count = 65537 is a chunk of 65535 and one of 2.  A matrix of 2 rows and 3
    entries over 2 variables; the z vectors cycle through 7 distinct ones, so the expectation is 7 oracle products tiled; every output is
    compared."""
    O, fd, count = oracle, 0, 65537
    rp = np.array([0, 2, 3], dtype=np.uint64)
    col = np.array([0, 1, 1], dtype=np.uint64)
    val = np.ascontiguousarray(O.gen_scalars(fd, SEED + 5100, 0, 3))
    z7 = np.ascontiguousarray(O.gen_scalars(fd, SEED + 5101, 0, 14)).reshape(7, 2, 4)
    want7 = np.stack([np.asarray(O.matrix_prod(fd, (rp, col, val), np.ascontiguousarray(z7[k])), dtype=np.uint64).reshape(2, 4) for k in range(7)])
    idx = np.arange(count) % 7
    d = upload_csr(ctx, (rp, col, val))
    dz = ctx.upload(np.ascontiguousarray(z7[idx]))
    out = ctx.upload(np.full((count + 1, 2, 4), GUARD64, dtype=np.uint64))
    ctx.r1cs_prod_batch(fd, d[0].ptr, d[1].ptr, d[2].ptr, 2, dz.ptr, 2, count, out.ptr, 2)
    got = out.numpy()
    assert (got[count] == GUARD64).all()
    assert (got[:count] == want7[idx]).all(), np.flatnonzero((got[:count] != want7[idx]).any(axis=(1, 2)))[:8]


def test_stream_order(ctx, oracle):
    """kg_field_vec_axpy produces the z block, the batched product reads it and a kg_field_vec_op reads the product: three enqueues, no
    sync in between, one sync, compare (z = a + s b and the doubling restated in Python integers)"""
    O, fd, m, count = oracle, 0, 300, 3
    sh, dev, _, _ = case(O, ctx, fd, m)
    p, n = MODULI[fd], count * sh.nvars
    a, b = O.gen_scalars(fd, SEED + 5200, 0, n), O.gen_scalars(fd, SEED + 5201, 0, n)
    s = O.gen_scalars(fd, SEED + 5202, 0, 1)[0]
    si = to_ints(s.reshape(1, 4), p)[0]
    z = to_mont([(x + si * y) % p for x, y in zip(to_ints(a, p), to_ints(b, p))], p).reshape(count, sh.nvars, 4)
    want = [to_mont([2 * v % p for v in to_ints(O.matrix_prod(fd, sh.mats[1], np.ascontiguousarray(z[k])), p)], p) for k in range(count)]
    da, db = ctx.upload(a), ctx.upload(b)
    dz = ctx.upload(np.zeros((n, 4), dtype=np.uint64))
    prod = ctx.upload(np.zeros((count * m, 4), dtype=np.uint64))
    dbl = ctx.upload(np.zeros((count * m, 4), dtype=np.uint64))
    d = dev[1]
    ctx.sync()
    ctx.field_vec_axpy(fd, da.ptr, s, db.ptr, dz.ptr, n)
    ctx.r1cs_prod_batch(fd, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr, sh.nvars, count, prod.ptr, m)
    ctx.field_vec_op(fd, "double", prod.ptr, 0, dbl.ptr, count * m)
    ctx.sync()
    got = dbl.numpy().reshape(count, m, 4)
    for k in range(count):
        assert (got[k] == want[k]).all(), k


def test_status_codes_and_empties(ctx, oracle):
    """every KG_ERR_BAD_ARG case of the header, the guarded outputs untouched after a sync; count == 0 and m == 0 are KG_OK and write nothing"""
    fd, m, count = 0, 13, 3
    sh, dev, zs, want = case(oracle, ctx, fd, m)
    d = dev[0]
    dz = ctx.upload(np.ascontiguousarray(zs[:count]))
    out = ctx.upload(np.full((count * m + 4, 4), GUARD64, dtype=np.uint64))
    vp = lambda v: C.c_void_p(int(v) if v else 0)

    def call(h=ctx._h, field=fd, rp=d[0].ptr, col=d[1].ptr, val=d[2].ptr, m_=m, z=dz.ptr, zs_=sh.nvars, count_=count, o=out.ptr, os_=m):
        return ctx._lib.kg_r1cs_prod_batch(h, field, vp(rp), vp(col), vp(val), C.c_size_t(m_), vp(z), C.c_size_t(zs_), C.c_size_t(count_), vp(o), C.c_size_t(os_))

    bad = [dict(h=None), dict(field=2), dict(field=-1), dict(rp=0), dict(col=0), dict(val=0), dict(z=0), dict(o=0),
           dict(os_=m - 1), dict(m_=1 << 32, os_=1 << 32), dict(zs_=1 << 60, count_=16), dict(os_=1 << 60, count_=16),
           dict(count_=(1 << 64) - 1)]
    for kw in bad:
        assert call(**kw) == KG_ERR_BAD_ARG, kw
        ctx.sync()
        assert (out.numpy() == GUARD64).all(), kw
    assert call(count_=0) == 0 and call(count_=0, rp=0, col=0, val=0, z=0, o=0) == 0
    assert call(m_=0, os_=0) == 0 and call(m_=0, rp=0, col=0, val=0, z=0, o=0) == 0
    ctx.sync()
    assert (out.numpy() == GUARD64).all()
    assert call() == 0                                     # and the call itself, after all that
    got = out.numpy()
    for b in range(count):
        assert (got[b * m:(b + 1) * m] == want[0][b]).all()
    assert (got[count * m:] == GUARD64).all()
