"""kg_commit_batch (csrc/msm_small_batch.hip): many short MSMs of one length against one base array in one call, the points finished and
normalised on the device.  Every point is compared with the oracle's msm_curve_addition -> to_affine (groth16/src/msm.rs:6-48) AND, bit for
bit, with kg_commit of the same vector: every length 1 .. 40, the rows of the shape table at their edges on all three curves (unsplit and
split windows), vectors of different kinds inside one batch, forced shapes, both other endomorphism settings (child processes), a batch one
vector longer than a launch group, the lengths that fall back to single calls, and the outputs consumed in stream order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import primitive_cases as PC
from test_gpu_parity import SEED, edge_mix

pytestmark = pytest.mark.gpu
SMALL_DEFAULT = 32768       # KG_SMALL_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV = {0: "g1", 1: "gk", 2: "g2"}
GUARD64, GUARD8 = np.uint64(0xDEADBEEFCAFEF00D), np.uint8(0xA5)


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def identity_words(O, curve):
    """(0, 1) in the ABI form: what kg_fixed_base_mul and kg_commit write for the identity"""
    e = 8 if curve == 2 else 4
    out = np.zeros(2 * e, dtype=np.uint64)
    out[e:e + 4] = O.f_consts(0 if curve == 1 else 1)["r"]
    return out


def want_point(O, curve, bases, scal, inf):
    xy, fl = O.to_affine(CV[curve], O.msm(CV[curve], bases, scal, inf, threads=4))
    return None if fl else np.asarray(xy, dtype=np.uint64)


def inputs(O, curve, sfd, n, count, stride, seed):
    """n bases with the edge mix (an identity base, a zero scalar, repeated points, scalars 1 and -1) and count * stride scalars: vector b is
    the n scalars from element b * stride; vector 0 carries the edge mix's scalars"""
    bases, s0, inf = edge_mix(O, CV[curve], curve, sfd, n, seed)
    scal = O.gen_scalars(sfd, seed + 7, 0, count * stride)
    scal[:n] = s0
    return bases, scal, inf


def run_batch(ctx, curve, db, di, ds, n, count, stride):
    """the call into guarded output arrays: (points, flags) of the count vectors; nothing is written behind them"""
    w = 16 if curve == 2 else 8
    dxy = ctx.upload(np.full((count + 2, w), GUARD64, dtype=np.uint64))
    dfl = ctx.upload(np.full(count + 24, GUARD8, dtype=np.uint8))
    ctx.commit_batch(curve, db, di, ds, n, count, stride, dxy.ptr, dfl.ptr)
    xy, fl = dxy.numpy(), dfl.numpy()
    assert (xy[count:] == GUARD64).all() and (fl[count:] == GUARD8).all(), "written beyond count points"
    return xy[:count], fl[:count]


def check_vector(O, ctx, curve, got_xy, got_fl, want, db, di, ds_vec, n, what):
    """one point of a batch against the oracle's point and against kg_commit of the same vector"""
    if want is None:
        assert got_fl == 1 and (got_xy == identity_words(O, curve)).all(), what
    else:
        assert got_fl == 0 and (got_xy == want).all(), what
    cxy, cfl = ctx.commit(curve, db, di, ds_vec, n)
    assert cfl == got_fl and (cxy == got_xy).all(), what


def test_every_length_up_to_40(ctx, oracle):
    """n = 1 .. 40, three vectors that are different slices of one scalar array (stride n + 3), on G1 with the edge mix (an identity base, a
    zero scalar, repeated points, scalars 1 and -1)"""
    O = oracle
    bases, scal, inf = inputs(O, 0, 0, 40, 3, 43, SEED + 1200)
    db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(inf)
    for n in range(1, 41):
        stride = n + 3
        xy, fl = run_batch(ctx, 0, db.ptr, di.ptr, ds.ptr, n, 3, stride)
        for b in range(3):
            v = scal[b * stride:b * stride + n]
            check_vector(O, ctx, 0, xy[b], fl[b], want_point(O, 0, bases[:n], v, inf[:n]), db.ptr, di.ptr, ds.ptr + 32 * b * stride, n, (n, b))


@pytest.mark.parametrize("curve,sfd", [(0, 0), (1, 1)])
@pytest.mark.parametrize("n", [384, 385, 1536, 1537, 2048])
def test_plan_rows_at_their_edges_g1_grumpkin(ctx, oracle, curve, sfd, n):
    """both sides of every row of msm_small_plan up to the longest batched input: one launch per group (NB = 1) up to 384 pairs, split
    windows (the batched combine shell) beyond; count 1, 2 and 5"""
    O = oracle
    stride = n + 1
    bases, scal, inf = inputs(O, curve, sfd, n, 5, stride, SEED + 1300 + n + curve)
    db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(inf)
    want = [want_point(O, curve, bases, scal[b * stride:b * stride + n], inf) for b in range(5)]
    for count in (1, 2, 5):
        xy, fl = run_batch(ctx, curve, db.ptr, di.ptr, ds.ptr, n, count, stride)
        for b in range(count):
            check_vector(O, ctx, curve, xy[b], fl[b], want[b], db.ptr, di.ptr, ds.ptr + 32 * b * stride, n, (n, count, b))


@pytest.mark.parametrize("n", [48, 49, 160, 161, 600])
def test_plan_rows_at_their_edges_g2(ctx, oracle, n):
    """G2's rows: NB = 1 up to 48 pairs, 2 up to 160, 4 beyond; bases are generator multiples from kg_fixed_base_mul with one identity"""
    from test_gpu_large import _g2_bases
    O = oracle
    stride = n + 2
    dxy, dinf = _g2_bases(ctx, O, n, SEED + 1400 + n)
    bases, inf = dxy.numpy(), dinf.numpy()
    scal = O.gen_scalars(0, SEED + 1401 + n, 0, 5 * stride)
    scal[3] = 0
    ds = ctx.upload(scal)
    want = [want_point(O, 2, bases, scal[b * stride:b * stride + n], inf) for b in range(5)]
    for count in (1, 2, 5):
        xy, fl = run_batch(ctx, 2, dxy.ptr, dinf.ptr, ds.ptr, n, count, stride)
        for b in range(count):
            check_vector(O, ctx, 2, xy[b], fl[b], want[b], dxy.ptr, dinf.ptr, ds.ptr + 32 * b * stride, n, (n, count, b))


def test_vectors_of_different_kinds_in_one_batch(ctx, oracle, pyoracle):
    """an all-zero vector, one non-zero scalar, the scalars 1, 2, 2^126, 2^127, r - 1 and the rounding boundaries of the endomorphism split,
    P and -P under one scalar, one scalar over one base repeated, and a random vector -- in ONE batch; then the same batch with every base
    flagged the identity, and without a flag array"""
    O = oracle
    r = pyoracle.G1.n
    lam = PC.glv_module().consts(pyoracle.G1)[0]
    _, bound, _ = PC.glv_edge_scalars(0, r, lam, count_random=0)
    special = [1, 2, 1 << 126, 1 << 127, r - 1] + bound
    n = len(special)
    assert n >= 16
    to_mont = lambda k: O.f_to_mont(0, np.array([(k >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64))
    bases = O.gen_bases(0, SEED + 1500, 0, n)
    bases[1] = bases[0]; bases[1, 4:] = O.f_neg(1, bases[0, 4:])          # -P beside P
    bases[4:13] = bases[4]                                                # one base repeated
    inf = np.zeros(n, dtype=np.uint8)
    inf[14] = 1
    k = O.gen_scalars(0, SEED + 1501, 0, 1)[0]
    vec = np.zeros((6, n, 4), dtype=np.uint64)
    vec[1, n - 2] = k                                                     # one non-zero scalar
    vec[2] = np.stack([to_mont(s) for s in special])
    vec[3, 0] = k; vec[3, 1] = k                                          # k P + k (-P): the identity
    vec[4, 4:13] = k                                                      # one scalar repeated over one base repeated
    vec[5] = O.gen_scalars(0, SEED + 1502, 0, n)
    db, ds, di = ctx.upload(bases), ctx.upload(vec), ctx.upload(inf)
    all_inf = ctx.upload(np.ones(n, dtype=np.uint8))
    for flags, dflags in ((inf, di.ptr), (np.ones(n, dtype=np.uint8), all_inf.ptr), (None, 0)):
        xy, fl = run_batch(ctx, 0, db.ptr, dflags, ds.ptr, n, 6, n)
        want = [want_point(O, 0, bases, vec[b], flags) for b in range(6)]
        if flags is inf:
            assert want[0] is None and want[3] is None and all(want[b] is not None for b in (1, 2, 4, 5))
        if flags is not None and flags.all():
            assert all(w is None for w in want)
        for b in range(6):
            check_vector(O, ctx, 0, xy[b], fl[b], want[b], db.ptr, dflags, ds.ptr + 32 * b * n, n, (b, None if flags is None else int(flags.sum())))
    # empty vectors: every output is the identity; an empty batch: nothing is written
    xy, fl = run_batch(ctx, 0, db.ptr, di.ptr, ds.ptr, 0, 3, 5)
    assert (fl == 1).all() and (xy == identity_words(O, 0)).all()
    run_batch(ctx, 0, db.ptr, di.ptr, ds.ptr, n, 0, n)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_empty_vectors_are_identities_on_every_curve(ctx, oracle, curve):
    """n = 0 reads neither bases nor scalars: the finish kernel alone runs and writes (0, 1) with flag 1 for every vector -- the identity
    branch of the affine writer every kernel shares (common.h put_affine_abi), once per coordinate field"""
    xy, fl = run_batch(ctx, curve, 0, 0, 0, 0, 3, 0)
    assert (fl == 1).all() and (xy == identity_words(oracle, curve)).all()


@pytest.mark.parametrize("c,r", [(2, 0), (3, 2), (5, 1), (6, 0), (8, 3)])
def test_forced_shapes(ctx, oracle, c, r):
    """kg_msm_set_small applies to the batch as it does to kg_commit: window widths that do not divide the halves' 128 bits, one bucket per
    workgroup, 32 workgroups per window (6, 0), sixteen ranges (8, 3)"""
    O = oracle
    for n in (37, 1000):
        stride = n + 5
        bases, scal, inf = inputs(O, 0, 0, n, 3, stride, SEED + 1600 + n)
        db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(inf)
        want = [want_point(O, 0, bases, scal[b * stride:b * stride + n], inf) for b in range(3)]
        ctx.set_msm_small(SMALL_DEFAULT, c, r)
        try:
            xy, fl = run_batch(ctx, 0, db.ptr, di.ptr, ds.ptr, n, 3, stride)
            for b in range(3):
                check_vector(O, ctx, 0, xy[b], fl[b], want[b], db.ptr, di.ptr, ds.ptr + 32 * b * stride, n, (n, c, r, b))
        finally:
            ctx.set_msm_small(SMALL_DEFAULT, 0, -1)


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import kogarashi_amd as K
from oracle import oracle as O
from test_gpu_msm_batch import inputs, run_batch, check_vector, want_point
ctx = K.Context(0)
for curve, sfd, lens in ((0, 0, (37, 1000, 2048)), (1, 1, (385,))):
    for n in lens:
        stride = n + 2
        bases, scal, inf = inputs(O, curve, sfd, n, 3, stride, 7100 + n)
        db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(inf)
        xy, fl = run_batch(ctx, curve, db.ptr, di.ptr, ds.ptr, n, 3, stride)
        for b in range(3):
            check_vector(O, ctx, curve, xy[b], fl[b], want_point(O, curve, bases, scal[b * stride:b * stride + n], inf), db.ptr, di.ptr,
                         ds.ptr + 32 * b * stride, n, (curve, n, b))
ctx.close()
print("ok")
"""


@pytest.mark.parametrize("glv", ["0", "2"])
def test_other_endomorphism_settings(glv):
    """KG_SMALL_GLV=0 (never: 255-bit scalars, twice the windows) and 2 (wherever the index field allows) are read when the library loads:
    a child process each, which starts the GPU once"""
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, KG_SMALL_GLV=glv), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (glv, r.stdout[-500:], r.stderr[-2000:])


def test_one_vector_more_than_a_launch_group(ctx, oracle):
    """count = per_launch + 1 at n = 2: two groups over the same scratch, the second one vector long; vector b is row b mod 5 of five
    distinct vectors"""
    import kogarashi_amd.lib as L
    O = oracle
    n = 2
    groups1, per = L.commit_batch_plan(0, n, 1)
    assert groups1 == 1 and 1 <= per <= 65535
    count = per + 1
    assert L.commit_batch_plan(0, n, count) == (2, per) and L.commit_batch_plan(0, n, per) == (1, per)
    bases = O.gen_bases(0, SEED + 1700, 0, n)
    rows = O.gen_scalars(0, SEED + 1701, 0, 5 * n).reshape(5, n, 4)
    rows[3, 1] = 0
    scal = np.ascontiguousarray(rows[np.arange(count) % 5])
    db, ds = ctx.upload(bases), ctx.upload(scal)
    want = [want_point(O, 0, bases, rows[j], None) for j in range(5)]
    xy, fl = run_batch(ctx, 0, db.ptr, 0, ds.ptr, n, count, n)
    assert not fl.any()
    for j in range(5):
        assert (xy[j::5] == want[j]).all(), j
        cxy, cfl = ctx.commit(0, db.ptr, 0, ds.ptr + 32 * j * n, n)
        assert not cfl and (cxy == want[j]).all()


@pytest.mark.parametrize("n", [2049, 3000])
def test_lengths_beyond_the_batched_kernels_fall_back_to_single_calls(ctx, oracle, n):
    import kogarashi_amd.lib as L
    O = oracle
    assert L.commit_batch_plan(0, n, 2) == (0, 0)
    stride = n + 1
    bases, scal, inf = inputs(O, 0, 0, n, 2, stride, SEED + 1800 + n)
    db, ds, di = ctx.upload(bases), ctx.upload(scal), ctx.upload(inf)
    xy, fl = run_batch(ctx, 0, db.ptr, di.ptr, ds.ptr, n, 2, stride)
    for b in range(2):
        check_vector(O, ctx, 0, xy[b], fl[b], want_point(O, 0, bases, scal[b * stride:b * stride + n], inf), db.ptr, di.ptr, ds.ptr + 32 * b * stride, n, (n, b))


@pytest.mark.parametrize("curve", [0, 2])
def test_outputs_are_valid_in_stream_order(ctx, oracle, curve):
    """kg_points_check enqueued right behind the batch, on the batch's own output arrays: every finite point is on the curve and in the
    subgroup; and two batches in a row into different outputs without a sync between them (the second reuses the scratch behind the first)"""
    import kogarashi_amd as K
    O = oracle
    n, count, w = (300, 9, 8) if curve == 0 else (100, 6, 16)
    if curve == 0:
        bases, scal, inf = inputs(O, 0, 0, n, 2 * count, n, SEED + 1900)
        db, di = ctx.upload(bases), ctx.upload(inf)
    else:
        from test_gpu_large import _g2_bases
        db, di = _g2_bases(ctx, O, n, SEED + 1901)
        bases, inf = db.numpy(), di.numpy()
        scal = O.gen_scalars(0, SEED + 1902, 0, 2 * count * n)
    scal[:n] = 0                                                          # vector 0: the identity (skipped by the check through its flag)
    ds = ctx.upload(scal)
    oxy = [ctx.upload(np.zeros((count, w), dtype=np.uint64)) for _ in range(2)]
    ofl = [ctx.upload(np.full(count, GUARD8, dtype=np.uint8)) for _ in range(2)]
    ctx.sync()
    ctx.commit_batch(curve, db.ptr, di.ptr, ds.ptr, n, count, n, oxy[0].ptr, ofl[0].ptr)
    ctx.commit_batch(curve, db.ptr, di.ptr, ds.ptr + 32 * count * n, n, count, n, oxy[1].ptr, ofl[1].ptr)
    for j in range(2):
        bad, first = ctx.points_check(curve, oxy[j].ptr, ofl[j].ptr, count, K.KG_CHECK_CURVE | K.KG_CHECK_SUBGROUP)
        assert (bad, first) == (0, count), (j, bad, first)
    for j in range(2):
        xy, fl = oxy[j].numpy(), ofl[j].numpy()
        assert fl[0] == (1 if j == 0 else 0)
        for b in range(count):
            v = scal[(j * count + b) * n:(j * count + b + 1) * n]
            check_vector(O, ctx, curve, xy[b], fl[b], want_point(O, curve, bases, v, inf), db.ptr, di.ptr, ds.ptr + 32 * (j * count + b) * n, n, (curve, j, b))
