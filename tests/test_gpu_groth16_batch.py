"""kg_groth16_prove_batch (csrc/groth16_batch.hip): many proofs of one circuit in one call -- one fill kernel, the batched transform, five
batched short MSMs and the assembly of prover.rs:75-92 on the device.  A proof is unique given (CRS, witness, r, s), so every check is
bit equality of all 32 words and all 3 flags: against the oracle's restatement of groth16/src/prover.rs and against
kg_groth16_prove_bn254 (Prover.create_proof) on the same inputs.  Circuits are the chain of oracle.chain_r1cs (l = 2, m_l_1 = m: MSM
lengths m + 2, m and m - 1)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x4B6F676172617368
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD64, GUARD8 = np.uint64(0xDEADBEEFCAFEF00D), np.uint8(0xA5)
KG_ERR_UNSUPPORTED, KG_ERR_CRS = -5, -6


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


_SETUPS = {}


def circuit(O, ctx, m, device=False):
    """(oracle's parameters or None, Prover) of the m-constraint chain; one CRS per m and context.  device=True: the CRS comes from
    kg_groth16_setup_bn254 (tests/test_gpu_groth16.py holds it equal to the oracle's) -- for the sizes checked against single calls only"""
    import kogarashi_amd as K
    key = (id(ctx), m, device)
    if key not in _SETUPS:
        cs = O.chain_r1cs(m, O.f_consts(0)["r"])
        toxic = O.gen_scalars(0, SEED + 701, 0, 5)
        if device:
            from kogarashi_amd.api import groth16_setup
            from test_gpu_groth16 import _FrOps
            full, params = None, groth16_setup(cs.a, cs.b, cs.c, cs.m, cs.l, cs.m_l_1, toxic, _FrOps(O), ctx=ctx)
        else:
            full = O.groth16_params(cs, toxic, threads=8)
            params = dict(full)
            params["vk_g2"] = full["vk_g2"][:2]
        _SETUPS[key] = (full, K.Prover(params, cs.m, cs.l, cs.m_l_1, ctx=ctx))
    return _SETUPS[key]


def make_job(O, m, t0, r, s):
    cs = O.chain_r1cs(m, t0)
    a, b, c = cs.evaluate()
    return cs, (a, b, c, cs.x, cs.w, np.asarray(r, dtype=np.uint64), np.asarray(s, dtype=np.uint64))


def random_jobs(O, m, count, seed):
    t0 = O.gen_scalars(0, seed, 0, count)
    rs = O.gen_scalars(0, seed + 1, 0, 2 * count)
    return [make_job(O, m, t0[b], rs[2 * b], rs[2 * b + 1]) for b in range(count)]


def oracle_proof(O, full, cs, job):
    want = O.groth16_prove(cs, full, job[5], job[6], evals=job[:3])
    return np.concatenate([np.asarray(want[0]).reshape(-1), np.asarray(want[1]).reshape(-1), np.asarray(want[2]).reshape(-1)]).astype(np.uint64), np.asarray(want[3], dtype=np.uint8)


def single_proof(prover, job):
    got = prover.create_proof(*job)
    return np.concatenate([got[0], got[1], got[2]]), np.asarray(got[3], dtype=np.uint8)


def pack(jobs, k, n, stride, fill):
    """field k of every job as one array of count x stride elements; the gaps between two proofs hold `fill`"""
    out = np.full((len(jobs), stride, 4), fill, dtype=np.uint64)
    for b, j in enumerate(jobs):
        out[b, :n] = np.asarray(j[k], dtype=np.uint64).reshape(-1, 4)[:n]
    return out


def raw_call(ctx, crs, ptrs, strides, count, d_out, d_inf):
    a, b, c, x, w, r, s = ptrs
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    return ctx._lib.kg_groth16_prove_batch(ctx._h, C.byref(crs), vp(a), vp(b), vp(c), C.c_size_t(strides[0]), vp(x), C.c_size_t(strides[1]), vp(w),
                                           C.c_size_t(strides[2]), vp(r), vp(s), C.c_size_t(count), vp(d_out), vp(d_inf))


def run_batch(ctx, prover, jobs, extra=(0, 0, 0), fill=0, keep=None):
    """the call on packed uploads into guarded outputs: (proofs[count, 32], flags[count, 3]); nothing is written behind them.  extra: what
    each stride exceeds its length by; keep: a list that receives (host array, device array) of the five inputs"""
    m, l, w_len = prover.m, prover.l, prover.m_l_1
    count = len(jobs)
    strides = (m + extra[0], l + extra[1], w_len + extra[2])
    host = [pack(jobs, 0, m, strides[0], fill), pack(jobs, 1, m, strides[0], fill), pack(jobs, 2, m, strides[0], fill),
            pack(jobs, 3, l, strides[1], fill), pack(jobs, 4, w_len, strides[2], fill)]
    dev = [ctx.upload(h) for h in host]
    dr, ds = ctx.upload(pack(jobs, 5, 1, 1, 0)), ctx.upload(pack(jobs, 6, 1, 1, 0))
    d_out = ctx.upload(np.full((count + 2, 32), GUARD64, dtype=np.uint64))
    d_inf = ctx.upload(np.full(3 * count + 24, GUARD8, dtype=np.uint8))
    ctx.groth16_prove_batch(prover.crs, dev[0].ptr, dev[1].ptr, dev[2].ptr, strides[0], dev[3].ptr, strides[1], dev[4].ptr, strides[2], dr.ptr, ds.ptr,
                            count, d_out.ptr, d_inf.ptr)
    out, inf = d_out.numpy(), d_inf.numpy()
    assert (out[count:] == GUARD64).all() and (inf[3 * count:] == GUARD8).all(), "written beyond count proofs"
    if keep is not None:
        keep.extend(zip(host, dev))
    return out[:count], inf[:3 * count].reshape(count, 3)


def assert_same(got, want, what):
    assert (got[1] == want[1]).all(), (what, "flags", got[1], want[1])
    assert (got[0] == want[0]).all(), (what, "words")


@pytest.mark.parametrize("m", [1, 2, 5, 16, 100, 1024])
def test_sizes_against_oracle_and_single_call(ctx, oracle, m):
    """m = 1: n = 2 and h's MSM is empty; 16: n = m, no padding; 5, 100: padding; three distinct witnesses and (r, s)"""
    O = oracle
    full, prover = circuit(O, ctx, m)
    jobs = random_jobs(O, m, 3, SEED + 710 + m)
    out, inf = run_batch(ctx, prover, [j for _, j in jobs])
    for b, (cs, job) in enumerate(jobs):
        assert_same((out[b], inf[b]), oracle_proof(O, full, cs, job), (m, b, "oracle"))
        assert_same((out[b], inf[b]), single_proof(prover, job), (m, b, "single call"))


def test_upper_edge_of_the_batched_msm(ctx, oracle):
    """m = 2046: the witness MSMs are 2048 pairs long, the longest kg_commit_batch runs batched"""
    import kogarashi_amd.lib as L
    O = oracle
    _, prover = circuit(O, ctx, 2046, device=True)
    assert L.groth16_prove_batch_plan(2046, 2, 2046, 2) == (1, 2)
    jobs = random_jobs(O, 2046, 2, SEED + 730)
    out, inf = run_batch(ctx, prover, [j for _, j in jobs])
    for b, (_, job) in enumerate(jobs):
        assert_same((out[b], inf[b]), single_proof(prover, job), (2046, b))


def test_one_constraint_more_is_unsupported(ctx, oracle):
    """m = 2047 (2049 witness entries): KG_ERR_UNSUPPORTED, plan 0, nothing enqueued -- the arrays are never read, the outputs untouched"""
    import kogarashi_amd.lib as L
    assert L.groth16_prove_batch_plan(2047, 2, 2047, 2) == (0, 0)
    dummy = ctx.upload(np.zeros((64, 4), dtype=np.uint64))
    crs = L.Groth16Crs()
    crs.m, crs.l, crs.m_l_1 = 2047, 2, 2047
    for name in ("h", "l", "a", "b_g1", "b_g2"):
        setattr(crs, "d_" + name, dummy.ptr)
    d_out = ctx.upload(np.full((2, 32), GUARD64, dtype=np.uint64))
    d_inf = ctx.upload(np.full(6, GUARD8, dtype=np.uint8))
    p = dummy.ptr
    assert raw_call(ctx, crs, (p, p, p, p, p, p, p), (2047, 2, 2047), 2, d_out.ptr, d_inf.ptr) == KG_ERR_UNSUPPORTED
    ctx.sync()
    assert (d_out.numpy() == GUARD64).all() and (d_inf.numpy() == GUARD8).all()


_SINGLES = {}


def m5_jobs_and_singles(O, ctx, count):
    """the first `count` of 130 jobs at m = 5 with their single-call proofs, computed once"""
    _, prover = circuit(O, ctx, 5)
    key = id(ctx)
    if key not in _SINGLES:
        jobs = [j for _, j in random_jobs(O, 5, 130, SEED + 740)]
        _SINGLES[key] = (jobs, [single_proof(prover, j) for j in jobs])
    jobs, singles = _SINGLES[key]
    return prover, jobs[:count], singles[:count]


@pytest.mark.parametrize("count", [1, 15, 16, 17, 63, 64, 65, 130])
def test_wave_and_workgroup_edges_of_the_assembly(ctx, oracle, count):
    """The G1 chain kernel runs lane 4 * proof + role in one-wave workgroups: 16 proofs fill a wave, 17 start the next (15 / 16 / 17).  The
    G2 kernel and the finishing kernel run a lane per proof: 64 fill a wave, 65 start the next (63 / 64 / 65); 130 leaves a last wave of 2
    and a last chain wave of 8 lanes; 1 is a lone proof (4 chain lanes)."""
    prover, jobs, singles = m5_jobs_and_singles(oracle, ctx, count)
    out, inf = run_batch(ctx, prover, jobs)
    for b in range(count):
        assert_same((out[b], inf[b]), singles[b], (count, b))


def test_edge_blinding_scalars_in_one_batch(ctx, oracle):
    """(r, s) over {0, 1, p - 1, random}^2: r = 0 or s = 0 makes chain results the identity, r = s = 0 makes C's blinding vanish"""
    O = oracle
    full, prover = circuit(O, ctx, 5)
    one = np.asarray(O.f_consts(0)["r"], dtype=np.uint64)
    rnd = O.gen_scalars(0, SEED + 750, 0, 2)
    vals = [np.zeros(4, dtype=np.uint64), one, np.asarray(O.f_neg(0, one), dtype=np.uint64), None]
    t0 = O.gen_scalars(0, SEED + 751, 0, 16)
    jobs = []
    for i, r in enumerate(vals):
        for k, s in enumerate(vals):
            jobs.append(make_job(O, 5, t0[4 * i + k], rnd[0] if r is None else r, rnd[1] if s is None else s))
    out, inf = run_batch(ctx, prover, [j for _, j in jobs])
    for b, (cs, job) in enumerate(jobs):
        assert_same((out[b], inf[b]), oracle_proof(O, full, cs, job), ("blinding", b))


def test_degenerate_witnesses_among_ordinary_ones(ctx, oracle):
    """t0 = 0: every wire but the constant is zero -- Sl and Sh are the identity, h the zero polynomial; t0 = p - 1: t1 = 0 and on"""
    O = oracle
    full, prover = circuit(O, ctx, 5)
    one = np.asarray(O.f_consts(0)["r"], dtype=np.uint64)
    t = O.gen_scalars(0, SEED + 760, 0, 2)
    rs = O.gen_scalars(0, SEED + 761, 0, 8)
    t0s = [t[0], np.zeros(4, dtype=np.uint64), np.asarray(O.f_neg(0, one), dtype=np.uint64), t[1]]
    jobs = [make_job(O, 5, t0s[b], rs[2 * b], rs[2 * b + 1]) for b in range(4)]
    assert not np.asarray(jobs[1][1][4]).any() and not np.asarray(jobs[2][1][4]).any()
    out, inf = run_batch(ctx, prover, [j for _, j in jobs])
    for b, (cs, job) in enumerate(jobs):
        assert_same((out[b], inf[b]), oracle_proof(O, full, cs, job), ("degenerate", b))


def test_strides_with_garbage_between_the_proofs(ctx, oracle):
    """every stride larger than its length, the gaps filled with a non-canonical value (2^64 - 1 in every word): exact, and the five input
    arrays are byte-identical after the call"""
    O = oracle
    _, prover = circuit(O, ctx, 5)
    jobs = [j for _, j in random_jobs(O, 5, 5, SEED + 770)]
    keep = []
    out, inf = run_batch(ctx, prover, jobs, extra=(3, 2, 5), fill=np.uint64(0xFFFFFFFFFFFFFFFF), keep=keep)
    for b, job in enumerate(jobs):
        assert_same((out[b], inf[b]), single_proof(prover, job), ("strides", b))
    for host, dev in keep:
        assert dev.numpy().tobytes() == host.tobytes()


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import kogarashi_amd as K
import kogarashi_amd.lib as L
from oracle import oracle as O
from test_gpu_groth16_batch import circuit, random_jobs, run_batch, single_proof, assert_same, SEED
m, count = 1024, 16
per = (1 << 20) // ((3 * 1024 + 1026) * 32 + 1024)            # the group rule restated: 1 MiB / scratch bytes per proof
assert per == 7 and L.groth16_prove_batch_plan(m, 2, m, count) == (3, 7)
ctx = K.Context(0)
_, prover = circuit(O, ctx, m, device=True)
jobs = [j for _, j in random_jobs(O, m, count, SEED + 780)]
out, inf = run_batch(ctx, prover, jobs)
for b, job in enumerate(jobs):
    assert_same((out[b], inf[b]), single_proof(prover, job), ("groups", b))
ctx.close()
print("ok")
"""


def test_launch_groups_over_one_scratch():
    """KG_G16_BATCH_MB=1 is read when the library loads: a child process.  m = 1024, count = 16: groups of 7, 7 and 2 proofs"""
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, KG_G16_BATCH_MB="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_stream_order(ctx, oracle):
    """a device-to-device copy of the outputs right behind the batch, no sync between; two batches back to back over the same scratch;
    a single proof and a batched commitment between two batches on one context"""
    O = oracle
    prover, jobs, singles = m5_jobs_and_singles(O, ctx, 20)
    m, l, w_len = prover.m, prover.l, prover.m_l_1

    def uploads(js):
        arrs = [ctx.upload(pack(js, k, n, n, 0)) for k, n in ((0, m), (1, m), (2, m), (3, l), (4, w_len))]
        return arrs + [ctx.upload(pack(js, 5, 1, 1, 0)), ctx.upload(pack(js, 6, 1, 1, 0))]

    def enqueue(d, count):
        d_out, d_inf = ctx.empty((count, 32)), ctx.empty((count, 3), dtype=np.uint8)
        ctx.groth16_prove_batch(prover.crs, d[0].ptr, d[1].ptr, d[2].ptr, m, d[3].ptr, l, d[4].ptr, w_len, d[5].ptr, d[6].ptr, count, d_out.ptr, d_inf.ptr)
        return d_out, d_inf

    def check(out, inf, first, count, what):
        for b in range(count):
            assert_same((out[b], inf[b]), singles[first + b], (what, b))

    d1, d2 = uploads(jobs[:12]), uploads(jobs[12:20])
    ctx.sync()
    o1, f1 = enqueue(d1, 12)
    c_out, c_inf = ctx.empty((12, 32)), ctx.empty((12, 3), dtype=np.uint8)
    ctx.copy_d2d(c_out.ptr, o1.ptr, 12 * 32 * 8)
    ctx.copy_d2d(c_inf.ptr, f1.ptr, 36)
    o2, f2 = enqueue(d2, 8)                                # the second batch reuses the scratch behind the first
    ctx.sync()
    check(c_out.numpy(), c_inf.numpy(), 0, 12, "copy behind the batch")
    check(o2.numpy(), f2.numpy(), 12, 8, "second batch")
    # a single proof and a batched commitment between two batches
    o3, f3 = enqueue(d2, 8)
    assert_same(single_proof(prover, jobs[3]), singles[3], "single proof between batches")
    scal = O.gen_scalars(0, SEED + 790, 0, 4 * (m + 2))
    ds = ctx.upload(scal)
    cxy, cfl = ctx.empty((4, 8)), ctx.empty((4,), dtype=np.uint8)
    ctx.commit_batch(0, prover.crs.d_a, prover.crs.d_a_inf or 0, ds.ptr, m + 2, 4, m + 2, cxy.ptr, cfl.ptr)
    o4, f4 = enqueue(d1, 12)
    ctx.sync()
    check(o3.numpy(), f3.numpy(), 12, 8, "batch before the single proof")
    check(o4.numpy(), f4.numpy(), 0, 12, "batch after the commitment")
    got_xy, got_fl = cxy.numpy(), cfl.numpy()
    for b in range(4):
        xy, fl = ctx.commit(0, prover.crs.d_a, prover.crs.d_a_inf or 0, ds.ptr + 32 * b * (m + 2), m + 2)
        assert fl == got_fl[b] and (xy == got_xy[b]).all()


def test_status_codes(ctx, oracle):
    """a delta flag: KG_ERR_CRS before anything is enqueued, the outputs untouched; count = 0: KG_OK"""
    import kogarashi_amd.lib as L
    O = oracle
    prover, jobs, _ = m5_jobs_and_singles(O, ctx, 2)
    m, l, w_len = prover.m, prover.l, prover.m_l_1
    d = [ctx.upload(pack(jobs, k, n, n, 0)) for k, n in ((0, m), (1, m), (2, m), (3, l), (4, w_len), (5, 1), (6, 1))]
    ptrs = tuple(x.ptr for x in d)
    for flag in ("delta_g1_inf", "delta_g2_inf"):
        crs = L.Groth16Crs.from_buffer_copy(prover.crs)
        setattr(crs, flag, 1)
        d_out = ctx.upload(np.full((2, 32), GUARD64, dtype=np.uint64))
        d_inf = ctx.upload(np.full(6, GUARD8, dtype=np.uint8))
        assert raw_call(ctx, crs, ptrs, (m, l, w_len), 2, d_out.ptr, d_inf.ptr) == KG_ERR_CRS
        ctx.sync()
        assert (d_out.numpy() == GUARD64).all() and (d_inf.numpy() == GUARD8).all()
        with pytest.raises(L.ProverSubVersionCrsAttack):
            ctx.groth16_prove_batch(crs, *ptrs[:3], m, ptrs[3], l, ptrs[4], w_len, ptrs[5], ptrs[6], 2, d_out.ptr, d_inf.ptr)
    assert raw_call(ctx, prover.crs, ptrs, (m, l, w_len), 0, 0, 0) == 0
    assert raw_call(ctx, prover.crs, (0,) * 7, (m, l, w_len), 0, 0, 0) == 0
    out, inf = prover.create_proofs_batch([])
    assert out.shape == (0, 32) and inf.shape == (0, 3)


def test_create_proofs_batch(ctx, oracle):
    """the Python entry: packed uploads, (count, 32) and (count, 3) back"""
    prover, jobs, singles = m5_jobs_and_singles(oracle, ctx, 6)
    out, inf = prover.create_proofs_batch(jobs)
    assert out.shape == (6, 32) and inf.shape == (6, 3)
    for b in range(6):
        assert_same((out[b], inf[b]), singles[b], ("create_proofs_batch", b))
