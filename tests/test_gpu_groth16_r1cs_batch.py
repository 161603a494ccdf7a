"""kg_groth16_prove_r1cs_batch (csrc/groth16_batch.hip): many proofs of one circuit from the witnesses alone -- the fill kernel builds
z = x || w, three batched CSR products (kg_r1cs_prod_batch's kernels) write A z, B z, C z of a whole launch group straight into the padded
rows, and from the transforms on it is kg_groth16_prove_batch.  A proof is unique given (CRS, witness, r, s), so every check is bit equality
of all 32 words and all 3 flags: against the oracle, against kg_groth16_prove_r1cs_bn254 (Prover.create_proof_from_witness) and against
kg_groth16_prove_batch fed with cs.evaluate().  Helpers come from tests/test_gpu_groth16_batch.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_groth16_batch import (GUARD8, GUARD64, KG_ERR_CRS, KG_ERR_UNSUPPORTED, ROOT, SEED, assert_same, circuit, oracle_proof, pack, random_jobs,
                                    run_batch)

pytestmark = pytest.mark.gpu
KG_ERR_BAD_ARG = -2
GARBAGE = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def chain_prover(O, ctx, m, device=False):
    """circuit() of the batch tests with the chain's matrices attached (they do not depend on the witness)"""
    full, prover = circuit(O, ctx, m, device=device)
    if not hasattr(prover, "_cs"):
        cs = O.chain_r1cs(m, O.f_consts(0)["r"])
        prover.attach_constraint_system(cs.a, cs.b, cs.c)
    return full, prover


def csr_ptrs(prover):
    return [tuple(d.ptr for d in trip) for trip in prover._cs]


def single_from_witness(prover, job):
    got = prover.create_proof_from_witness(job[3], job[4], job[5], job[6])
    return np.concatenate([got[0], got[1], got[2]]), np.asarray(got[3], dtype=np.uint8)


def uploads(ctx, prover, jobs, extra=(0, 0), fill=0):
    """(host arrays, device arrays, strides) of x, w, r, s packed; extra: what the strides of x and w exceed their lengths by"""
    strides = (prover.l + extra[0], prover.m_l_1 + extra[1])
    host = [pack(jobs, 3, prover.l, strides[0], fill), pack(jobs, 4, prover.m_l_1, strides[1], fill), pack(jobs, 5, 1, 1, 0), pack(jobs, 6, 1, 1, 0)]
    return host, [ctx.upload(h) for h in host], strides


def enqueue(ctx, prover, dev, strides, count):
    """the call into guarded outputs, not synchronised"""
    d_out = ctx.upload(np.full((count + 2, 32), GUARD64, dtype=np.uint64))
    d_inf = ctx.upload(np.full(3 * count + 24, GUARD8, dtype=np.uint8))
    a, b, c = csr_ptrs(prover)
    ctx.groth16_prove_r1cs_batch(prover.crs, a, b, c, dev[0].ptr, strides[0], dev[1].ptr, strides[1], dev[2].ptr, dev[3].ptr, count, d_out.ptr, d_inf.ptr)
    return d_out, d_inf


def collect(d_out, d_inf, count):
    out, inf = d_out.numpy(), d_inf.numpy()
    assert (out[count:] == GUARD64).all() and (inf[3 * count:] == GUARD8).all(), "written beyond count proofs"
    return out[:count], inf[:3 * count].reshape(count, 3)


def run_r1cs_batch(ctx, prover, jobs, extra=(0, 0), fill=0, keep=None):
    host, dev, strides = uploads(ctx, prover, jobs, extra, fill)
    out = collect(*enqueue(ctx, prover, dev, strides, len(jobs)), len(jobs))
    if keep is not None:
        keep.extend(zip(host, dev))
    return out


@pytest.mark.parametrize("m", [1, 5, 16, 100])
def test_chain_against_oracle_single_call_and_evaluation_batch(ctx, oracle, m):
    """m = 1: n = 2, one row and an empty h; 16: no padding; 5, 100: the products leave padded rows behind them"""
    O = oracle
    full, prover = chain_prover(O, ctx, m)
    jobs = random_jobs(O, m, 3, SEED + 810 + m)
    out, inf = run_r1cs_batch(ctx, prover, [j for _, j in jobs])
    ev_out, ev_inf = run_batch(ctx, prover, [j for _, j in jobs])
    for b, (cs, job) in enumerate(jobs):
        assert_same((out[b], inf[b]), oracle_proof(O, full, cs, job), (m, b, "oracle"))
        assert_same((out[b], inf[b]), single_from_witness(prover, job), (m, b, "kg_groth16_prove_r1cs_bn254"))
        assert_same((out[b], inf[b]), (ev_out[b], ev_inf[b]), (m, b, "kg_groth16_prove_batch on cs.evaluate()"))


def test_upper_edge_of_the_batched_msm(ctx, oracle):
    """m = 2046: the witness MSMs are 2048 pairs long, the longest the batch accepts; device CRS, against the single R1CS call"""
    O = oracle
    _, prover = chain_prover(O, ctx, 2046, device=True)
    jobs = [j for _, j in random_jobs(O, 2046, 2, SEED + 830)]
    out, inf = run_r1cs_batch(ctx, prover, jobs)
    for b, job in enumerate(jobs):
        assert_same((out[b], inf[b]), single_from_witness(prover, job), (2046, b))


def raw_call(ctx, crs, mats, x, xs, w, ws, r, s, count, d_out, d_inf):
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    ref = lambda v: C.byref(v) if v is not None else None
    return ctx._lib.kg_groth16_prove_r1cs_batch(ctx._h, C.byref(crs), ref(mats[0]), ref(mats[1]), ref(mats[2]), vp(x), C.c_size_t(xs), vp(w), C.c_size_t(ws),
                                                vp(r), vp(s), C.c_size_t(count), vp(d_out), vp(d_inf))


def test_one_constraint_more_is_unsupported(ctx):
    """m = 2047 (2049 witness entries): KG_ERR_UNSUPPORTED before anything is enqueued -- nothing is read, the outputs are untouched"""
    import kogarashi_amd.lib as L
    dummy = ctx.upload(np.zeros((64, 4), dtype=np.uint64))
    crs = L.Groth16Crs()
    crs.m, crs.l, crs.m_l_1 = 2047, 2, 2047
    for name in ("h", "l", "a", "b_g1", "b_g2"):
        setattr(crs, "d_" + name, dummy.ptr)
    p = dummy.ptr
    mats = [L.Csr(p, p, p) for _ in range(3)]
    d_out = ctx.upload(np.full((2, 32), GUARD64, dtype=np.uint64))
    d_inf = ctx.upload(np.full(6, GUARD8, dtype=np.uint8))
    assert raw_call(ctx, crs, mats, p, 2, p, 2047, p, p, 2, d_out.ptr, d_inf.ptr) == KG_ERR_UNSUPPORTED
    ctx.sync()
    assert (d_out.numpy() == GUARD64).all() and (d_inf.numpy() == GUARD8).all()


def test_circuit_with_long_rows_through_the_prover(ctx, oracle):
    """The m = 300 shape of tests/r1cs_cases.py over Fr as the "circuit" (l = 4, m_l_1 = nvars - 4): rows of 49 .. 254 entries and one of
    5000, so the wave and the huge-row kernels write into padded rows of stride n = 512 -- the only case that does.  CRS from the device
    setup, random x || w: the witness is unsatisfied, the prover does not care and bit identity with kg_groth16_prove_r1cs_bn254 holds."""
    import kogarashi_amd as K
    from kogarashi_amd.api import groth16_setup
    from r1cs_cases import Shape
    from test_gpu_groth16 import _FrOps
    O, m, l, count = oracle, 300, 4, 3
    sh = Shape(O, 0, m)
    m_l_1 = sh.nvars - l
    a, b, c = sh.mats
    params = groth16_setup(a, b, c, m, l, m_l_1, O.gen_scalars(0, SEED + 841, 0, 5), _FrOps(O), ctx=ctx)
    prover = K.Prover(params, m, l, m_l_1, ctx=ctx)
    prover.attach_constraint_system(a, b, c)
    z = np.ascontiguousarray(O.gen_scalars(0, SEED + 842, 0, count * sh.nvars)).reshape(count, sh.nvars, 4)
    rs = O.gen_scalars(0, SEED + 843, 0, 2 * count)
    jobs = [(None, None, None, z[k, :l], z[k, l:], rs[2 * k], rs[2 * k + 1]) for k in range(count)]
    out, inf = run_r1cs_batch(ctx, prover, jobs)
    for k, job in enumerate(jobs):
        assert_same((out[k], inf[k]), single_from_witness(prover, job), ("long rows", k))


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import kogarashi_amd as K
import kogarashi_amd.lib as L
from oracle import oracle as O
from test_gpu_groth16_batch import random_jobs, assert_same, SEED
from test_gpu_groth16_r1cs_batch import chain_prover, run_r1cs_batch, single_from_witness
m, count = 1024, 16
assert L.groth16_prove_batch_plan(m, 2, m, count) == (3, 7)      # the plan answers for both entries: groups of 7, 7 and 2 proofs
ctx = K.Context(0)
_, prover = chain_prover(O, ctx, m, device=True)
jobs = [j for _, j in random_jobs(O, m, count, SEED + 880)]
out, inf = run_r1cs_batch(ctx, prover, jobs)
for b, job in enumerate(jobs):
    assert_same((out[b], inf[b]), single_from_witness(prover, job), ("groups", b))
ctx.close()
print("ok")
"""


def test_launch_groups_over_one_scratch():
    """KG_G16_BATCH_MB=1 is read when the library loads: a child process.  m = 1024, count = 16: three groups reuse the scratch's z block and
    the work lists"""
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, KG_G16_BATCH_MB="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


_SINGLES = {}


def m5_jobs_and_singles(O, ctx, count):
    _, prover = chain_prover(O, ctx, 5)
    if id(ctx) not in _SINGLES:
        jobs = [j for _, j in random_jobs(O, 5, 20, SEED + 840)]
        _SINGLES[id(ctx)] = (jobs, [single_from_witness(prover, j) for j in jobs])
    jobs, singles = _SINGLES[id(ctx)]
    return prover, jobs[:count], singles[:count]


def test_strides_with_garbage_and_stream_order(ctx, oracle):
    """strides of x and w larger than their lengths with a non-canonical value in the gaps, guard values behind the proofs, the inputs
    byte-identical afterwards; then two batches enqueued back to back over the same scratch and work lists, one sync"""
    prover, jobs, singles = m5_jobs_and_singles(oracle, ctx, 20)
    keep = []
    out, inf = run_r1cs_batch(ctx, prover, jobs[:5], extra=(2, 5), fill=GARBAGE, keep=keep)
    for b in range(5):
        assert_same((out[b], inf[b]), singles[b], ("strides", b))
    for host, dev in keep:
        assert dev.numpy().tobytes() == host.tobytes()
    _, d1, s1 = uploads(ctx, prover, jobs[:12], extra=(1, 3), fill=GARBAGE)
    _, d2, s2 = uploads(ctx, prover, jobs[12:20])
    ctx.sync()
    o1 = enqueue(ctx, prover, d1, s1, 12)
    o2 = enqueue(ctx, prover, d2, s2, 8)
    ctx.sync()
    out1, inf1 = collect(*o1, 12)
    out2, inf2 = collect(*o2, 8)
    for b in range(12):
        assert_same((out1[b], inf1[b]), singles[b], ("first batch", b))
    for b in range(8):
        assert_same((out2[b], inf2[b]), singles[12 + b], ("second batch", b))


def test_status_codes(ctx, oracle):
    """a null kg_csr, a null member array, a stride shorter than its length: KG_ERR_BAD_ARG; a delta flag: KG_ERR_CRS; all before anything is
    enqueued, the outputs untouched; count == 0: KG_OK"""
    import kogarashi_amd.lib as L
    prover, jobs, _ = m5_jobs_and_singles(oracle, ctx, 2)
    _, d, (xs, ws) = uploads(ctx, prover, jobs)
    x, w, r, s = (v.ptr for v in d)
    full = [L.Csr(*t) for t in csr_ptrs(prover)]
    d_out = ctx.upload(np.full((2, 32), GUARD64, dtype=np.uint64))
    d_inf = ctx.upload(np.full(6, GUARD8, dtype=np.uint8))

    def untouched():
        ctx.sync()
        return (d_out.numpy() == GUARD64).all() and (d_inf.numpy() == GUARD8).all()

    for which in range(3):
        mats = list(full)
        mats[which] = None
        assert raw_call(ctx, prover.crs, mats, x, xs, w, ws, r, s, 2, d_out.ptr, d_inf.ptr) == KG_ERR_BAD_ARG and untouched()
        for member in range(3):
            t = list(csr_ptrs(prover)[which])
            t[member] = None
            mats[which] = L.Csr(*t)
            assert raw_call(ctx, prover.crs, mats, x, xs, w, ws, r, s, 2, d_out.ptr, d_inf.ptr) == KG_ERR_BAD_ARG and untouched()
    assert raw_call(ctx, prover.crs, full, x, xs - 1, w, ws, r, s, 2, d_out.ptr, d_inf.ptr) == KG_ERR_BAD_ARG and untouched()
    assert raw_call(ctx, prover.crs, full, x, xs, w, ws - 1, r, s, 2, d_out.ptr, d_inf.ptr) == KG_ERR_BAD_ARG and untouched()
    for flag in ("delta_g1_inf", "delta_g2_inf"):
        crs = L.Groth16Crs.from_buffer_copy(prover.crs)
        setattr(crs, flag, 1)
        assert raw_call(ctx, crs, full, x, xs, w, ws, r, s, 2, d_out.ptr, d_inf.ptr) == KG_ERR_CRS and untouched()
        with pytest.raises(L.ProverSubVersionCrsAttack):
            ctx.groth16_prove_r1cs_batch(crs, *csr_ptrs(prover), x, xs, w, ws, r, s, 2, d_out.ptr, d_inf.ptr)
    assert raw_call(ctx, prover.crs, full, x, xs, w, ws, r, s, 0, 0, 0) == 0
    assert raw_call(ctx, prover.crs, [None, None, None], 0, xs, 0, ws, 0, 0, 0, 0, 0) == 0
    assert untouched()


def test_create_proofs_batch_from_witness(ctx, oracle):
    """the Python entry: jobs are (x, w, r, s); an empty list gives empty arrays, a list of 4 the four single proofs"""
    prover, jobs, singles = m5_jobs_and_singles(oracle, ctx, 4)
    out, inf = prover.create_proofs_batch_from_witness([])
    assert out.shape == (0, 32) and inf.shape == (0, 3)
    out, inf = prover.create_proofs_batch_from_witness([j[3:] for j in jobs])
    assert out.shape == (4, 32) and inf.shape == (4, 3)
    for b in range(4):
        assert_same((out[b], inf[b]), singles[b], ("create_proofs_batch_from_witness", b))
