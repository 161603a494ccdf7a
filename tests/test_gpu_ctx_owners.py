"""What a context owns (kogarashi_amd/csrc/common.h: every work space a GrowBuf, every event and queue an owner of its handle): the memory
comes back when the context goes, and every work space can grow while earlier work that uses the old block is still queued."""
import gc

import numpy as np
import pytest

from test_gpu_parity import SEED, aff, gpu_aff

pytestmark = pytest.mark.gpu

MIB = 1 << 20
PARENT_DRIFT = 152 * MIB    # what the parent commit drifts in test_context_cycles_give_their_memory_back (see there)


@pytest.fixture(scope="module")
def proof_1024(oracle):
    """the m = 1024 chain circuit, its CRS, (r, s) and the oracle's proof: made once, read by both tests"""
    O = oracle
    cs = O.chain_r1cs(1024, O.gen_scalars(0, SEED + 1700, 0, 1)[0])
    params = O.groth16_params(cs, O.gen_scalars(0, SEED + 1701, 0, 5), threads=8)
    r, s = O.gen_scalars(0, SEED + 1702, 0, 2)
    want = O.groth16_prove(cs, params, r, s)
    params["vk_g2"] = params["vk_g2"][:2]
    return cs, params, r, s, want


def _one_cycle(K, ctx, bases, proof):
    """every owned resource of a context touched once; everything the cycle allocates through the context is released before it returns"""
    n = 1 << 18
    cs, params, r, s, _ = proof
    bases_ptr = bases.data_ptr()
    ds = ctx.empty((n, 4))
    ctx.gen_bases(0, SEED + 1710, 0, n, bases_ptr)
    ctx.gen_scalars(0, SEED + 1711, 0, n, ds.ptr)
    ctx.msm(0, bases_ptr, 0, ds.ptr, n)                                   # ws_sort, ws_run, ws_pb, the queues and their events
    hb, hs = bases.cpu().numpy().view(np.uint64).reshape(n, 8), ds.numpy()      # (the blocking MSM has drained the generator kernels)
    ctx.msm_host(0, hb, None, hs, n)                                      # up_buf, the upload queue
    dv = ctx.upload(hs)
    ctx.ntt(dv.ptr, 18, False, False)                                     # ws2, twiddle tables
    prover = K.Prover(params, cs.m, cs.l, cs.m_l_1, ctx=ctx)
    prover.attach_constraint_system(cs.a, cs.b, cs.c)
    prover.create_proof_from_witness(cs.x, cs.w, r, s)                    # ws3, ws_vec, fork / join events
    oxy, oinf = ctx.empty((8, 8)), ctx.empty((8,), dtype=np.uint8)
    ctx.commit_batch(0, bases_ptr, 0, ds.ptr, 64, 8, 64, oxy.ptr, oinf.ptr)      # ws_small_batch
    fxy, finf = ctx.empty((4096, 8)), ctx.empty((4096,), dtype=np.uint8)
    ctx.fixed_base_mul(0, ds.ptr, 4096, fxy.ptr, finf.ptr)                # the generator table and fb_tmp
    ctx.bases_register(0, bases_ptr, 0, n)                                # both resident forms, left registered
    ctx.bases_precompute(bases_ptr, n)
    ctx.sync()
    del prover


def test_context_cycles_give_their_memory_back(oracle, proof_1024):
    """One warm-up cycle, then four, each on a fresh context: a blocking MSM and a host-array MSM of 2^18 G1 pairs, an NTT of 2^18, a proof
    from the witness with m = 1024, a batched commitment of 8 x 64, 4096 fixed-base multiples, a registered array with its window table
    (left registered), close.  At these sizes every large work space is 8 MiB or more, so one of them lost per cycle is 32 MiB after four.
    The device's free memory after the last cycle is compared with the value after the warm-up; the bound is what the parent commit
    (manual teardown in kg_ctx_destroy) drifts in this same test, PARENT_DRIFT, plus 4 MiB.
    The parent's drift, measured on an MI355X with this test alone in the process: 159383552 bytes = 152.0 MiB, and the same figure with
    the owners.  It is not the library's: run one step per context (four contexts each), no step drifts at all, but the first
    kg_fixed_base_mul of a process takes 152 MiB that stay with the process -- the runtime's scratch memory for that kernel's private
    segment, kept per hardware queue.  A later context's main queue can land on a hardware queue that has none yet, and then the runtime
    allocates it again, once per hardware queue; that happened once in the four cycles of the measured runs.
    (The bases live in a tensor of the caller's, allocated before the warm-up: a block from kg_malloc that outlives its context stays the
    host's, which is not what is measured here.)"""
    import torch
    import kogarashi_amd as K
    bases = torch.empty((1 << 18) * 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def cycle():
        ctx = K.Context(0)
        try:
            _one_cycle(K, ctx, bases, proof_1024)
            gc.collect()                       # the cycle's device arrays go back to the context before it closes
        finally:
            ctx.close()
        return torch.cuda.mem_get_info(0)[0]

    after_warmup = cycle()
    for _ in range(4):
        after_last = cycle()
    drift = after_warmup - after_last
    print(f"free after warm-up {after_warmup / MIB:.1f} MiB, after four more cycles {after_last / MIB:.1f} MiB: drift {drift / MIB:.2f} MiB")
    assert drift <= PARENT_DRIFT + 4 * MIB


def test_every_work_space_grows_under_pending_work(oracle, proof_1024):
    """The buffers test_work_space_growth_with_msms_in_flight does not reach, on one fresh context: each operation small, then at a size
    whose request exceeds the first block (slack included), with the earlier work still queued where the call is asynchronous; every
    result against the oracle."""
    import kogarashi_amd as K
    O = oracle
    ctx = K.Context(0)
    try:
        # NTT 2^10, then 2^14 (ws2): the first transform is still on the stream when the second one grows the buffer
        v = {k: O.gen_scalars(0, SEED + 1720 + k, 0, 1 << k) for k in (10, 14)}
        d = {k: ctx.upload(v[k]) for k in v}
        ctx.ntt(d[10].ptr, 10, False, False)
        ctx.ntt(d[14].ptr, 14, False, False)
        for k in v:
            assert (d[k].numpy() == O.Fft(k).dft(v[k], threads=8)).all(), ("ntt", k)

        # proof from the witness with m = 64, then m = 1024 (ws3, ws_vec)
        cs = O.chain_r1cs(64, O.gen_scalars(0, SEED + 1730, 0, 1)[0])
        params = O.groth16_params(cs, O.gen_scalars(0, SEED + 1731, 0, 5), threads=8)
        r, s = O.gen_scalars(0, SEED + 1732, 0, 2)
        small = (cs, params, r, s, O.groth16_prove(cs, params, r, s))
        params["vk_g2"] = params["vk_g2"][:2]
        for cs, params, r, s, want in (small, proof_1024):
            prover = K.Prover(params, cs.m, cs.l, cs.m_l_1, ctx=ctx)
            prover.attach_constraint_system(cs.a, cs.b, cs.c)
            got = prover.create_proof_from_witness(cs.x, cs.w, r, s)
            assert all((got[i] == want[i]).all() for i in range(4)), ("proof", cs.m)

        # batched commitment of 2, then 64 vectors of 64 scalars (ws_small_batch): asynchronous, read back after both
        n, counts = 64, (2, 64)
        bases = O.gen_bases(0, SEED + 1740, 0, n)
        scal = O.gen_scalars(0, SEED + 1741, 0, counts[1] * n)
        db, ds = ctx.upload(bases), ctx.upload(scal)
        outs = [(ctx.empty((c, 8)), ctx.empty((c,), dtype=np.uint8)) for c in counts]
        for c, (oxy, ofl) in zip(counts, outs):
            ctx.commit_batch(0, db.ptr, 0, ds.ptr, n, c, n, oxy.ptr, ofl.ptr)
        for c, (oxy, ofl) in zip(counts, outs):
            xy, fl = oxy.numpy(), ofl.numpy()
            for b in range(c):
                wxy, winf = O.to_affine("g1", O.msm("g1", bases, scal[b * n:(b + 1) * n], None, threads=4))
                assert fl[b] == winf == 0 and (xy[b] == wxy).all(), ("commit_batch", c, b)

        # fixed-base multiples: 64 (no table yet: the plain kernel), 600 and 4096 (fb_tmp, growing under the 600's two passes)
        k = O.gen_scalars(0, SEED + 1750, 0, 4096)
        dk = ctx.upload(k)
        fb = [(m, ctx.empty((m, 8)), ctx.empty((m,), dtype=np.uint8)) for m in (64, 600, 4096)]
        for m, dxy, dinf in fb:
            ctx.fixed_base_mul(0, dk.ptr, m, dxy.ptr, dinf.ptr)
        want_xy, want_inf = O.fixed_base_mul(0, k)
        for m, dxy, dinf in fb:
            assert (dinf.numpy() == want_inf[:m]).all() and (dxy.numpy() == want_xy[:m]).all(), ("fixed_base_mul", m)

        # host arrays of 3000, then 70000 pairs (up_buf; the second call also leaves the short kernel for the sliced pipeline)
        hb, hs = O.gen_bases(0, SEED + 1760, 0, 70000), O.gen_scalars(0, SEED + 1761, 0, 70000)
        for m in (3000, 70000):
            assert gpu_aff(ctx.msm_host(0, hb[:m], None, hs[:m], m), 4) == aff(O, "g1", O.msm("g1", hb[:m], hs[:m], None, threads=8)), ("msm_host", m)

        # one ticket begun twice with a short shape whose windows split over workgroups (c = 4, r = 1: four bucket ranges per window),
        # at 300 pairs (the plane points alone) and at 3000 (beyond 2048 pairs the converted scalars and the spill space join them:
        # ws_small of the ticket's slot grows), another ticket's MSM pending meanwhile
        ctx.set_msm_small(-2, 4, 1)
        try:
            dhb, dhs = ctx.upload(hb[:3000]), ctx.upload(hs[:3000])
            want = {m: aff(O, "g1", O.msm("g1", hb[:m], hs[:m], None, threads=8)) for m in (300, 3000)}
            ctx.msm_begin(0, dhb.ptr, 0, dhs.ptr, 300, 0)
            ctx.msm_begin(0, dhb.ptr, 0, dhs.ptr, 300, 1)
            assert gpu_aff(ctx.msm_end(0, 0), 4) == want[300]
            ctx.msm_begin(0, dhb.ptr, 0, dhs.ptr, 3000, 0)
            assert gpu_aff(ctx.msm_end(0, 1), 4) == want[300]
            assert gpu_aff(ctx.msm_end(0, 0), 4) == want[3000]
        finally:
            ctx.set_msm_small(-2, 0, -1)

        # the R1CS product with m = 100, then m = 5000 (ws_vec again, through kg_r1cs_prod): both queued, then read
        rng = np.random.default_rng(11)
        nv, prods = 400, []
        z = O.gen_scalars(0, SEED + 1770, 0, nv)
        dz = ctx.upload(z)
        for m in (100, 5000):
            cnt = rng.integers(0, 6, m)
            rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
            col = rng.integers(0, nv, int(rp[-1])).astype(np.uint64)
            val = O.gen_scalars(0, SEED + 1771 + m, 0, int(rp[-1]))
            dev = [ctx.upload(t) for t in (rp, col, val)]
            out = ctx.empty((m, 4))
            ctx.r1cs_prod(0, dev[0].ptr, dev[1].ptr, dev[2].ptr, m, dz.ptr, out.ptr)
            prods.append((m, out, dev, O.matrix_prod(0, (rp, col, val), z)))
        for m, out, _, want in prods:
            assert (out.numpy() == want).all(), ("r1cs_prod", m)
    finally:
        gc.collect()
        ctx.close()
