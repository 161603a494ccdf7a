"""kg_groth16_prove_batch beside the two loops it replaces, in one process on one context with resident inputs: the chain circuit at
m in {2^4, 2^6, 2^8, 2^10, 2046} constraints with count in {4, 16, 64, 256} distinct witnesses (dense arrays: stride = length), timed as
  (a) batch   : one kg_groth16_prove_batch followed by one kg_ctx_sync;
  (b) inflight: count proofs through kg_groth16_prove_begin / _end, two in flight (what Prover.create_proofs does, without its uploads);
  (c) blocking: count calls of kg_groth16_prove_bn254.
The loops run with the inputs declared complete (kg_ctx_set_inputs_complete, as bench.py measures them).  The three are measured in
alternating rounds (a, b, c, a, b, c, ...) so that a drift of the box meets all of them; every figure is the median of --reps (>= 20) rounds
after warm-up rounds, by a wall clock around work that ends in a synchronise or in the last proof.  Before the timing every proof of the
batch is compared with the blocking call's.  After it, one profiled batch gives the phase split of the call (device events around the
launches, summed over its launch groups): fill / transforms / point-wise step / the five batched MSMs / G1 chains / G2 chain and B /
finishing lanes.  Cells where the batch is slower than a loop are marked, not hidden; the last lines give the crossover count per size.
No gate: the exit status is 0 unless a proof differs.

    python tools/dbg/g16_batch_timing.py [--out profiles/g16_batch_timing.txt] [--reps 20] [--cells m:count,...]
"""
import argparse
import gc
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import kogarashi_amd as K  # noqa: E402
from kogarashi_amd import lib as L  # noqa: E402
from kogarashi_amd import synthetic as S  # noqa: E402
from kogarashi_amd.api import groth16_setup  # noqa: E402

SIZES = (1 << 4, 1 << 6, 1 << 8, 1 << 10, 2046)
COUNTS = (4, 16, 64, 256)
PHASES = (("fill", ("g16_batch_fill",)), ("ntt", ("ntt_batch",)), ("combine", ("g16_batch_combine",)),
          ("msm", ("small_msm_batch", "small_combine_batch", "small_finish_batch")), ("chains_g1", ("g16_batch_chains_g1",)),
          ("b_g2", ("g16_batch_b_g2",)), ("finish_g1", ("g16_batch_finish_g1",)))


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g16_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cells", default="", help="m:count,... instead of the whole table (a profiler run of one cell)")
    a = ap.parse_args()
    reps = max(a.reps, 20)
    cells = [(m, c) for m in SIZES for c in COUNTS]
    if a.cells:
        cells = [tuple(int(v) for v in item.split(":")) for item in a.cells.split(",")]
    gc.disable()                                           # no cyclic collection inside a timed loop
    ctx = K.Context(0)
    ctx.set_inputs_complete(True)
    rows = [f"{'m':>5s} {'count':>5s} {'groups':>6s} {'batch us':>10s} {'inflight us':>12s} {'blocking us':>12s} {'us/proof':>9s} {'batch/inflight':>14s} {'batch/blocking':>14s} "
            + " ".join(f"{name + ' us':>12s}" for name, _ in PHASES) + "  note"]
    slower, ratio = [], {}
    for m in sorted({m for m, _ in cells}):
        cs0 = S.ChainCircuit(m)
        params = groth16_setup(cs0.a, cs0.b, cs0.c, m, cs0.l, cs0.m_l_1, S.fixed_toxic(), S.FrOps, ctx=ctx)
        prover = K.Prover(params, m, cs0.l, cs0.m_l_1, ctx=ctx)
        top = max(c for mm, c in cells if mm == m)
        circ = [S.ChainCircuit(m, t0=0x123456789ABCDEF0123456789ABCDEF + 977 * b) for b in range(top)]
        r0, s0 = S.fixed_rs()
        rs = S.mont_vec([(S.FrOps.to_i(r0) + 31 * b) % S.R_MOD for b in range(top)] + [(S.FrOps.to_i(s0) + 57 * b) % S.R_MOD for b in range(top)])
        da, db, dc = (ctx.upload(np.stack([getattr(c, name) for c in circ])) for name in ("a_eval", "b_eval", "c_eval"))
        dx, dw = ctx.upload(np.stack([c.x for c in circ])), ctx.upload(np.stack([c.w for c in circ]))
        dr, ds = ctx.upload(rs[:top]), ctx.upload(rs[top:])
        l, wl = cs0.l, cs0.m_l_1
        for count in [c for mm, c in cells if mm == m]:
            d_out, d_inf = ctx.empty((count, 32)), ctx.empty((count, 3), dtype=np.uint8)
            ctx.sync()

            def batch():
                ctx.groth16_prove_batch(prover.crs, da.ptr, db.ptr, dc.ptr, m, dx.ptr, l, dw.ptr, wl, dr.ptr, ds.ptr, count, d_out.ptr, d_inf.ptr)
                ctx.sync()

            def args(b):
                return (prover.crs, da.ptr + 32 * b * m, db.ptr + 32 * b * m, dc.ptr + 32 * b * m, dx.ptr + 32 * b * l, dw.ptr + 32 * b * wl, rs[b], rs[top + b])

            def blocking():
                return [ctx.groth16_prove(*args(b)) for b in range(count)]

            def inflight():
                out = []
                for b in range(count):
                    if b >= 2:
                        out.append(ctx.groth16_prove_end(b & 1))
                    ctx.groth16_prove_begin(*args(b), b & 1)
                for b in range(max(count - 2, 0), count):
                    out.append(ctx.groth16_prove_end(b & 1))
                return out

            # the same proofs three ways, before anything is timed
            batch()
            got, gfl = d_out.numpy(), d_inf.numpy()
            ref, fly = blocking(), inflight()
            for b in range(count):
                assert (got[b] == np.concatenate(ref[b][:3])).all() and (gfl[b] == ref[b][3]).all(), (m, count, b)
                assert all((x == y).all() for x, y in zip(fly[b], ref[b])), (m, count, b)
            for _ in range(a.warm):
                batch(); inflight(); blocking()
            tb, tf, tl = [], [], []
            for _ in range(reps):                          # alternating rounds
                tb.append(timed_us(batch))
                tf.append(timed_us(inflight))
                tl.append(timed_us(blocking))
            mb, mf, ml = statistics.median(tb), statistics.median(tf), statistics.median(tl)
            ctx.profile_enable(True)
            batch()
            ph = ctx.profile_summary()
            ctx.profile_enable(False)
            us = lambda names: sum(ph.get(n, (0.0, 0))[0] for n in names) * 1e3
            note = []
            if mb >= mf:
                note.append("batch SLOWER than two in flight")
            if mb >= ml:
                note.append("batch SLOWER than the blocking loop")
            if note:
                slower.append((m, count))
            ratio[(m, count)] = mb / mf
            rows.append(f"{m:5d} {count:5d} {L.groth16_prove_batch_plan(m, l, wl, count)[0]:6d} {mb:10.1f} {mf:12.1f} {ml:12.1f} {mb / count:9.1f} {mb / mf:14.3f} {mb / ml:14.3f} "
                        + " ".join(f"{us(names):12.1f}" for _, names in PHASES) + "  " + "; ".join(note))
            print(rows[-1], flush=True)
            del d_out, d_inf
        del prover, da, db, dc, dx, dw, dr, ds
    head = ("kg_groth16_prove_batch timing (tools/dbg/g16_batch_timing.py): chain circuit, resident inputs, dense batches; batch = one call + one sync, inflight = count "
            "proofs through kg_groth16_prove_begin / _end two in flight, blocking = count kg_groth16_prove_bn254 calls (inputs declared complete for both loops); "
            f"alternating rounds, medians of {reps} after {a.warm} warm-up rounds, wall clock; the phase columns: device events around the launches of one profiled batch")
    tail = []
    for m in sorted({m for m, _ in ratio}):
        wins = [c for (mm, c), q in sorted(ratio.items()) if mm == m and q < 1.0]
        tail.append(f"m = {m}: the batch beats two in flight from count = {min(wins)}" if wins else f"m = {m}: the batch beats two in flight at no measured count")
    tail.append("cells where the batch is slower than a loop: " + (", ".join(f"({m}, {c})" for m, c in slower) if slower else "none"))
    text = "\n".join([head] + rows + tail) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
