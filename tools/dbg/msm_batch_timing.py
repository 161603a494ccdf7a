"""kg_commit_batch beside the two loops it replaces, in one process on one context with resident inputs: G1 at n in {32, 2^10, 2048} with
count in {4, 16, 256}, G2 at n in {32, 2^10} with count in {4, 64}; count dense vectors (stride = n) against one base array, timed as
  (a) batch   : one kg_commit_batch followed by one kg_ctx_sync;
  (b) blocking: count calls of kg_commit (each waits for its point);
  (c) inflight: count calls through kg_msm_begin / kg_msm_end, four tickets in flight.
The three are measured in alternating rounds (a, b, c, a, b, c, ...) so that a drift of the box meets all of them; every figure is the median
of --reps (>= 20) rounds after warm-up rounds, by a wall clock around work that ends in a synchronise or in the last result.  Before the
timing every point of the batch is compared with kg_commit's.  After it, one profiled batch gives the phase split (device events around the
launches): main kernel / combine / finish.  The gate: the batch at (G1, 2^10, 256) must be faster than the four-in-flight loop beside it --
the exit status is 1 otherwise.  Cells where the batch is slower than a loop are marked, not hidden.

    python tools/dbg/msm_batch_timing.py [--out profiles/msm_batch_timing.txt] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import kogarashi_amd as K  # noqa: E402
from kogarashi_amd import lib as L  # noqa: E402

SEED = 0x4B6F676172617368
CELLS = [(K.KG_G1, n, c) for n in (32, 1 << 10, 2048) for c in (4, 16, 256)] + [(K.KG_G2, n, c) for n in (32, 1 << 10) for c in (4, 64)]
GATE = (K.KG_G1, 1 << 10, 256)


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def make_bases(ctx, curve, n, seed):
    if curve == K.KG_G2:                                   # generator multiples: in the r-torsion, as the short kernel's halved scalars need
        dk = ctx.empty((n, 4))
        ctx.gen_scalars(K.KG_FR, seed, 0, n, dk.ptr)
        dxy, dinf = ctx.empty((n, 16)), ctx.empty((n,), dtype=np.uint8)
        ctx.fixed_base_mul(curve, dk.ptr, n, dxy.ptr, dinf.ptr)
        return dxy, dinf
    d = ctx.empty((n, 8))
    ctx.gen_bases(curve, seed, 0, n, d.ptr)
    return d, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    reps = max(a.reps, 20)
    ctx = K.Context(0)
    rows, slower = [], []
    gate_met = None
    rows.append(f"{'curve':>5s} {'n':>5s} {'count':>5s} {'groups':>6s} {'batch us':>10s} {'blocking us':>12s} {'inflight us':>12s} {'batch/blocking':>14s} {'batch/inflight':>14s}"
                f" {'main us':>9s} {'combine us':>10s} {'finish us':>10s}  note")
    for curve, n, count in CELLS:
        w = 16 if curve == K.KG_G2 else 8
        db, di = make_bases(ctx, curve, n, SEED + 31 * n + curve)
        dip = di.ptr if di is not None else 0
        ds = ctx.empty((count * n, 4))
        ctx.gen_scalars(K.KG_FR, SEED + 17 * n + count, 0, count * n, ds.ptr)
        oxy, ofl = ctx.empty((count, w)), ctx.empty((count,), dtype=np.uint8)
        ctx.sync()

        def batch():
            ctx.commit_batch(curve, db.ptr, dip, ds.ptr, n, count, n, oxy.ptr, ofl.ptr)
            ctx.sync()

        def blocking():
            return [ctx.commit(curve, db.ptr, dip, ds.ptr + 32 * b * n, n) for b in range(count)]

        def inflight():
            out = []
            for b in range(count):
                if b >= 4:
                    out.append(ctx.msm_end(curve, b % 4))
                ctx.msm_begin(curve, db.ptr, dip, ds.ptr + 32 * b * n, n, b % 4)
            for b in range(max(count - 4, 0), count):
                out.append(ctx.msm_end(curve, b % 4))
            return out

        # the same points three ways, before anything is timed
        batch()
        bxy, bfl = oxy.numpy(), ofl.numpy()
        ref, fly = blocking(), inflight()
        for b in range(count):
            assert int(bfl[b]) == ref[b][1] and (bxy[b] == ref[b][0]).all(), (curve, n, count, b)
            assert (fly[b][:w] == ref[b][0]).all(), (curve, n, count, b)
        for _ in range(a.warm):
            batch(); blocking(); inflight()
        tb, tl, tf = [], [], []
        for _ in range(reps):                              # alternating rounds
            tb.append(timed_us(batch))
            tl.append(timed_us(blocking))
            tf.append(timed_us(inflight))
        mb, ml, mf = statistics.median(tb), statistics.median(tl), statistics.median(tf)
        ctx.profile_enable(True)
        batch()
        ph = ctx.profile_summary()
        ctx.profile_enable(False)
        us = lambda name: ph.get(name, (0.0, 0))[0] * 1e3
        note = []
        if mb >= ml:
            note.append("batch SLOWER than the blocking loop")
        if mb >= mf:
            note.append("batch SLOWER than four in flight")
        if mb >= ml or mb >= mf:
            slower.append((curve, n, count))
        if (curve, n, count) == GATE:
            gate_met = mb < mf
            note.append("gate: met" if gate_met else "gate: MISSED")
        rows.append(f"{('G1', 'Gk', 'G2')[curve]:>5s} {n:5d} {count:5d} {L.commit_batch_plan(curve, n, count)[0]:6d} {mb:10.1f} {ml:12.1f} {mf:12.1f} {mb / ml:14.3f} {mb / mf:14.3f}"
                    f" {us('small_msm_batch'):9.1f} {us('small_combine_batch'):10.1f} {us('small_finish_batch'):10.1f}  {'; '.join(note)}")
        del db, di, ds, oxy, ofl
    head = ("kg_commit_batch timing (tools/dbg/msm_batch_timing.py): resident inputs, dense batches; batch = one call + one sync, blocking = count kg_commit calls, "
            f"inflight = count kg_msm_begin / kg_msm_end with four tickets; alternating rounds, medians of {reps} after {a.warm} warm-up rounds, wall clock; "
            "main / combine / finish: device events around the launches of one profiled batch (summed over its launch groups)")
    tail = [f"gate (G1, n = 1024, count = 256: batch median < four-in-flight median): {'met' if gate_met else 'MISSED'}",
            "cells where the batch is slower than a loop: " + (", ".join(f"({('G1', 'Gk', 'G2')[c]}, {n}, {k})" for c, n, k in slower) if slower else "none")]
    text = "\n".join([head] + rows + tail) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 0 if gate_met else 1


if __name__ == "__main__":
    sys.exit(main())
