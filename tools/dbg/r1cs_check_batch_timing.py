"""kg_r1cs_check_batch / kg_groth16_witness_check_batch beside what a caller did before them, in one process on one context with resident
inputs: the chain circuit at m in {2^4, 2^10, 2046, 2^14} constraints with count in {4, 16, 256} distinct valid witnesses, timed as
  (a) batch   : one kg_r1cs_check_batch on the packed z vectors followed by one kg_ctx_sync;
  (b) singles : count blocking kg_r1cs_check calls on the same pre-built z vectors -- the only way before the batched entry;
  (c) prove   : kg_groth16_prove_r1cs_batch followed by one kg_ctx_sync, alone, and
  (c') checked: kg_groth16_witness_check_batch on the same x / w arrays enqueued in front of that proving call, then one kg_ctx_sync -- the
                difference is what the check adds to a batch (m <= 2046 only: the batched prover takes no longer circuit).
The variants are measured in alternating rounds (a, b, c, c', a, ...) so that a drift of the box meets all of them; every figure is the
median of --reps (>= 20) rounds after warm-up rounds, by a wall clock around work that ends in a synchronise, with the interquartile range
of the rounds beside it.  Before the timing every summary pair of (a) and of the split form is compared with (b)'s answers.
No gate and no promised ratio: the table says where the batch loses to the loop as plainly as where it wins.

    python tools/dbg/r1cs_check_batch_timing.py [--out profiles/r1cs_check_batch_timing.txt] [--reps 20] [--cells m:count,...] [--no-prove]
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
from kogarashi_amd import synthetic as S  # noqa: E402
from kogarashi_amd.api import groth16_setup  # noqa: E402

SIZES = (1 << 4, 1 << 10, 2046, 1 << 14)
COUNTS = (4, 16, 256)
PROVER_MAX = 2046


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def med_iqr(ts):
    q = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q[2] - q[0]


class witness:
    """x = [1, t_0], w = [t_1 .. t_m] of the chain t_{i+1} = t_i (t_i + 1): synthetic.ChainCircuit's assignment without its matrices"""

    def __init__(self, m, t0):
        t = [t0 % S.R_MOD]
        for _ in range(m):
            t.append(t[-1] * (t[-1] + 1) % S.R_MOD)
        tm = S.mont_vec(t)
        self.x, self.w = np.stack([np.array(S.mont(1), dtype=np.uint64), tm[0]]), tm[1:]


def run_cells(ctx, cells, reps, warm, prove, rows):
    for m in sorted({m for m, _ in cells}):
        cs0 = S.ChainCircuit(m)
        l, wl = cs0.l, cs0.m_l_1
        nz = l + wl
        top = max(c for mm, c in cells if mm == m)
        circ = [witness(m, 0x123456789ABCDEF0123456789ABCDEF + 977 * b) for b in range(top)]
        prover = None
        if prove and m <= PROVER_MAX:
            params = groth16_setup(cs0.a, cs0.b, cs0.c, m, l, wl, S.fixed_toxic(), S.FrOps, ctx=ctx)
            prover = K.Prover(params, m, l, wl, ctx=ctx)
            prover.attach_constraint_system(cs0.a, cs0.b, cs0.c)
            keep = prover._cs
        else:
            keep = [(ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)), ctx.upload(np.ascontiguousarray(col, dtype=np.uint64)),
                     ctx.upload(np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4))) for rp, col, val in (cs0.a, cs0.b, cs0.c)]
        mats = [tuple(d.ptr for d in trip) for trip in keep]
        dx, dw = ctx.upload(np.stack([c.x for c in circ])), ctx.upload(np.stack([c.w for c in circ]))
        dz = ctx.upload(np.stack([np.concatenate([c.x, c.w]) for c in circ]))
        r0, s0 = S.fixed_rs()
        rs = S.mont_vec([(S.FrOps.to_i(r0) + 31 * b) % S.R_MOD for b in range(top)] + [(S.FrOps.to_i(s0) + 57 * b) % S.R_MOD for b in range(top)])
        dr, ds = ctx.upload(rs[:top]), ctx.upload(rs[top:])
        for count in [c for mm, c in cells if mm == m]:
            sum_a, sum_c = ctx.empty((count, 2), dtype=np.uint32), ctx.empty((count, 2), dtype=np.uint32)
            o, f = ctx.empty((count, 32)), ctx.empty((count, 3), dtype=np.uint8)
            single = []
            ctx.sync()

            def batch():
                ctx.r1cs_check_batch(0, mats[0], mats[1], mats[2], m, dz.ptr, nz, count, summary=sum_a)
                ctx.sync()

            def singles():
                single.clear()
                for b in range(count):
                    single.append(ctx.r1cs_check(0, mats[0], mats[1], mats[2], m, dz.ptr + 32 * b * nz))

            def prove_alone():
                ctx.groth16_prove_r1cs_batch(prover.crs, mats[0], mats[1], mats[2], dx.ptr, l, dw.ptr, wl, dr.ptr, ds.ptr, count, o.ptr, f.ptr)
                ctx.sync()

            def prove_checked():
                ctx.groth16_witness_check_batch(mats[0], mats[1], mats[2], m, l, wl, dx.ptr, l, dw.ptr, wl, count, summary=sum_c)
                ctx.groth16_prove_r1cs_batch(prover.crs, mats[0], mats[1], mats[2], dx.ptr, l, dw.ptr, wl, dr.ptr, ds.ptr, count, o.ptr, f.ptr)
                ctx.sync()

            variants = [batch, singles] + ([prove_alone, prove_checked] if prover else [])
            batch(); singles()
            ctx.groth16_witness_check_batch(mats[0], mats[1], mats[2], m, l, wl, dx.ptr, l, dw.ptr, wl, count, summary=sum_c)
            want = np.array(single, dtype=np.uint32)
            assert (want == np.array([0, m], dtype=np.uint32)).all(), (m, count, "the chain's own assignments hold")
            assert (sum_a.numpy() == want).all() and (sum_c.numpy() == want).all(), (m, count)
            for _ in range(warm):
                for v in variants:
                    v()
            ts = [[] for _ in variants]
            for _ in range(reps):                          # alternating rounds
                for t, v in zip(ts, variants):
                    t.append(timed_us(v))
            stats = [med_iqr(t) for t in ts]
            (ma, ia), (mb, ib) = stats[:2]
            note = "batch faster by more than the spread" if mb - ma > max(ia, ib) else ("within the spread" if abs(mb - ma) <= max(ia, ib) else "batch SLOWER than the loop")
            line = f"{m:6d} {count:5d} {ma:11.1f} {ia:9.1f} {mb:11.1f} {ib:9.1f} {ma / mb:7.3f}"
            if prover:
                (mc, ic), (md, id_) = stats[2:]
                line += f" {mc:11.1f} {ic:9.1f} {md:11.1f} {id_:9.1f} {md - mc:10.1f}"
            else:
                line += f" {'-':>11s} {'-':>9s} {'-':>11s} {'-':>9s} {'-':>10s}"
            rows.append(line + "  " + note)
            print(rows[-1], flush=True)
        del prover, keep, dx, dw, dz, dr, ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cells", default="", help="m:count,... instead of the whole table")
    ap.add_argument("--no-prove", action="store_true", help="skip (c) and (c'): no CRS is set up")
    a = ap.parse_args()
    reps = max(a.reps, 20)
    cells = [(m, c) for m in SIZES for c in COUNTS]
    if a.cells:
        cells = [tuple(int(v) for v in item.split(":")) for item in a.cells.split(",")]
    gc.disable()                                           # no cyclic collection inside a timed loop
    ctx = K.Context(0)
    head = ("kg_r1cs_check_batch timing (tools/dbg/r1cs_check_batch_timing.py): chain circuit over Fr, resident inputs, dense batches, every witness valid, no status "
            "array; (a) = one kg_r1cs_check_batch + one sync, (b) = count blocking kg_r1cs_check calls on the pre-built z vectors, (c) = kg_groth16_prove_r1cs_batch + "
            "one sync, (c') = kg_groth16_witness_check_batch on the same x / w in front of it + one sync; alternating rounds, medians of "
            f"{reps} after {a.warm} warm-up rounds, wall clock, iqr = interquartile range of the rounds")
    rows = [head, f"{'m':>6s} {'count':>5s} {'(a) us':>11s} {'iqr':>9s} {'(b) us':>11s} {'iqr':>9s} {'a/b':>7s} {'(c) us':>11s} {'iqr':>9s} {'checked us':>11s} {'iqr':>9s} {'added us':>10s}  note"]
    run_cells(ctx, cells, reps, a.warm, not a.no_prove, rows)
    text = "\n".join(rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
