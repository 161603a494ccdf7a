"""kg_groth16_prove_r1cs_batch beside what a caller with witnesses did before it, in one process on one context with resident inputs: the
chain circuit at m in {2^4, 2^10, 2046} constraints with count in {16, 256} distinct witnesses (dense arrays: stride = length), timed as
  (a) r1cs batch : one kg_groth16_prove_r1cs_batch followed by one kg_ctx_sync;
  (b) evaluate   : 3 * count calls of kg_r1cs_evaluate into packed arrays, then kg_groth16_prove_batch, then one kg_ctx_sync -- every
                   line of it is code from before the batched product existed: the baseline;
  (c) inflight   : count proofs through kg_groth16_prove_r1cs_begin / kg_groth16_prove_end, two in flight.
The three are measured in alternating rounds (a, b, c, a, b, c, ...) so that a drift of the box meets all of them; every figure is the
median of --reps (>= 20) rounds after warm-up rounds, by a wall clock around work that ends in a synchronise or in the last proof, with the
interquartile range of the rounds beside it.  Before the timing every proof of (a) is compared with (b)'s and (c)'s.
Stand-alone, kg_r1cs_prod_batch against count calls of kg_r1cs_prod (each followed by one sync at the end of the round) at m = 2^10 with
count = 256 and at m = 2^18 with count = 16 -- the second shows what re-reading a 13 MB matrix per vector costs.
No gate: the exit status is 0 unless a proof or a product differs.

    python tools/dbg/r1cs_batch_timing.py [--out profiles/r1cs_batch_timing.txt] [--reps 20] [--cells m:count,...] [--no-prod]
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

SIZES = (1 << 4, 1 << 10, 2046)
COUNTS = (16, 256)
PROD_CELLS = ((1 << 10, 256), (1 << 18, 16))


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def med_iqr(ts):
    q = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q[2] - q[0]


def witnesses(m, top):
    return [S.ChainCircuit(m, t0=0x123456789ABCDEF0123456789ABCDEF + 977 * b) for b in range(top)]


def prover_cells(ctx, cells, reps, warm, rows):
    for m in sorted({m for m, _ in cells}):
        cs0 = S.ChainCircuit(m)
        params = groth16_setup(cs0.a, cs0.b, cs0.c, m, cs0.l, cs0.m_l_1, S.fixed_toxic(), S.FrOps, ctx=ctx)
        prover = K.Prover(params, m, cs0.l, cs0.m_l_1, ctx=ctx)
        prover.attach_constraint_system(cs0.a, cs0.b, cs0.c)
        mats = [tuple(d.ptr for d in trip) for trip in prover._cs]
        top = max(c for mm, c in cells if mm == m)
        circ = witnesses(m, top)
        r0, s0 = S.fixed_rs()
        rs = S.mont_vec([(S.FrOps.to_i(r0) + 31 * b) % S.R_MOD for b in range(top)] + [(S.FrOps.to_i(s0) + 57 * b) % S.R_MOD for b in range(top)])
        l, wl = cs0.l, cs0.m_l_1
        nz = l + wl
        dx, dw = ctx.upload(np.stack([c.x for c in circ])), ctx.upload(np.stack([c.w for c in circ]))
        dz = ctx.upload(np.stack([np.concatenate([c.x, c.w]) for c in circ]))        # what (b)'s caller holds to evaluate against
        dr, ds = ctx.upload(rs[:top]), ctx.upload(rs[top:])
        ev = [ctx.empty((top * m, 4)) for _ in range(3)]
        for count in [c for mm, c in cells if mm == m]:
            o_a, f_a = ctx.empty((count, 32)), ctx.empty((count, 3), dtype=np.uint8)
            o_b, f_b = ctx.empty((count, 32)), ctx.empty((count, 3), dtype=np.uint8)
            ctx.sync()

            def r1cs_batch():
                ctx.groth16_prove_r1cs_batch(prover.crs, mats[0], mats[1], mats[2], dx.ptr, l, dw.ptr, wl, dr.ptr, ds.ptr, count, o_a.ptr, f_a.ptr)
                ctx.sync()

            def evaluate():
                for b in range(count):
                    for v in range(3):
                        ctx.r1cs_evaluate(mats[v][0], mats[v][1], mats[v][2], m, dz.ptr + 32 * b * nz, ev[v].ptr + 32 * b * m)
                ctx.groth16_prove_batch(prover.crs, ev[0].ptr, ev[1].ptr, ev[2].ptr, m, dx.ptr, l, dw.ptr, wl, dr.ptr, ds.ptr, count, o_b.ptr, f_b.ptr)
                ctx.sync()

            def inflight():
                out = []
                for b in range(count):
                    if b >= 2:
                        out.append(ctx.groth16_prove_end(b & 1))
                    ctx.groth16_prove_r1cs_begin(prover.crs, mats[0], mats[1], mats[2], dx.ptr + 32 * b * l, dw.ptr + 32 * b * wl, rs[b], rs[top + b], b & 1)
                for b in range(max(count - 2, 0), count):
                    out.append(ctx.groth16_prove_end(b & 1))
                return out

            r1cs_batch(); evaluate()
            fly = inflight()
            got, gfl, want, wfl = o_a.numpy(), f_a.numpy(), o_b.numpy(), f_b.numpy()
            assert (got == want).all() and (gfl == wfl).all(), (m, count, "evaluate + kg_groth16_prove_batch")
            for b in range(count):
                assert (got[b] == np.concatenate(fly[b][:3])).all() and (gfl[b] == fly[b][3]).all(), (m, count, b, "two in flight")
            for _ in range(warm):
                r1cs_batch(); evaluate(); inflight()
            ta, tb, tc = [], [], []
            for _ in range(reps):                          # alternating rounds
                ta.append(timed_us(r1cs_batch))
                tb.append(timed_us(evaluate))
                tc.append(timed_us(inflight))
            (ma, ia), (mb, ib), (mc, ic) = med_iqr(ta), med_iqr(tb), med_iqr(tc)
            gain = mb - ma
            note = "faster than (b) by more than the spread" if gain > max(ia, ib) else ("NOT faster than (b) by more than the spread" if gain > 0 else "SLOWER than (b)")
            rows.append(f"{m:5d} {count:5d} {L.groth16_prove_batch_plan(m, l, wl, count)[0]:6d} {ma:11.1f} {ia:9.1f} {mb:11.1f} {ib:9.1f} {mc:11.1f} {ic:9.1f} "
                        f"{gain:10.1f} {ma / mb:7.3f} {ma / mc:7.3f}  {note}")
            print(rows[-1], flush=True)
        del prover, dx, dw, dz, dr, ds, ev


def prod_cells(ctx, reps, warm, rows):
    for m, count in PROD_CELLS:
        cs0 = S.ChainCircuit(m)
        rp, col, val = cs0.a
        d = (ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)), ctx.upload(np.ascontiguousarray(col, dtype=np.uint64)),
             ctx.upload(np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)))
        nz = cs0.l + cs0.m_l_1
        z = np.stack([np.concatenate([cs0.x, cs0.w])] * count)
        z[:, 1:, 0] += np.arange(count, dtype=np.uint64)[:, None]             # distinct vectors (canonical: the low word only, far below p)
        dz = ctx.upload(z)
        o_b, o_s = ctx.empty((count * m, 4)), ctx.empty((count * m, 4))
        ctx.sync()

        def batched():
            ctx.r1cs_prod_batch(0, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr, nz, count, o_b.ptr, m)
            ctx.sync()

        def singles():
            for b in range(count):
                ctx.r1cs_prod(0, d[0].ptr, d[1].ptr, d[2].ptr, m, dz.ptr + 32 * b * nz, o_s.ptr + 32 * b * m)
            ctx.sync()

        batched(); singles()
        assert o_b.numpy().tobytes() == o_s.numpy().tobytes(), (m, count)
        for _ in range(warm):
            batched(); singles()
        tb, ts = [], []
        for _ in range(reps):
            tb.append(timed_us(batched))
            ts.append(timed_us(singles))
        (mb, ib), (ms, is_) = med_iqr(tb), med_iqr(ts)
        mib = (int(rp[-1]) * 40 + (m + 1) * 8) / 2**20
        rows.append(f"{m:7d} {count:5d} {mib:9.1f} {mb:11.1f} {ib:9.1f} {ms:11.1f} {is_:9.1f} {mb / ms:7.3f}")
        print(rows[-1], flush=True)
        del d, dz, o_b, o_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cells", default="", help="m:count,... instead of the whole prover table")
    ap.add_argument("--no-prod", action="store_true", help="skip the stand-alone product")
    a = ap.parse_args()
    reps = max(a.reps, 20)
    cells = [(m, c) for m in SIZES for c in COUNTS]
    if a.cells:
        cells = [tuple(int(v) for v in item.split(":")) for item in a.cells.split(",")]
    gc.disable()                                           # no cyclic collection inside a timed loop
    ctx = K.Context(0)
    head = ("kg_groth16_prove_r1cs_batch timing (tools/dbg/r1cs_batch_timing.py): chain circuit, resident inputs, dense batches; (a) = one call + one sync, (b) = 3 * count "
            "kg_r1cs_evaluate calls into packed arrays + kg_groth16_prove_batch + one sync (the baseline: code from before the batched product), (c) = count proofs through "
            f"kg_groth16_prove_r1cs_begin / _end two in flight; alternating rounds, medians of {reps} after {a.warm} warm-up rounds, wall clock, iqr = interquartile range of the rounds")
    rows = [head, f"{'m':>5s} {'count':>5s} {'groups':>6s} {'(a) us':>11s} {'iqr':>9s} {'(b) us':>11s} {'iqr':>9s} {'(c) us':>11s} {'iqr':>9s} {'(b)-(a) us':>10s} {'a/b':>7s} {'a/c':>7s}  note"]
    prover_cells(ctx, cells, reps, a.warm, rows)
    if not a.no_prod:
        rows.append("kg_r1cs_prod_batch against count kg_r1cs_prod calls, one sync at the end of each (matrix A of the chain circuit, Fr; MiB = the matrix's row_ptr, col and val)")
        rows.append(f"{'m':>7s} {'count':>5s} {'MiB':>9s} {'batch us':>11s} {'iqr':>9s} {'singles us':>11s} {'iqr':>9s} {'b/s':>7s}")
        prod_cells(ctx, reps, a.warm, rows)
    text = "\n".join(rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
