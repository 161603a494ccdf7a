"""A batch of Nova folds beside what a caller did before the batched entries, in one process on one context with resident inputs: the chain
circuit over Fr / G1 at m in {2^4, 2^10, 2046, 2^14} constraints (the last one beyond kg_commit_batch's 2048 pairs: its blocking loop)
with count in {4, 16, 64, 256} pairs (z1_b, z2_b, E_b, r_b), timed at the C level -- the raw entries on device arrays, none of api.py's
packing -- as
  (a) batch  : what NovaProver.fold_begin + fold_end enqueue: kg_nova_cross_term_batch, kg_commit_batch over the T rows, the read-back of the
               count commitments, the upload of the challenges and of the point fold's Q operands, two kg_field_vec_axpy_batch (z1 += r z2,
               E += r T), one kg_points_muladd_batch over the 2 count interleaved pairs, one kg_ctx_sync;
  (b) loop   : per pair kg_nova_cross_term (u on the host), a blocking kg_commit, three kg_field_vec_axpy (W, E, u | x), two two-point
               kg_msm_host, and one kg_ctx_sync at the end -- the only way before the batched entries.
and the three primitives alone, each followed by one kg_ctx_sync, beside their single-call loops:
  cross  kg_nova_cross_term_batch        against count kg_nova_cross_term
  axpy   kg_field_vec_axpy_batch on z    against count kg_field_vec_axpy
  points kg_points_muladd_batch, 2 count against 2 count two-point kg_msm_host
The variants are measured in alternating rounds so that a drift of the box meets all of them; every figure is the median of --reps (>= 20)
rounds after warm-up rounds, by a wall clock around work that ends in a synchronise, with the interquartile range of the rounds beside it.
Before the timing the batch's folded z, E and points are compared with the loop's.  No gate and no promised ratio: the table says where the
batch loses to the loop as plainly as where it wins.

    python tools/dbg/nova_fold_batch_timing.py [--out profiles/nova_fold_batch_timing.txt] [--reps 20] [--cells m:count,...]
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

SIZES = (1 << 4, 1 << 10, 2046, 1 << 14)
COUNTS = (4, 16, 64, 256)
FR, G1 = 0, 0


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def med_iqr(ts):
    q = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q[2] - q[0]


def chain_z(m, t0):
    """z = (1 | t_0 | t_1 .. t_m) of the chain t_{i+1} = t_i (t_i + 1): synthetic.ChainCircuit's assignment, u = x[0] = 1"""
    t = [t0 % S.R_MOD]
    for _ in range(m):
        t.append(t[-1] * (t[-1] + 1) % S.R_MOD)
    return np.concatenate([np.array(S.mont(1), dtype=np.uint64).reshape(1, 4), S.mont_vec(t)])


def run_cells(ctx, cells, reps, warm, rows):
    one = np.array(S.mont(1), dtype=np.uint64)
    for m in sorted({m for m, _ in cells}):
        cs0 = S.ChainCircuit(m)
        lx, nz = cs0.l - 1, cs0.l + cs0.m_l_1              # z = (u | x' | w): l = 1 + len(x')
        nw = nz - 1 - lx
        keep = [(ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)), ctx.upload(np.ascontiguousarray(col, dtype=np.uint64)),
                 ctx.upload(np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4))) for rp, col, val in (cs0.a, cs0.b, cs0.c)]
        mats = [tuple(d.ptr for d in trip) for trip in keep]
        top = max(c for mm, c in cells if mm == m)
        z1h = np.stack([chain_z(m, 0x123456789ABCDEF0123456789ABCDEF + 977 * b) for b in range(top)])
        z2h = np.stack([chain_z(m, 0xFEDCBA9876543210FEDCBA987654321 + 761 * b) for b in range(top)])
        g = ctx.empty((m, 8))
        ctx.gen_bases(G1, 0x4B6F676172617368, 0, m, g.ptr)
        ctx.bases_register(G1, g.ptr, 0, m)
        d_rs, d_e0 = ctx.empty((top, 4)), ctx.empty((top, m, 4))
        ctx.gen_scalars(FR, 0x4B6F676172617369, 0, top, d_rs.ptr)
        ctx.gen_scalars(FR, 0x4B6F67617261736A, 0, top * m, d_e0.ptr)
        rs = d_rs.numpy()
        # the instances' commitments: any curve points will do for the timing
        pts = ctx.empty((4 * top, 8))
        ctx.gen_bases(G1, 0x4B6F67617261736B, 0, 4 * top, pts.ptr)
        pts_h = pts.numpy().reshape(top, 4, 8)             # per pair: cW1, cE1, cW2, (unused)
        for count in [c for mm, c in cells if mm == m]:
            dz1s, dz2 = ctx.upload(z1h[:count]), ctx.upload(z2h[:count])
            dz1, de = ctx.empty((count, nz, 4)), ctx.empty((count, m, 4))
            dt, d_ct, d_cti = ctx.empty((count, m, 4)), ctx.empty((count, 8)), ctx.empty((count,), dtype=np.uint8)
            du1 = ctx.upload(np.ascontiguousarray(z1h[:count, 0]))
            pxy_h = np.ascontiguousarray(pts_h[:count, :2].reshape(2 * count, 8))
            dpxy_src, dpxy, dpinf = ctx.upload(pxy_h), ctx.empty((2 * count, 8)), ctx.upload(np.zeros(2 * count, dtype=np.uint8))
            dqxy, dqinf, dr = ctx.empty((2 * count, 8)), ctx.empty((2 * count,), dtype=np.uint8), ctx.empty((count, 4))
            qxy_h, qinf_h = np.zeros((2 * count, 8), dtype=np.uint64), np.zeros(2 * count, dtype=np.uint8)
            qxy_h[0::2] = pts_h[:count, 2]
            ct_h, cti_h = np.zeros((count, 8), dtype=np.uint64), np.zeros(count, dtype=np.uint8)
            # the loop's own arrays
            lw, le, lux = ctx.empty((count, nw, 4)), ctx.empty((count, m, 4)), ctx.empty((count, 1 + lx, 4))
            lt = ctx.empty((m, 4))
            ux2 = ctx.upload(np.ascontiguousarray(z2h[:count, :1 + lx]))
            loop_pts = []
            n = m                                          # the key has m generators: n = min(m, len(ck))
            ctx.sync()

            def reset():                                   # both variants fold in place: fresh copies of z1 and E (not timed)
                ctx.copy_d2d(dz1.ptr, dz1s.ptr, count * nz * 32)
                ctx.copy_d2d(de.ptr, d_e0.ptr, count * m * 32)
                ctx.copy_d2d(le.ptr, d_e0.ptr, count * m * 32)
                ctx.copy_d2d(dpxy.ptr, dpxy_src.ptr, 2 * count * 64)
                for b in range(count):
                    ctx.copy_d2d(lw.ptr + 32 * b * nw, dz1s.ptr + 32 * (b * nz + 1 + lx), nw * 32)
                    ctx.copy_d2d(lux.ptr + 32 * b * (1 + lx), dz1s.ptr + 32 * b * nz, (1 + lx) * 32)
                ctx.sync()

            def batch():
                ctx.nova_cross_term_batch(FR, mats[0], mats[1], mats[2], m, dz1.ptr, nz, dz2.ptr, nz, count, du1.ptr, 0, dt.ptr, m)
                ctx.commit_batch(G1, g.ptr, 0, dt.ptr, n, count, m, d_ct.ptr, d_cti.ptr)
                ct_h[:], cti_h[:] = d_ct.numpy(), d_cti.numpy()              # the phase's read-back; the transcript would run here
                qxy_h[1::2], qinf_h[1::2] = ct_h, cti_h
                ctx.write(dqxy.ptr, qxy_h)
                ctx.write(dqinf.ptr, qinf_h)
                ctx.write(dr.ptr, rs[:count])
                ctx.field_vec_axpy_batch(FR, dz1.ptr, nz, dr.ptr, dz2.ptr, nz, dz1.ptr, nz, nz, count)
                ctx.field_vec_axpy_batch(FR, de.ptr, m, dr.ptr, dt.ptr, m, de.ptr, m, m, count)
                ctx.points_muladd_batch(G1, dpxy.ptr, dpinf.ptr, dqxy.ptr, dqinf.ptr, dr.ptr, 2, 2 * count, dpxy.ptr, dpinf.ptr)
                ctx.sync()

            def fold_point(p1, p2, r):
                return ctx.msm_host(G1, np.stack([p1, p2]), np.zeros(2, dtype=np.uint8), np.stack([one, r]), 2)

            def loop():
                loop_pts.clear()
                for b in range(count):
                    r = rs[b]
                    ctx.nova_cross_term(FR, mats[0], mats[1], mats[2], m, dz1s.ptr + 32 * b * nz, dz2.ptr + 32 * b * nz, z1h[b, 0], one, lt.ptr)
                    cxy, cinf = ctx.commit(G1, g.ptr, 0, lt.ptr, n)
                    ctx.field_vec_axpy(FR, lw.ptr + 32 * b * nw, r, dz2.ptr + 32 * (b * nz + 1 + lx), lw.ptr + 32 * b * nw, nw)
                    ctx.field_vec_axpy(FR, le.ptr + 32 * b * m, r, lt.ptr, le.ptr + 32 * b * m, m)
                    ctx.field_vec_axpy(FR, lux.ptr + 32 * b * (1 + lx), r, ux2.ptr + 32 * b * (1 + lx), lux.ptr + 32 * b * (1 + lx), 1 + lx)
                    loop_pts.append(fold_point(pts_h[b, 0], pts_h[b, 2], r))
                    loop_pts.append(fold_point(pts_h[b, 1], cxy, r))
                ctx.sync()

            def cross_batch():
                ctx.nova_cross_term_batch(FR, mats[0], mats[1], mats[2], m, dz1s.ptr, nz, dz2.ptr, nz, count, du1.ptr, 0, dt.ptr, m)
                ctx.sync()

            def cross_loop():
                for b in range(count):
                    ctx.nova_cross_term(FR, mats[0], mats[1], mats[2], m, dz1s.ptr + 32 * b * nz, dz2.ptr + 32 * b * nz, z1h[b, 0], one, lt.ptr)
                ctx.sync()

            def axpy_batch():
                ctx.field_vec_axpy_batch(FR, dz1s.ptr, nz, dr.ptr, dz2.ptr, nz, dz1.ptr, nz, nz, count)
                ctx.sync()

            def axpy_loop():
                for b in range(count):
                    ctx.field_vec_axpy(FR, dz1s.ptr + 32 * b * nz, rs[b], dz2.ptr + 32 * b * nz, dz1.ptr + 32 * b * nz, nz)
                ctx.sync()

            def points_batch():
                ctx.points_muladd_batch(G1, dpxy_src.ptr, dpinf.ptr, dqxy.ptr, dqinf.ptr, dr.ptr, 2, 2 * count, dpxy.ptr, dpinf.ptr)
                ctx.sync()

            def points_loop():
                for j in range(2 * count):
                    fold_point(pxy_h[j], qxy_h[j], rs[j // 2])

            # the batch's results are the loop's
            reset(); batch()
            got_z, got_e, got_p = dz1.numpy(), de.numpy(), dpxy.numpy()
            assert not dpinf.numpy().any()
            reset(); loop()
            assert (got_e == le.numpy()).all() and (got_z[:, 1 + lx:] == lw.numpy()).all() and (got_z[:, :1 + lx] == lux.numpy()).all(), (m, count)
            assert all((got_p[j] == loop_pts[j][:8]).all() and loop_pts[j][8:].any() for j in range(2 * count)), (m, count)
            variants = [(batch, True), (loop, True), (cross_batch, False), (cross_loop, False), (axpy_batch, False), (axpy_loop, False), (points_batch, False),
                        (points_loop, False)]
            for _ in range(warm):
                for v, fresh in variants:
                    if fresh:
                        reset()
                    v()
            ts = [[] for _ in variants]
            for _ in range(reps):                          # alternating rounds
                for t, (v, fresh) in zip(ts, variants):
                    if fresh:
                        reset()
                    t.append(timed_us(v))
            st = [med_iqr(t) for t in ts]
            (ma, ia), (mb, ib) = st[:2]
            note = "batch faster by more than the spread" if mb - ma > max(ia, ib) else ("within the spread" if abs(mb - ma) <= max(ia, ib) else "batch SLOWER than the loop")
            line = f"{m:6d} {count:5d} {ma:11.1f} {ia:9.1f} {mb:11.1f} {ib:9.1f} {ma / mb:7.3f}"
            for k in (2, 4, 6):
                line += f" {st[k][0]:10.1f} {st[k][1]:8.1f} {st[k + 1][0]:10.1f} {st[k + 1][1]:8.1f}"
            rows.append(line + "  " + note)
            print(rows[-1], flush=True)
        ctx.bases_unregister(g.ptr)
        del keep, g, d_rs, d_e0, pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nova_fold_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cells", default="", help="m:count,... instead of the whole table")
    a = ap.parse_args()
    reps = max(a.reps, 20)
    cells = [(m, c) for m in SIZES for c in COUNTS]
    if a.cells:
        cells = [tuple(int(v) for v in item.split(":")) for item in a.cells.split(",")]
    gc.disable()                                           # no cyclic collection inside a timed loop
    ctx = K.Context(0)
    head = ("batched Nova fold timing (tools/dbg/nova_fold_batch_timing.py): chain circuit over Fr / G1, resident inputs, C-level entries; (a) = cross-term batch + "
            "commit batch + read-back of count points + upload of challenges and Q + two axpy batches + point batch + one sync, (b) = per pair kg_nova_cross_term + "
            "blocking kg_commit + three kg_field_vec_axpy + two two-point kg_msm_host, one sync at the end; then each primitive + one sync beside its single-call "
            f"loop; alternating rounds, medians of {reps} after {a.warm} warm-up rounds, wall clock, iqr = interquartile range of the rounds; m = 16384 runs "
            "kg_commit_batch's blocking loop")
    rows = [head, f"{'m':>6s} {'count':>5s} {'(a) us':>11s} {'iqr':>9s} {'(b) us':>11s} {'iqr':>9s} {'a/b':>7s} {'cross us':>10s} {'iqr':>8s} {'loop us':>10s} {'iqr':>8s}"
                  f" {'axpy us':>10s} {'iqr':>8s} {'loop us':>10s} {'iqr':>8s} {'points us':>10s} {'iqr':>8s} {'loop us':>10s} {'iqr':>8s}  note"]
    run_cells(ctx, cells, reps, a.warm, rows)
    text = "\n".join(rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
