"""kg_r1cs_check beside its two yardsticks, on the same context and the same resident shape: kg_nova_cross_term (the fused kernel it is
modelled on: twice the row products) and the composition that was the only way to ask the question before -- three kg_r1cs_prod, a mul, a scale
and an add, two m x 32 B downloads and a numpy compare (its three m x 32 B temporaries allocated once, outside the clock).  Two workloads: the
chain circuit (rows of 1 / 2 / 1 entries) at 2^18 rows and a random shape (0..6 entries per row, 254-entry rows, a 200- and a 5000-entry row) at
2^20 rows.  E is made on the device so that every row holds (the check must answer (0, m)); a second line times it with every 1000th row broken.
Every figure is the median of --reps (>= 20) blocking calls after warm-up, by a synchronised wall clock.

    python tools/dbg/r1cs_check_time.py [--out profiles/r1cs_check_timing.txt] [--reps 25]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import kogarashi_amd as K  # noqa: E402

SEED = 0x4B6F676172617368
FD = K.KG_FR


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def mont_one(ctx):
    d = ctx.upload(np.array([[1, 0, 0, 0]], dtype=np.uint64))
    ctx.field_vec_op(FD, "to_mont", d.ptr, 0, d.ptr, 1)
    return d.numpy()[0].copy()


def chain_shape(ctx, m):
    """t_{i+1} = t_i (t_i + 1): A = t_i, B = t_i + 1, C = t_{i+1} over z = (1 | t_0 | t_1 .. t_m)"""
    one = mont_one(ctx)
    wire = np.arange(1, m + 1, dtype=np.uint64)
    b_col = np.zeros(2 * m, dtype=np.uint64)
    b_col[0::2] = wire
    mats = [(np.arange(m + 1, dtype=np.uint64), wire, np.tile(one, (m, 1))),
            (np.arange(0, 2 * m + 1, 2, dtype=np.uint64), b_col, np.tile(one, (2 * m, 1))),
            (np.arange(m + 1, dtype=np.uint64), wire + np.uint64(1), np.tile(one, (m, 1)))]
    return [tuple(ctx.upload(np.ascontiguousarray(a)) for a in t) for t in mats], m + 2


def random_shape(ctx, m):
    rng = np.random.default_rng(7)
    nvars = m // 2
    out = []
    for j in range(3):
        counts = rng.integers(0, 7, m)
        counts[7] = 200
        counts[1000 + j::4099] = 254                     # range-check-like rows, at different constraints in A, B and C
        counts[61] = 5000 if j == 1 else counts[61]
        rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        nnz = int(rp[-1])
        col = rng.integers(0, nvars, nnz).astype(np.uint64)
        val = ctx.empty((nnz, 4))
        ctx.gen_scalars(FD, SEED + 20 + j, 0, nnz, val.ptr)
        out.append((ctx.upload(rp), ctx.upload(col), val))
    return out, nvars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check_timing.txt"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--log-chain", type=int, default=18)
    ap.add_argument("--log-random", type=int, default=20)
    a = ap.parse_args()
    reps = max(a.reps, 20)
    ctx = K.Context(0)
    rows = []
    for name, make, lg in (("chain circuit", chain_shape, a.log_chain), ("random shape with long rows", random_shape, a.log_random)):
        m = 1 << lg
        dev, nvars = make(ctx, m)
        ptrs = [tuple(d.ptr for d in t) for t in dev]
        nnz = sum(t[1].shape[0] for t in dev)
        z, z2 = ctx.empty((nvars, 4)), ctx.empty((nvars, 4))
        ctx.gen_scalars(FD, SEED + 1, 0, nvars, z.ptr)
        ctx.gen_scalars(FD, SEED + 2, 0, nvars, z2.ptr)
        u = ctx.empty((1, 4))
        ctx.gen_scalars(FD, SEED + 3, 0, 1, u.ptr)
        u = u.numpy()[0].copy()
        az, bz, cz, e, out = (ctx.empty((m, 4)) for _ in range(5))
        status = ctx.empty((m,), dtype=np.uint8)

        def composition(e_dev):
            for p, o in zip(ptrs, (az, bz, cz)):
                ctx.r1cs_prod(FD, p[0], p[1], p[2], m, z.ptr, o.ptr)
            ctx.field_vec_op(FD, "mul", az.ptr, bz.ptr, az.ptr, m)
            ctx.field_vec_scale(FD, cz.ptr, u, cz.ptr, m)
            ctx.field_vec_op(FD, "add", cz.ptr, e_dev.ptr, cz.ptr, m)
            return bool((az.numpy() == cz.numpy()).all())

        # E := Az o Bz - u Cz, so that every row holds
        for p, o in zip(ptrs, (az, bz, cz)):
            ctx.r1cs_prod(FD, p[0], p[1], p[2], m, z.ptr, o.ptr)
        ctx.field_vec_op(FD, "mul", az.ptr, bz.ptr, e.ptr, m)
        ctx.field_vec_scale(FD, cz.ptr, u, cz.ptr, m)
        ctx.field_vec_op(FD, "sub", e.ptr, cz.ptr, e.ptr, m)
        ctx.sync()
        assert ctx.r1cs_check(FD, *ptrs, m, z.ptr, u, e.ptr, status.ptr) == (0, m) and composition(e)
        eb = e.numpy()
        eb[::1000, 0] ^= np.uint64(1)
        eb = ctx.upload(eb)
        assert ctx.r1cs_check(FD, *ptrs, m, z.ptr, u, eb.ptr) == ((m + 999) // 1000, 0) and not composition(eb)

        def cross():
            ctx.nova_cross_term(FD, *ptrs, m, z.ptr, z2.ptr, u, u, out.ptr)
            ctx.sync()

        def line(what, fn, note=""):
            med, lo = median_ms(fn, reps)
            rows.append(f"{what:<66s} median {med:9.3f} ms   min {lo:9.3f} ms   {note}")

        rows.append(f"-- {name}: 2^{lg} rows, {nnz} matrix entries in A, B, C")
        line("kg_r1cs_check, relaxed (u, E), no status array", lambda: ctx.r1cs_check(FD, *ptrs, m, z.ptr, u, e.ptr))
        line("kg_r1cs_check, relaxed (u, E), status array", lambda: ctx.r1cs_check(FD, *ptrs, m, z.ptr, u, e.ptr, status.ptr))
        line("kg_r1cs_check, relaxed, every 1000th row broken", lambda: ctx.r1cs_check(FD, *ptrs, m, z.ptr, u, eb.ptr))
        line("kg_r1cs_check, plain (u = 1, E = 0: nearly every row fails)", lambda: ctx.r1cs_check(FD, *ptrs, m, z.ptr))
        line("kg_nova_cross_term, same shape (+ sync)", cross)
        line("3 kg_r1cs_prod + mul + scale + add + 2 downloads + compare", lambda: composition(e), note=f"{64 * m / 2**20:.0f} MiB downloaded")
    text = "\n".join(["kg_r1cs_check timing (tools/dbg/r1cs_check_time.py): blocking calls, synchronised wall clock, "
                      f"median and minimum of {reps} calls after 3 warm-up calls"] + rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
