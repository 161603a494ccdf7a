"""kg_points_check at the bench's proof size: the G1 curve check over 2^20 points, the G2 curve check and the G2 subgroup check over 2^18,
beside two yardsticks from the same run -- kg_bases_register of the same arrays (the call the check precedes) and the blocking G2 MSM of
2^18 pairs.  Every figure is the median of --reps (>= 20) blocking calls after warm-up, by a synchronised wall clock (the check reads its
two summary words back, so a call's wall time is its device time plus one round trip).

    python tools/dbg/points_check_time.py [--out profiles/points_check_timing.txt] [--reps 25]
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


def median_ms(fn, reps, warm=3, after=None):
    for _ in range(warm):
        fn()
        if after:
            after()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after:
            after()
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_check_timing.txt"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--log-g1", type=int, default=20)
    ap.add_argument("--log-g2", type=int, default=18)
    a = ap.parse_args()
    reps = max(a.reps, 20)
    ctx = K.Context(0)
    n1, n2 = 1 << a.log_g1, 1 << a.log_g2
    g1 = ctx.empty((n1, 8))
    ctx.gen_bases(K.KG_G1, SEED, 0, n1, g1.ptr)
    k = ctx.empty((n2, 4))
    ctx.gen_scalars(K.KG_FR, SEED + 1, 0, n2, k.ptr)
    g2, g2_inf = ctx.empty((n2, 16)), ctx.empty((n2,), dtype=np.uint8)
    ctx.fixed_base_mul(K.KG_G2, k.ptr, n2, g2.ptr, g2_inf.ptr)
    s = ctx.empty((n2, 4))
    ctx.gen_scalars(K.KG_FR, SEED + 2, 0, n2, s.ptr)
    st1, st2 = ctx.empty((n1,), dtype=np.uint8), ctx.empty((n2,), dtype=np.uint8)
    ctx.sync()
    both = K.KG_CHECK_CURVE | K.KG_CHECK_SUBGROUP
    assert ctx.points_check(K.KG_G1, g1.ptr, 0, n1, both, st1.ptr) == (0, n1)
    assert ctx.points_check(K.KG_G2, g2.ptr, 0, n2, both, st2.ptr) == (0, n2)
    rows = []

    def row(name, fn, after=None, note=""):
        med, lo = median_ms(fn, reps, after=after)
        rows.append(f"{name:<58s} median {med:9.3f} ms   min {lo:9.3f} ms   {note}")

    row(f"G1 curve check, 2^{a.log_g1} points", lambda: ctx.points_check(K.KG_G1, g1.ptr, 0, n1, K.KG_CHECK_CURVE, st1.ptr),
        note=f"{64 * n1 / 1e6:.0f} MB read")
    row(f"G2 curve check, 2^{a.log_g2} points", lambda: ctx.points_check(K.KG_G2, g2.ptr, 0, n2, K.KG_CHECK_CURVE, st2.ptr),
        note=f"{128 * n2 / 1e6:.0f} MB read")
    row(f"G2 curve + subgroup check, 2^{a.log_g2} points", lambda: ctx.points_check(K.KG_G2, g2.ptr, 0, n2, both, st2.ptr))

    def reg(curve, d, n):
        def f():
            ctx.bases_register(curve, d.ptr, 0, n)
            ctx.sync()
        return f

    row(f"kg_bases_register, G1 2^{a.log_g1} (+ sync)", reg(K.KG_G1, g1, n1), after=lambda: ctx.bases_unregister(g1.ptr))
    row(f"kg_bases_register, G2 2^{a.log_g2} (+ sync)", reg(K.KG_G2, g2, n2), after=lambda: ctx.bases_unregister(g2.ptr))
    ctx.bases_register(K.KG_G2, g2.ptr, 0, n2)
    ctx.set_inputs_complete(True)
    row(f"blocking kg_msm, G2 2^{a.log_g2} pairs, registered bases", lambda: ctx.msm(K.KG_G2, g2.ptr, 0, s.ptr, n2))
    ctx.bases_unregister(g2.ptr)
    text = "\n".join(["kg_points_check timing (tools/dbg/points_check_time.py): blocking calls, synchronised wall clock, "
                      f"median and minimum of {reps} calls after 3 warm-up calls"] + rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
