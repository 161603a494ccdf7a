"""kg_ntt_bn254_fr_batch beside the loop it replaces, on one context and one buffer: for log_n in {4, 8, 10, 11, 12, 16, 20} and count in
{1, 8, 64, 256} (rows above 1 GiB of data are skipped), coset_dft in place on count dense transforms (stride = n), timed as
  (a) loop : count calls of kg_ntt_bn254_fr followed by one kg_ctx_sync -- the single-transform path, the baseline;
  (b) batch: one kg_ntt_bn254_fr_batch followed by one kg_ctx_sync.
The two are measured in alternating rounds (a, b, a, b, ...) so that a drift of the box meets both; every figure is the median of --reps
(>= 25) rounds after warm-up rounds, by a synchronised wall clock.  The gate: for log_n <= 11 and count >= 8 the batched median must be below
the loop's -- the loop is `count` dependent launches of one workgroup each, so a batch that does not beat it is broken, not slow.  The
exit status is 1 when a gated row misses.

    python tools/dbg/ntt_batch_time.py [--out profiles/ntt_batch_timing.txt] [--reps 25]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import kogarashi_amd as K  # noqa: E402
from kogarashi_amd import lib as L  # noqa: E402

SEED = 0x4B6F676172617368
LOGS = (4, 8, 10, 11, 12, 16, 20)
COUNTS = (1, 8, 64, 256)
MAX_BYTES = 1 << 30


def timed_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_batch_timing.txt"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    reps = max(a.reps, 25)
    ctx = K.Context(0)
    rows, missed = [], []
    rows.append(f"{'log_n':>5s} {'count':>5s} {'groups':>6s} {'loop median us':>15s} {'loop min..max us':>22s} {'batch median us':>16s} {'batch / loop':>12s}  note")
    for k in LOGS:
        n = 1 << k
        for count in COUNTS:
            if count * n * 32 > MAX_BYTES:
                rows.append(f"{k:5d} {count:5d}   skipped: {count * n * 32 / 2**30:.0f} GiB of data")
                continue
            d = ctx.empty((count * n, 4))
            ctx.gen_scalars(K.KG_FR, SEED + 16 * k + count, 0, count * n, d.ptr)
            ctx.sync()

            def loop():
                for b in range(count):
                    ctx.ntt(d.ptr + b * n * 32, k, False, True)
                ctx.sync()

            def batch():
                ctx.ntt_batch(d.ptr, k, count, n, False, True)
                ctx.sync()

            for _ in range(a.warm):
                loop()
                batch()
            tl, tb = [], []
            for _ in range(reps):                      # alternating rounds
                tl.append(timed_us(loop))
                tb.append(timed_us(batch))
            ml, mb = statistics.median(tl), statistics.median(tb)
            gated = k <= 11 and count >= 8
            note = ""
            if gated:
                note = "gate: met" if mb < ml else "gate: MISSED"
                if mb >= ml:
                    missed.append((k, count))
            elif k == 20 and count == 8:
                note = "batch median within the loop's min..max" if min(tl) <= mb <= max(tl) else (
                    "batch median below the loop's minimum" if mb < min(tl) else "batch median ABOVE the loop's maximum")
            rows.append(f"{k:5d} {count:5d} {L.ntt_batch_plan(k, count)[0]:6d} {ml:15.1f} {min(tl):10.1f}..{max(tl):<10.1f} {mb:16.1f} {mb / ml:12.3f}  {note}")
            del d
    head = ("kg_ntt_bn254_fr_batch timing (tools/dbg/ntt_batch_time.py): coset_dft, dense batches; loop = count calls of kg_ntt_bn254_fr + one sync, "
            f"batch = one call + one sync; alternating rounds, medians of {reps} after {a.warm} warm-up rounds, synchronised wall clock")
    tail = "gate (log_n <= 11, count >= 8: batch median < loop median): " + ("met on every row" if not missed else f"MISSED at {missed}")
    text = "\n".join([head] + rows + [tail]) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
