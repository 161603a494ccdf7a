"""Reference, case builders and checkers for the integer kernels of the long MSM's scalar side (csrc/msm_sort_kernels.h, msm_task_kernels.h,
msm_level_kernels.h), which tests/device/devprobe_sort.h launches one at a time (tests/test_gpu_sort_kernels.py).

Pure numpy and Python integers, importable without a GPU (tests/test_sort_cases_host.py runs the census of the cases and feeds every checker
mutated outputs here).  The reference is written from the documented meaning of the tables, not from the kernels:

  digits   H = sum_{w < W-1} 2^(wc + c-1), e_w = ((k + H) >> wc) mod 2^c, signed digit d_w = e_w - 2^(c-1); the top window is the unsigned rest
           (17 bits).  sum_w d_w 2^(wc) = k is asserted for every scalar a case uses.  Bucket of a digit: |d| - 1; the entry carries the sign.
  tasks    (msm_common.h) a window's task length T carries hot_shift in its top two bits; a bucket of v entries is cut into tasks of
           t = T & 0x3fffffff entries, or of t >> hot_shift if v > 32 t (a hot bucket); T_top applies to window top_w.

Every table a kernel READS is the reference's, so each kernel is judged alone.  Every comparison is exact.  Output buffers carry a guard
region behind the owned words (OBuf); the checkers look at the guard of every buffer they are given."""
import ctypes as C
import random

import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001      # Fr
Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47      # Fq
MODULUS = {0: R_MOD, 1: Q_MOD}

GUARD = 64                       # guard elements behind every output buffer
FILL = 0xA5C3F00D                # what an owned word holds before the launch
GFILL = 0x5EED6A4D               # what a guard word holds
MULTI_SEG = 0x80000000
SEG = 8192
GATHER_SUM_MAX = 32
LEN_BINS = 256
T_MASK = 0x3FFFFFFF
BIG, BIG_CAP = 16, 64
PREP_CH = 4096

SORT_EXPORTS = ["dp_sort_prep", "dp_sort_onepass", "dp_sort_zero_fill", "dp_sort_group_scan", "dp_sort_merge_groups", "dp_sort_group_scatter_big",
                "dp_sort_fine_local", "dp_sort_fine_scatter", "dp_task_bucket_tables", "dp_task_bases", "dp_task_len_scatter", "dp_level_ops"]


def seg_len(fb):
    return 20480 if fb == 9 else SEG


# ---------------------------------------------------------------------------------------------------------------------------------------------
# buffers and the call into the probe library
# ---------------------------------------------------------------------------------------------------------------------------------------------
class OBuf:
    """an output buffer: `words` owned elements (filled with `fill`, or a copy of `init`) and GUARD guard elements behind them"""

    def __init__(self, words, fill=FILL, dtype=np.uint32, init=None):
        self.words = int(words)
        self.a = np.empty(self.words + GUARD, dtype=dtype)
        self.a[:self.words] = fill if init is None else np.asarray(init, dtype=dtype).reshape(-1)
        self.a[self.words:] = GFILL
        self.fill = fill

    @property
    def own(self):
        return self.a[:self.words]

    def guard_ok(self):
        return bool((self.a[self.words:] == GFILL).all())


class KBuf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("bytes", C.c_uint64), ("io", C.c_uint32), ("reserved", C.c_uint32)]


class DeviceError(RuntimeError):
    """a HIP status from a probe entry: the device may have faulted, so the caller starts nothing more on it"""


def call(dev, name, bufs, params):
    """bufs: numpy arrays (inputs), OBufs (copied back) or None (a null pointer); params: integers.  Fails on any status but 0."""
    kb = (KBuf * len(bufs))()
    keep = []
    for i, b in enumerate(bufs):
        if b is None:
            kb[i] = KBuf(None, 0, 0, 0)
            continue
        a = b.a if isinstance(b, OBuf) else np.ascontiguousarray(b)
        keep.append(a)
        kb[i] = KBuf(a.ctypes.data, a.nbytes, 1 if isinstance(b, OBuf) else 0, 0)
    pa = (C.c_int64 * max(len(params), 1))(*[int(v) for v in params])
    fn = getattr(dev, name)
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(KBuf), C.POINTER(C.c_int64)]
    st = fn(kb, pa)
    if st > 0:
        raise DeviceError(f"{name}: HIP status {st}")
    assert st == 0, f"{name}: refused with {st} (-1: a parameter, -2: a buffer shorter than the launch needs)"


def check_guards(out, what=""):
    bad = [k for k, b in out.items() if isinstance(b, OBuf) and not b.guard_ok()]
    assert not bad, f"{what}: guard region touched behind {bad}"


def excl(a, axis=-1):
    a = np.asarray(a, dtype=np.int64)
    return np.cumsum(a, axis=axis) - a


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def canon(vals, labels):
    """the values ordered by (label, value): equal for two arrays iff every label holds the same multiset"""
    return np.asarray(vals)[np.lexsort((vals, labels))]


def check_runs(row, starts, sizes, exp_vals, exp_labels, fill, what):
    """run r = row[starts[r] : starts[r] + sizes[r]] holds, as a multiset, the exp_vals whose label is r; every other element of row still
    holds `fill`.  starts / sizes are the reference's."""
    starts, sizes = np.asarray(starts, dtype=np.int64).reshape(-1), np.asarray(sizes, dtype=np.int64).reshape(-1)
    total = int(sizes.sum())
    pos = np.repeat(starts, sizes) + np.arange(total) - np.repeat(excl(sizes), sizes)
    assert total == 0 or (pos.min() >= 0 and pos.max() < len(row) and len(np.unique(pos)) == total), f"{what}: the reference's runs overlap"
    labels = np.repeat(np.arange(len(sizes)), sizes)
    exp_vals, exp_labels = np.asarray(exp_vals), np.asarray(exp_labels)
    assert len(exp_vals) == total, f"{what}: the reference's sizes and entries disagree"
    got, want = canon(row[pos], labels), canon(exp_vals.astype(row.dtype), exp_labels)
    if not np.array_equal(got, want):
        j = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{what}: run {int(np.sort(labels)[j])} holds {int(got[j]):#x}, expected {int(want[j]):#x} (first of {int((got != want).sum())})")
    rest = np.ones(len(row), dtype=bool)
    rest[pos] = False
    assert (row[rest] == fill).all(), f"{what}: {int((row[rest] != fill).sum())} words outside the runs were written"


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    if not np.array_equal(got, want.astype(got.dtype)):
        j = int(np.nonzero(got != want.astype(got.dtype))[0][0])
        raise AssertionError(f"{what}: word {j} is {int(got[j]):#x}, expected {int(want[j]):#x} ({int((got != want.astype(got.dtype)).sum())} differ)")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# digits
# ---------------------------------------------------------------------------------------------------------------------------------------------
def windows(c):
    return (255 + c - 1) // c


def bias(c):
    return sum(1 << (w * c + c - 1) for w in range(windows(c) - 1))


def bias_words(c):
    H = bias(c)
    return np.array([(H >> (32 * j)) & 0xFFFFFFFF for j in range(8)], dtype=np.uint32)


class Digits:
    """the biased words and the signed digits of a list of scalars for a window width c"""

    def __init__(self, ks, c):
        self.ks, self.c, self.W, self.n = list(ks), c, windows(c), len(ks)
        H, W, half, mask = bias(c), self.W, 1 << (c - 1), (1 << c) - 1
        es = [k + H for k in self.ks]
        assert all(0 <= k and e < (1 << 256) for k, e in zip(self.ks, es))
        self.kt = np.frombuffer(b"".join(e.to_bytes(32, "little") for e in es), dtype="<u4").reshape(self.n, 8).T.copy()     # [8][n]
        d = np.empty((W, self.n), dtype=np.int64)
        for i, e in enumerate(es):
            acc = 0
            for w in range(W - 1):
                dw = ((e >> (w * c)) & mask) - half
                d[w, i] = dw
                acc += dw << (w * c)
            top = e >> ((W - 1) * c)
            assert top < (1 << 17) and top <= half, "the top window does not fit its buckets"
            d[W - 1, i] = top
            assert acc + (top << ((W - 1) * c)) == self.ks[i], "digits do not recompose the scalar"
        self.d = d
        self.m = np.abs(d)                                   # 0: skipped; bucket = m - 1
        self.neg = d < 0

    def entries(self, w):
        """(index | sign << 31, bucket) of the scalars with a non-zero digit in window w"""
        sel = np.nonzero(self.m[w])[0]
        return (sel | (self.neg[w][sel].astype(np.int64) << 31)).astype(np.uint32), self.m[w][sel] - 1, sel

    def hist(self, nch, chunk_len, shift):
        """[W][nch][B >> shift] entries per (window, chunk, bucket >> shift)"""
        nb = (1 << (self.c - 1)) >> shift
        h = np.zeros((self.W, nch, nb), dtype=np.int64)
        ch = np.arange(self.n) // chunk_len
        assert self.n == 0 or ch.max() < nch
        for w in range(self.W):
            _, bk, sel = self.entries(w)
            np.add.at(h[w], (ch[sel], bk >> shift), 1)
        return h


def scalar_values(field, c):
    """the edge scalars of a field for a window width: 0, 1, r - 1, 2^k and 2^k - 1 at every window boundary, sums that carry through all
    eight words of k + H, every digit -2^(c-1) (the largest bucket of every signed window), every digit 0"""
    r, W, H = MODULUS[field], windows(c), bias(c)
    v = [0, 1, r - 1, r - 2, 2, (1 << 254) - 1 if (1 << 254) - 1 < r else r - 3]
    for w in range(1, W):
        for k in ((1 << (w * c)), (1 << (w * c)) - 1, (1 << (w * c)) + 1, 1 << (w * c - 1)):
            if k < r:
                v.append(k)
    hl = H & ((1 << 224) - 1)
    carry = (1 << 224) - hl                                  # k + H: every word below the top one overflows into the next
    v += [carry, carry - 1, carry + 1, carry + (1 << 250), (1 << 32) - (H & 0xFFFFFFFF)]
    v.append((1 << ((W - 1) * c)) - H)                       # e_w = 0 in every signed window: digit -2^(c-1); top digit 1
    two = (2 << ((W - 1) * c)) - H                           # the same with top digit 2, where the field and the top window's buckets hold it
    if two < r and c > 2:
        v.append(two)
    assert all(0 <= k < r for k in v)
    return v


def scalar_set(field, c, n, seed, kind="mix"):
    """n scalars: `mix` = the edge values, then uniform random ones, shuffled; `zero` / `largest` = one repeated value (every digit 0 / every
    signed digit -2^(c-1)); `uniform`"""
    r, W, H = MODULUS[field], windows(c), bias(c)
    rng = random.Random(seed * 1000003 + c * 131 + field)
    if kind == "zero":
        return [0] * n
    if kind == "largest":
        return [(1 << ((W - 1) * c)) - H] * n
    pool = [rng.randrange(r) for _ in range(min(n, 3000))]
    if kind == "mix":
        pool = scalar_values(field, c) + pool
    ks = [pool[i % len(pool)] for i in range(n)]
    if n >= len(pool):
        rng.shuffle(ks)
    return ks


def scalars_to_words(ks, to_mont):
    """(n, 4) uint64: the scalars in the form the C ABI takes, each chosen integer converted by `to_mont` (the oracle's f_to_mont on four limbs)"""
    cache, out = {}, np.empty((len(ks), 4), dtype=np.uint64)
    for i, k in enumerate(ks):
        if k not in cache:
            cache[k] = np.asarray(to_mont(np.array([(k >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)), dtype=np.uint64)
        out[i] = cache[k]
    return out


# ---- prep ---------------------------------------------------------------------------------------------------------------------------------
PREP_NS = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5]


def prep_cases():
    """(field, c, n, kind, seed) for k_prep_scalars: every n of the list, both fields, the edge mix"""
    out = []
    for field in (0, 1):
        for j, n in enumerate(PREP_NS):
            out.append((field, [16, 15, 13, 8, 5, 2, 17, 20][j], n, "mix", j))
        out += [(field, 16, 300, "zero", 9), (field, 16, 300, "largest", 10), (field, 13, 1000, "uniform", 11)]
    return out


def prep_count_cases():
    """(field, c, fb, n, chunk_len, nch, kind, seed) for k_prep_scalars_count; chunk_len is a multiple of 4096 and does not divide n; chunk
    counts 1, 2, 3, 8, 9.  Each runs with per_wg = 4096 and 1024."""
    return [(0, 12, 7, 4097, 8192, 1, "mix", 1), (1, 16, 7, 4096 + 4095, 4096, 2, "mix", 2), (0, 17, 7, 3 * 4096 + 5, 8192, 2, "mix", 3),
            (1, 18, 7, 2 * 4096 + 257, 4096, 3, "mix", 4), (0, 19, 9, 7 * 4096 + 255, 4096, 8, "mix", 5), (1, 20, 9, 8 * 4096 + 1, 4096, 9, "mix", 6),
            (0, 16, 7, 5000, 8192, 1, "largest", 7), (0, 16, 7, 5000, 8192, 1, "zero", 8), (1, 12, 7, 1, 4096, 1, "mix", 9)]


def check_prep(out, dg, what="prep"):
    check_guards(out, what)
    same(out["kt"].own, dg.kt, f"{what}: kt")


def check_prep_count(out, dg, fb, nch, chunk_len, what="prep_count"):
    check_guards(out, what)
    same(out["kt"].own, dg.kt, f"{what}: kt")
    same(out["cnt"].own, dg.hist(nch, chunk_len, fb), f"{what}: cnt")


# ---- one-pass sort ------------------------------------------------------------------------------------------------------------------------
def onepass_cases():
    """(field, c, n, nch, kind, seed): every one-pass width (c = 15, 16: 64 and 128 KiB of LDS), chunk counts 1, 2, 3, 8, 9 with a chunk length
    that does not divide n"""
    return [(0, 2, 257, 2, "mix", 1), (1, 5, 1, 1, "mix", 2), (0, 5, 4097, 9, "mix", 3), (1, 8, 4095, 8, "mix", 4), (0, 13, 3 * 4096 + 5, 3, "mix", 5),
            (1, 15, 4097, 2, "mix", 6), (0, 16, 3 * 4096 + 5, 3, "mix", 7), (1, 16, 255, 1, "largest", 8), (0, 15, 256, 1, "zero", 9),
            (0, 8, 4096, 3, "uniform", 10)]


class OnePass:
    def __init__(self, dg, nch):
        self.dg, self.nch, self.n, self.W, self.c = dg, nch, dg.n, dg.W, dg.c
        self.B = 1 << (dg.c - 1)
        self.chunk_len = (dg.n + nch - 1) // nch
        if nch > 1 and dg.n % self.chunk_len == 0:
            self.chunk_len += 1
        assert self.chunk_len * nch >= dg.n
        self.hist = dg.hist(nch, self.chunk_len, 0)           # [W][nch][B]
        self.prefix = excl(self.hist, axis=1)
        self.bsize = self.hist.sum(axis=1)                     # [W][B]
        self.bstart = excl(self.bsize, axis=1)

    def model_sorted(self):
        rows = np.full((self.W, self.n), FILL, dtype=np.uint32)
        for w in range(self.W):
            val, bk, _ = self.dg.entries(w)
            rows[w, :len(val)] = val[::-1][np.argsort(bk[::-1], kind="stable")]      # bucket order, descending index inside a bucket
        return rows

    def check_count(self, out, what="k_count"):
        check_guards(out, what)
        same(out["cnt"].own, self.hist, f"{what}: cnt")

    def check_scan(self, out, what="k_scan_chunks"):
        check_guards(out, what)
        same(out["cnt"].own, self.prefix, f"{what}: prefix over chunks")
        same(out["bsize"].own, self.bsize, f"{what}: bsize")

    def check_scatter(self, out, what="k_scatter"):
        check_guards(out, what)
        rows = out["sorted"].own.reshape(self.W, self.n)
        for w in range(self.W):
            val, bk, _ = self.dg.entries(w)
            check_runs(rows[w], self.bstart[w], self.bsize[w], val, bk, FILL, f"{what}: window {w}")


# ---- k_group_scan / k_merge_groups --------------------------------------------------------------------------------------------------------
class GroupScanCase:
    """synthetic (window, chunk, group) counters whose group totals are chosen: 0, 1, seg - 1, seg, seg + 1, 2 seg, 2 seg + 1, 3 seg + 7 ..."""

    def __init__(self, name, W, nch, G, B, seg, sizes, seed, zwords=0, extra_bsize=8):
        rng = np.random.RandomState(seed)
        self.name, self.W, self.nch, self.G, self.B, self.seg, self.zwords = name, W, nch, G, B, seg, zwords
        self.nt = 512 if G > 256 else 256
        gs = np.asarray(sizes, dtype=np.int64).reshape(W, G)
        cnt = np.zeros((W, nch, G), dtype=np.int64)
        for w in range(W):                                   # split every group total over the chunks at random
            for g in np.nonzero(gs[w])[0]:
                cuts = np.sort(rng.randint(0, gs[w, g] + 1, nch - 1)) if nch > 1 else np.zeros(0, dtype=np.int64)
                cnt[w, :, g] = np.diff(np.concatenate([[0], cuts, [gs[w, g]]]))
        self.cnt, self.gsize = cnt, gs
        self.extra_bsize = extra_bsize
        # reference
        self.prefix = excl(cnt, axis=1)
        self.gstart = excl(gs, axis=1)
        nseg = (gs + seg - 1) // seg
        self.segbase = np.zeros((W, G + 1), dtype=np.int64)
        self.segbase[:, :G] = excl(nseg, axis=1)
        self.multi = (gs > seg).any(axis=1)
        self.segbase[:, G] = nseg.sum(axis=1) | np.where(self.multi, MULTI_SEG, 0)

    def buffers(self):
        W, G, B = self.W, self.G, self.B
        return {"cnt": OBuf(self.cnt.size, init=self.cnt), "gsize": OBuf(W * G), "gstart": OBuf(W * G), "segbase": OBuf(W * (G + 1)),
                "bsize": OBuf(W * B + self.extra_bsize), "zero": OBuf(self.zwords + 5)}

    def model(self):
        o = self.buffers()
        o["cnt"].own[:] = self.prefix.reshape(-1)
        o["gsize"].own[:] = self.gsize.reshape(-1)
        o["gstart"].own[:] = self.gstart.reshape(-1)
        o["segbase"].own[:] = self.segbase.reshape(-1)
        o["bsize"].own[:self.W * self.B] = 0
        o["zero"].own[:self.zwords] = 0
        return o

    def check(self, out, what="k_group_scan"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        W, B = self.W, self.B
        same(out["cnt"].own, self.prefix, f"{what}: prefix over chunks")
        same(out["gsize"].own, self.gsize, f"{what}: gsize")
        same(out["gstart"].own, self.gstart, f"{what}: gstart")
        sb = out["segbase"].own.reshape(W, self.G + 1)
        same(sb[:, :self.G], self.segbase[:, :self.G], f"{what}: segbase")
        same(sb[:, self.G] & ~np.uint32(MULTI_SEG), self.segbase[:, self.G] & ~MULTI_SEG, f"{what}: segment total")
        same((sb[:, self.G] & np.uint32(MULTI_SEG)) != 0, self.multi, f"{what}: MULTI_SEG")
        assert not out["bsize"].own[:W * B].any(), f"{what}: bsize not cleared"
        assert (out["bsize"].own[W * B:] == FILL).all(), f"{what}: words behind the windows' bsize were written"
        assert not out["zero"].own[:self.zwords].any(), f"{what}: the zero words were not cleared"
        assert (out["zero"].own[self.zwords:] == FILL).all(), f"{what}: words behind zwords were written"


def _edge_sizes(seg):
    return [0, 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 3 * seg + 7]


def _place(G, sizes, slots):
    row = [0] * G
    for s, v in zip(slots, sizes):
        row[s] = v
    return row


def group_scan_cases():
    out = []
    for seg in (SEG, 20480):
        e = _edge_sizes(seg)
        # window 0: all eight edge sizes with runs of empty groups around them; window 1: nothing above seg (no MULTI_SEG); window 2: empty
        out.append(GroupScanCase(f"G16 seg{seg}", 3, 3, 16, 2048, seg, [_place(16, e, [2, 3, 4, 7, 8, 11, 12, 13]), _place(16, [seg, 5, seg - 1], [0, 9, 15]), [0] * 16],
                                 seg, zwords=16 + 512))
    rng = np.random.RandomState(5)
    out.append(GroupScanCase("G256 nch9", 2, 9, 256, 1 << 15, SEG, [rng.randint(0, 70, 256), _place(256, [SEG + 1], [255])], 6, zwords=3))
    out.append(GroupScanCase("G512 nch8 (512 threads)", 2, 8, 512, 1 << 16, SEG, [rng.randint(0, 40, 512), _place(512, [SEG, 1, SEG + 1], [0, 300, 511])], 7, zwords=0))
    out.append(GroupScanCase("G1024 nch17", 1, 17, 1024, 1 << 17, SEG, [rng.randint(0, 30, 1024)], 8, zwords=528))
    out.append(GroupScanCase("G512 FB9 nch1", 1, 1, 512, 1 << 18, 20480, [_place(512, [20480, 20481], [100, 101])], 9, zwords=1))
    out.append(GroupScanCase("G1024 FB9 nch2", 1, 2, 1024, 1 << 19, 20480, [rng.randint(0, 25, 1024)], 10, zwords=64))
    return out


class MergeCase:
    """k_merge_groups: per-window group sizes -> one run per group over all windows (segments of SEG entries)"""

    def __init__(self, name, W, G, gsize):
        self.name, self.W, self.G = name, W, G
        self.gsize = np.asarray(gsize, dtype=np.int64).reshape(W, G)
        self.woff = excl(self.gsize, axis=0)
        self.gsize_m = self.gsize.sum(axis=0)
        self.gstart_m = excl(self.gsize_m)
        nseg = (self.gsize_m + SEG - 1) // SEG
        self.multi = bool((self.gsize_m > SEG).any())
        self.segbase_m = np.concatenate([excl(nseg), [int(nseg.sum()) | (MULTI_SEG if self.multi else 0)]])

    def buffers(self):
        return {"woff": OBuf(self.W * self.G), "gsize_m": OBuf(self.G), "gstart_m": OBuf(self.G), "segbase_m": OBuf(self.G + 1)}

    def model(self):
        o = self.buffers()
        for k in o:
            o[k].own[:] = getattr(self, k).reshape(-1)
        return o

    def check(self, out, what="k_merge_groups"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        for k in ("woff", "gsize_m", "gstart_m"):
            same(out[k].own, getattr(self, k), f"{what}: {k}")
        same(out["segbase_m"].own[:self.G], self.segbase_m[:self.G], f"{what}: segbase_m")
        assert bool(out["segbase_m"].own[self.G] & MULTI_SEG) == self.multi, f"{what}: MULTI_SEG"
        same(out["segbase_m"].own[self.G:] & ~np.uint32(MULTI_SEG), self.segbase_m[self.G:] & ~MULTI_SEG, f"{what}: segment total")


def merge_cases():
    rng = np.random.RandomState(11)
    a = rng.randint(0, 300, (16, 256))
    a[:, 7] = 512                                            # 16 windows x 512 = exactly SEG
    a[:, 8] = 512
    a[15, 8] = 513                                           # SEG + 1
    a[:, 100:140] = 0                                        # a run of empty groups
    b = rng.randint(0, 40, (15, 512))                        # nothing reaches SEG: no MULTI_SEG
    return [MergeCase("c16 W16 G256", 16, 256, a), MergeCase("c17 W15 G512", 15, 512, b), MergeCase("W1 G1024", 1, 1024, rng.randint(0, 3, (1, 1024)) * SEG)]


# ---- k_group_scatter_big ------------------------------------------------------------------------------------------------------------------
GS_PAIRS = [(4096, 256), (4096, 512), (4096, 1024), (8192, 256), (8192, 512), (8192, 1024)]


def ent(fb, idx_tag, fine, neg):
    idx_tag, fine, neg = np.asarray(idx_tag, dtype=np.uint64), np.asarray(fine, dtype=np.uint64), np.asarray(neg, dtype=np.uint64)
    if fb == 7:
        return (idx_tag | (fine << np.uint64(24)) | (neg << np.uint64(31))).astype(np.uint32)
    return (fine << np.uint64(32)) | idx_tag | (neg << np.uint64(31))


def ent_fine(fb, e):
    return ((e >> 24) & 127) if fb == 7 else (e >> np.uint64(32))


def ent_out(fb, e):
    return (e & np.uint32(0x80FFFFFF)).astype(np.uint32) if fb == 7 else (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def ent_dtype(fb):
    return np.uint32 if fb == 7 else np.uint64


def ent_fill(fb):
    return FILL if fb == 7 else (FILL << 32) | 0x0BADF00D


def group_scatter_cases():
    """(field, c, fb, G, n, nch, chunk_len, merged, w0, gridw, tile, nt, kind, seed).  All six (c, FB, G) shapes of the two-pass sort, all six
    (TILE, NT) kernels for both entry widths, a window group (w0 > 0, a grid narrower than W), merged sorts at c = 16 and 17."""
    out, k = [], 0
    shapes = [(12, 7, 16), (16, 7, 256), (17, 7, 512), (18, 7, 1024), (19, 9, 512), (20, 9, 1024)]
    for j, (c, fb, G) in enumerate(shapes):
        W = windows(c)
        tile, nt = GS_PAIRS[j]
        out.append((j & 1, c, fb, G, 3 * 4096 + 5, 3, 5000, False, 0, W, tile, nt, "mix", 20 + j))
    for fb, c, G in ((7, 16, 256), (9, 19, 512)):
        for tile, nt in GS_PAIRS:
            W = windows(c)
            out.append((k & 1, c, fb, G, 8192 + 4097, 2, 8200, False, 3, W - 5, tile, nt, "mix", 40 + k))
            k += 1
    out.append((0, 16, 7, 256, 3 * 4096 + 5, 3, 4100, True, 0, windows(16), 4096, 256, "mix", 60))
    out.append((1, 17, 7, 512, 4097, 2, 4096, True, 0, windows(17), 8192, 512, "mix", 61))
    out.append((0, 16, 7, 256, 9000, 1, 9000, False, 0, windows(16), 4096, 1024, "largest", 62))
    out.append((0, 17, 7, 512, 300, 1, 300, False, windows(17) - 1, 1, 4096, 256, "mix", 63))       # the top window alone
    return out


class GroupScatter:
    def __init__(self, dg, fb, G, nch, chunk_len, merged, w0, gridw):
        self.dg, self.fb, self.G, self.nch, self.chunk_len, self.merged, self.w0, self.gridw = dg, fb, G, nch, chunk_len, merged, w0, gridw
        self.n, self.W, self.c = dg.n, dg.W, dg.c
        assert ((1 << (dg.c - 1)) >> fb) == G and chunk_len * nch >= dg.n
        hist = dg.hist(nch, chunk_len, fb)                     # [W][nch][G]
        self.cnt = excl(hist, axis=1)
        self.gsize = hist.sum(axis=1)                          # [W][G]
        self.mshift = 0
        while (1 << self.mshift) < self.n:
            self.mshift += 1
        if merged:
            assert (self.W << self.mshift) <= (1 << 24)
            self.woff = excl(self.gsize, axis=0)
            self.gsize_m = self.gsize.sum(axis=0)
            self.gstart = excl(self.gsize_m)                   # [G]
        else:
            self.woff = None
            self.gstart = excl(self.gsize, axis=1)             # [W][G]

    def expected(self, w):
        """entries and groups of window w"""
        val, bk, sel = self.dg.entries(w)
        tag = (w << self.mshift) if self.merged else 0
        return ent(self.fb, sel | tag, bk & ((1 << self.fb) - 1), self.dg.neg[w][sel]), bk >> self.fb

    def model(self):
        t = np.full(self.W * self.n, ent_fill(self.fb), dtype=ent_dtype(self.fb))
        ws = range(self.w0, self.w0 + self.gridw)
        if self.merged:
            e = [self.expected(w) for w in ws]
            vals, grp = np.concatenate([x[0] for x in e]), np.concatenate([x[1] for x in e])
            t[:len(vals)] = vals[np.argsort(grp, kind="stable")]
        else:
            for w in ws:
                vals, grp = self.expected(w)
                t[w * self.n:w * self.n + len(vals)] = vals[np.argsort(grp, kind="stable")]
        return {"tmp": OBuf(len(t), dtype=ent_dtype(self.fb), init=t, fill=ent_fill(self.fb))}

    def check(self, out, what="k_group_scatter_big"):
        check_guards(out, what)
        tmp, fill = out["tmp"].own, ent_fill(self.fb)
        ws = range(self.w0, self.w0 + self.gridw)
        if self.merged:
            # one run per (group, window): the window's entries of a group start woff[w][g] into the group's run
            e = [self.expected(w) for w in ws]
            vals = np.concatenate([x[0] for x in e])
            lab = np.concatenate([x[1] * self.W + w for x, w in zip(e, ws)])
            starts = (self.gstart[:, None] + self.woff.T).reshape(-1)          # [G][W]
            check_runs(tmp, starts, self.gsize.T.reshape(-1), vals, lab, fill, f"{what}: merged")
            return
        rows = tmp.reshape(self.W, self.n)
        for w in range(self.W):
            if w in ws:
                vals, grp = self.expected(w)
                check_runs(rows[w], self.gstart[w], self.gsize[w], vals, grp, fill, f"{what}: window {w}")
            else:
                assert (rows[w] == fill).all(), f"{what}: window {w} is outside the grid and was written"


# ---- the fine pass ------------------------------------------------------------------------------------------------------------------------
class FineCase:
    """synthetic first-pass entries: group sizes chosen around the segment length, groups placed between runs of empty groups, the entries of
    a group in one bucket, in two, or spread out"""

    def __init__(self, name, fb, G, layout, maxseg_extra, seed):
        # layout: per window a list of (group, size, spread) with spread 1 (one bucket), 2 (two buckets) or 0 (all FINE buckets at random)
        rng = np.random.RandomState(seed)
        self.name, self.fb, self.G, self.Wg = name, fb, G, len(layout)
        self.FINE, self.SEGN = 1 << fb, seg_len(fb)
        self.B = G * self.FINE
        gs = np.zeros((self.Wg, G), dtype=np.int64)
        for w, row in enumerate(layout):
            for g, size, _ in row:
                gs[w, g] = size
        self.gsize = gs
        self.gstart = excl(gs, axis=1)
        self.n = int(gs.sum(axis=1).max()) + 37               # row length of tmp and sorted: the longest window and some slack
        nseg = (gs + self.SEGN - 1) // self.SEGN
        self.segbase = np.zeros((self.Wg, G + 1), dtype=np.int64)
        self.segbase[:, :G] = excl(nseg, axis=1)
        self.multi = (gs > self.SEGN).any(axis=1)
        self.nseg = nseg.sum(axis=1)
        self.segbase[:, G] = self.nseg | np.where(self.multi, MULTI_SEG, 0)
        self.maxseg = int(self.nseg.max()) + maxseg_extra
        self.tmp = np.full((self.Wg, self.n), ent_fill(fb), dtype=ent_dtype(fb))
        self.fine = np.full((self.Wg, self.n), -1, dtype=np.int64)
        for w, row in enumerate(layout):
            total = int(gs[w].sum())
            idx = ((rng.permutation(total).astype(np.int64) * 2654435761 + 12345) % (1 << 24)).astype(np.uint64)     # distinct 24-bit indexes (odd multiplier)
            sign = rng.randint(0, 2, total)
            fine = np.empty(total, dtype=np.int64)
            for g, size, spread in row:
                lo = int(self.gstart[w, g])
                if spread == 0:
                    fine[lo:lo + size] = rng.randint(0, self.FINE, size)
                elif spread == 1:
                    fine[lo:lo + size] = self.FINE - 1
                else:
                    fine[lo:lo + size] = np.where(rng.randint(0, 2, size), 0, self.FINE // 2 + 1)
            self.tmp[w, :total] = ent(fb, idx, fine, sign)
            self.fine[w, :total] = fine
        # reference: bucket sizes, bucket starts, per-segment counts
        self.bsize = np.zeros((self.Wg, self.B), dtype=np.int64)
        self.segcnt = np.zeros((self.Wg, self.maxseg, self.FINE), dtype=np.int64)
        self.seg_group = np.full((self.Wg, self.maxseg), -1, dtype=np.int64)
        for w in range(self.Wg):
            for g in np.nonzero(gs[w])[0]:
                lo, sz = int(self.gstart[w, g]), int(gs[w, g])
                self.bsize[w, g * self.FINE:(g + 1) * self.FINE] = np.bincount(self.fine[w, lo:lo + sz], minlength=self.FINE)
                for k in range(int(nseg[w, g])):
                    s = int(self.segbase[w, g]) + k
                    self.seg_group[w, s] = g
                    a, b = lo + k * self.SEGN, min(lo + (k + 1) * self.SEGN, lo + sz)
                    self.segcnt[w, s] = np.bincount(self.fine[w, a:b], minlength=self.FINE)
        self.bstart = excl(self.bsize, axis=1)
        self.big = gs > self.SEGN                              # groups of several segments: counted by k_fine_local, placed by k_fine_scatter

    def bucket_entries(self, w, groups):
        """(value without the fine field, bucket) of the entries of window w that lie in the given groups"""
        vals, lab = [], []
        for g in groups:
            lo, sz = int(self.gstart[w, g]), int(self.gsize[w, g])
            vals.append(ent_out(self.fb, self.tmp[w, lo:lo + sz]))
            lab.append(g * self.FINE + self.fine[w, lo:lo + sz])
        if not vals:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
        return np.concatenate(vals), np.concatenate(lab)

    def segoff_ref(self, reverse=False):
        """a valid segoff: the segments of a group take their places inside each bucket in ascending (or descending) segment order"""
        so = np.zeros_like(self.segcnt)
        for w in range(self.Wg):
            for g in np.nonzero(self.big[w])[0]:
                ss = [s for s in range(self.maxseg) if self.seg_group[w, s] == g]
                run = np.zeros(self.FINE, dtype=np.int64)
                for s in (ss[::-1] if reverse else ss):
                    so[w, s] = run
                    run = run + self.segcnt[w, s]
        return so

    def local_buffers(self):
        W, F = self.Wg, self.FINE
        return {"bsize": OBuf(W * self.B, init=np.zeros(W * self.B)), "segcnt": OBuf(W * self.maxseg * F), "segoff": OBuf(W * self.maxseg * F),
                "sorted": OBuf(W * self.n)}

    def _sorted_rows(self, rows, big):
        for w in range(self.Wg):
            groups = [g for g in np.nonzero(self.gsize[w])[0] if bool(self.big[w, g]) == big]
            vals, lab = self.bucket_entries(w, groups)
            o = np.argsort(lab, kind="stable")
            sizes = np.bincount(lab, minlength=self.B)
            pos = np.repeat(self.bstart[w], sizes) + np.arange(len(vals)) - np.repeat(excl(sizes), sizes)
            rows[w, pos] = vals[o]

    def model_local(self):
        o = self.local_buffers()
        o["bsize"].own[:] = self.bsize.reshape(-1)
        sc, so = o["segcnt"].own.reshape(self.Wg, self.maxseg, self.FINE), o["segoff"].own.reshape(self.Wg, self.maxseg, self.FINE)
        ref = self.segoff_ref()
        for w in range(self.Wg):
            for s in range(self.maxseg):
                g = self.seg_group[w, s]
                if g >= 0 and self.big[w, g]:
                    sc[w, s], so[w, s] = self.segcnt[w, s], ref[w, s]
        self._sorted_rows(o["sorted"].own.reshape(self.Wg, self.n), False)
        return o

    def check_local(self, out, gridy=None, what="k_fine_local"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        W, F = self.Wg, self.FINE
        same(out["bsize"].own, self.bsize, f"{what}: bsize")
        sc, so = out["segcnt"].own.reshape(W, self.maxseg, F), out["segoff"].own.reshape(W, self.maxseg, F)
        rows = out["sorted"].own.reshape(W, self.n)
        for w in range(W):
            for s in range(self.maxseg):
                g = self.seg_group[w, s]
                if g < 0 or not self.big[w, g]:
                    assert (sc[w, s] == FILL).all() and (so[w, s] == FILL).all(), f"{what}: window {w} segment {s} is none of a larger group and was written"
                else:
                    same(sc[w, s], self.segcnt[w, s], f"{what}: segcnt of window {w} segment {s}")
            for g in np.nonzero(self.big[w])[0]:
                # per bucket, the segments' intervals [segoff, segoff + segcnt) tile [0, bsize) without overlap
                ss = [s for s in range(self.maxseg) if self.seg_group[w, s] == g]
                for f in range(F):
                    iv = sorted((int(so[w, s, f]), int(self.segcnt[w, s, f])) for s in ss if self.segcnt[w, s, f])
                    at = 0
                    for a, ln in iv:
                        assert a == at, f"{what}: window {w} group {g} bucket {f}: a segment's place starts at {a}, expected {at} (overlap or gap)"
                        at += ln
                    assert at == self.bsize[w, g * F + f]
            small = [g for g in np.nonzero(self.gsize[w])[0] if not self.big[w, g]]
            vals, lab = self.bucket_entries(w, small)
            sizes = np.bincount(lab, minlength=self.B) if len(lab) else np.zeros(self.B, dtype=np.int64)
            check_runs(rows[w], self.bstart[w], sizes, vals, lab, FILL, f"{what}: sorted, window {w}")

    def scatter_buffers(self):
        return {"sorted": OBuf(self.Wg * self.n)}

    def model_scatter(self):
        o = self.scatter_buffers()
        self._sorted_rows(o["sorted"].own.reshape(self.Wg, self.n), True)
        return o

    def check_scatter(self, out, what="k_fine_scatter"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        rows = out["sorted"].own.reshape(self.Wg, self.n)
        for w in range(self.Wg):
            vals, lab = self.bucket_entries(w, list(np.nonzero(self.big[w])[0]))
            sizes = np.bincount(lab, minlength=self.B) if len(lab) else np.zeros(self.B, dtype=np.int64)
            check_runs(rows[w], self.bstart[w], sizes, vals, lab, FILL, f"{what}: window {w}")


def fine_cases():
    out = []
    for fb, G in ((7, 32), (9, 16)):
        S = seg_len(fb)
        # window 0: runs of empty groups before, between and after; window 1: nothing above S (no MULTI_SEG); window 2 (the one the extra
        # columns of k_fine_scatter walk): mostly groups of several segments
        lay = [[(3, 0, 0), (4, 1, 1), (5, S - 1, 0), (9, S, 2), (10, S + 1, 1), (G - 3, 2 * S, 0)],
               [(0, S, 1), (7, 5, 0), (G - 1, S - 1, 2)],
               [(1, 2 * S + 1, 2), (2, 3 * S + 7, 0), (8, S, 0), (G - 2, S + 1, 2), (G - 1, 3, 1)]]
        out.append(FineCase(f"FB{fb}", fb, G, lay, 5, 70 + fb))
    out.append(FineCase("FB7 all empty", 7, 16, [[], []], 2, 80))
    out.append(FineCase("FB7 G1024", 7, 1024, [[(0, SEG + 1, 0), (511, 1, 0), (512, 1, 0), (1023, SEG + 1, 1)]], 1, 81))
    return out


# ---- task tables --------------------------------------------------------------------------------------------------------------------------
def len_key(v):
    return np.minimum(v, 255)


class TaskCase:
    """bucket sizes of Wg rows of B buckets, a task length with its hot shift, and the tables the task kernels derive from them"""

    def __init__(self, name, Wg, B, T, shift, top, sizes, hot_cap=8):
        self.name, self.Wg, self.B, self.T, self.shift, self.hot_cap = name, Wg, B, T, shift, hot_cap
        self.top_w = Wg - 1 if top else -1
        self.T0, self.T_top = T | (shift << 30), (2 * T) | (shift << 30)
        v = np.asarray(sizes, dtype=np.int64).reshape(Wg, B)
        self.bsize = v
        t = np.full((Wg, 1), T, dtype=np.int64)
        if top:
            t[Wg - 1] = 2 * T
        self.t = t
        self.hot = v > GATHER_SUM_MAX * t
        self.Tb = np.where(self.hot, t >> shift, t) + 0 * v
        self.ntask = np.where(v > 0, (v + self.Tb - 1) // self.Tb, 0)
        self.rem = np.where(v > 0, v - (self.ntask - 1) * self.Tb, 0)
        self.bstart = excl(v, axis=1)
        self.rel = excl(self.ntask, axis=1)
        self.row_total = self.ntask.sum(axis=1)
        self.base = np.concatenate([excl(self.row_total), [int(self.row_total.sum())]])
        self.ntasks = int(self.row_total.sum())
        self.maxv = np.array([int(v.max()), int(self.hot.sum()), int(self.ntask.max())], dtype=np.int64)
        gh = np.zeros(LEN_BINS, dtype=np.int64)
        nz = v > 0
        np.add.at(gh, len_key(self.rem[nz]), 1)
        np.add.at(gh, len_key(self.Tb[nz]), self.ntask[nz] - 1)
        self.ghist = gh
        self.cursor = (gh[::-1].cumsum() - gh[::-1])[::-1].copy()              # start of a key's bin: the tasks with a larger key
        self.hot_set = set(int(x) for x in np.nonzero(self.hot.reshape(-1))[0])
        self.nsplit = B // 4096 if B >= 8192 else 0
        assert self.ntasks < (1 << 22), "a case this large does not belong in the suite"

    # -- bucket tables (k_bucket_rows, or k_bucket_part + k_bucket_fill)
    def table_buffers(self):
        n = self.Wg * self.B
        return {"bstart": OBuf(n), "ntask": OBuf(n), "rel": OBuf(n), "row_total": OBuf(self.Wg), "maxv": OBuf(3, init=np.zeros(3)),
                "ghist": OBuf(LEN_BINS, init=np.zeros(LEN_BINS)), "hot_list": OBuf(self.hot_cap), "part": OBuf(max(self.Wg * self.nsplit * 2, 1))}

    def model_tables(self):
        o = self.table_buffers()
        for k in ("bstart", "ntask", "rel", "row_total", "maxv", "ghist"):
            o[k].own[:] = getattr(self, k).reshape(-1)
        hs = sorted(self.hot_set)[:self.hot_cap]
        o["hot_list"].own[:len(hs)] = hs
        return o

    def check_tables(self, out, what="bucket tables"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        for k in ("bstart", "ntask", "rel", "row_total", "maxv", "ghist"):
            same(out[k].own, getattr(self, k), f"{what}: {k}")
        listed = min(len(self.hot_set), self.hot_cap)
        hl = [int(x) for x in out["hot_list"].own[:listed]]
        assert len(set(hl)) == listed and set(hl) <= self.hot_set, f"{what}: hot_list {hl} is not {listed} distinct members of the hot set"
        assert (out["hot_list"].own[listed:] == FILL).all(), f"{what}: hot_list written behind the {listed} listed buckets"

    # -- k_task_bases
    def bases_buffers(self):
        return {"base": OBuf(self.Wg + 1), "info": OBuf(2), "cursor": OBuf(LEN_BINS), "host_info": OBuf(4)}

    def model_bases(self):
        o = self.bases_buffers()
        o["base"].own[:] = self.base
        o["info"].own[:] = [self.ntasks, self.maxv[0]]
        o["cursor"].own[:] = self.cursor
        o["host_info"].own[:] = [self.ntasks, self.maxv[0], self.maxv[1], self.maxv[2]]
        return o

    def check_bases(self, out, what="k_task_bases"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        same(out["base"].own, self.base, f"{what}: base")
        same(out["info"].own, [self.ntasks, self.maxv[0]], f"{what}: info")
        same(out["host_info"].own, [self.ntasks, self.maxv[0], self.maxv[1], self.maxv[2]], f"{what}: the four host words")
        same(out["cursor"].own, self.cursor, f"{what}: descending-key cursors")

    # -- k_len_scatter
    SLACK = 100

    def scatter_buffers(self):
        return {"cursor": OBuf(LEN_BINS, init=self.cursor), "task_bkt": OBuf(self.ntasks + self.SLACK), "task_id": OBuf(self.ntasks + self.SLACK)}

    def model_scatter(self):
        o = self.scatter_buffers()
        flat_nt = self.ntask.reshape(-1)
        bkt = np.repeat(np.arange(self.Wg * self.B), flat_nt)
        seg = np.arange(self.ntasks) - np.repeat(excl(flat_nt), flat_nt)
        ln = np.where(seg < np.repeat(flat_nt, flat_nt) - 1, np.repeat(self.Tb.reshape(-1), flat_nt), np.repeat(self.rem.reshape(-1), flat_nt))
        order = np.argsort(-len_key(ln), kind="stable")
        o["task_bkt"].own[:self.ntasks] = bkt[order]
        o["task_id"].own[:self.ntasks] = np.arange(self.ntasks)[order]          # base[w] + rel[bucket] + seg = the task's number in bucket order
        o["cursor"].own[:] = self.cursor + self.ghist
        return o

    def check_scatter(self, out, what="k_len_scatter"):
        what = f"{what} {self.name}"
        check_guards(out, what)
        nt = self.ntasks
        bkt, tid = out["task_bkt"].own, out["task_id"].own
        assert (bkt[nt:] == FILL).all() and (tid[nt:] == FILL).all(), f"{what}: written behind the {nt} tasks"
        bkt, tid = bkt[:nt].astype(np.int64), tid[:nt].astype(np.int64)
        assert (bkt < self.Wg * self.B).all(), f"{what}: a bucket number outside the rows"
        assert np.array_equal(np.sort(tid), np.arange(nt)), f"{what}: task_id is not a permutation of 0 .. {nt - 1}"
        first = self.base[bkt // self.B] + self.rel.reshape(-1)[bkt]
        seg = tid - first
        cnt = self.ntask.reshape(-1)[bkt]
        assert ((seg >= 0) & (seg < cnt)).all(), f"{what}: a task id outside its bucket's range"
        ln = np.where(seg < cnt - 1, self.Tb.reshape(-1)[bkt], self.rem.reshape(-1)[bkt])
        key = len_key(ln)
        assert (key[1:] <= key[:-1]).all(), f"{what}: the keys of the task lengths are not in descending order (first rise at {int(np.nonzero(key[1:] > key[:-1])[0][0]) + 1 if nt > 1 and (key[1:] > key[:-1]).any() else -1})"
        same(out["cursor"].own, self.cursor + self.ghist, f"{what}: cursors after the scatter")

    # -- locate_task
    def locate_expected(self):
        flat_nt = self.ntask.reshape(-1)
        bkt = np.repeat(np.arange(self.Wg * self.B), flat_nt)
        seg = np.arange(self.ntasks) - np.repeat(excl(flat_nt), flat_nt)
        return np.stack([bkt // self.B, bkt % self.B, seg], axis=1)


def _task_sizes(T):
    return [0, 1, T - 1, T, T + 1, 32 * T, 32 * T + 1, 17 * T + 1]


def task_cases():
    out = []
    rng = np.random.RandomState(3)
    for T in (32, 48, 2048):
        for shift in (0, 1, 2):
            for top in (False, True):
                if T == 2048 and (shift, top) not in ((2, True), (0, False)):
                    continue
                # row 0: the edge sizes between empty buckets; row 1 (the top window if there is one): the edge sizes of ITS length 2T
                B = 256
                r0 = np.zeros(B, dtype=np.int64)
                r0[[3, 4, 5, 100, 101, 200, 201, 255]] = _task_sizes(T)
                r1 = np.zeros(B, dtype=np.int64)
                r1[[0, 1, 2, 3, 4, 5, 6, 7]] = _task_sizes(2 * T if top else T)
                r1[8:40] = rng.randint(0, 3 * T, 32)
                out.append(TaskCase(f"T{T} shift{shift} top{int(top)} B256", 2, B, T, shift, top, [r0, r1]))
    # one workgroup's 1024 buckets with more than 64 of them above BIG full tasks (the BIG_CAP fallback), beside plain ones
    r = rng.randint(0, 40, 1024)
    r[rng.permutation(1024)[:70]] = 17 * 32 + 1
    out.append(TaskCase("BIG_CAP overflow B1024", 1, 1024, 32, 2, False, [r]))
    r = rng.randint(0, 40, 1024)
    r[[5, 600, 1023]] = [17 * 32 + 1, 20 * 32, 32 * 32]
    out.append(TaskCase("BIG B1024", 1, 1024, 32, 2, False, [r]))
    # hot count above the cap of 8
    r = rng.randint(0, 64, (3, 16))
    r[0, :6] = 32 * 32 + 1
    r[2, 10:16] = 64 * 32 + 5
    out.append(TaskCase("hot above cap B16", 3, 16, 32, 2, True, r))
    # scalar rows (per & 3 != 0) and short rows
    out.append(TaskCase("B2", 3, 2, 32, 2, True, [[0, 5], [1025, 31], [0, 0]]))
    out.append(TaskCase("B16", 2, 16, 48, 1, False, rng.randint(0, 100, (2, 16))))
    out.append(TaskCase("B1100", 2, 1100, 32, 2, True, rng.randint(0, 70, (2, 1100))))
    # vector rows
    r = rng.randint(0, 70, (2, 1024))
    r[1, 1000:] = 0
    out.append(TaskCase("B1024", 2, 1024, 32, 2, True, r))
    r = rng.randint(0, 50, (2, 4096))
    r[0, 77] = 32 * 32 + 1
    out.append(TaskCase("B4096", 2, 4096, 32, 0, False, r))
    # rows in parts
    for B, Wg in ((8192, 3), (32768, 2), (65536, 1), (1 << 19, 1)):
        r = rng.randint(0, 4, (Wg, B)) * rng.randint(0, 2, (Wg, B))
        r[0, [1, 4095, 4096, B - 1]] = [32 * 32 + 1, 17 * 32 + 1, 33, 32 * 32]
        if Wg > 1:
            r[Wg - 1, B // 2] = 64 * 32 + 1
        out.append(TaskCase(f"B{B} parts", Wg, B, 32, 2, Wg > 1, r))
    # all-empty rows: in front, between and behind
    r = np.zeros((4, 256), dtype=np.int64)
    r[1, 17] = 100
    r[1, 255] = 3
    out.append(TaskCase("empty rows B256", 4, 256, 32, 2, True, r))
    out.append(TaskCase("all empty B1024", 2, 1024, 32, 2, False, np.zeros((2, 1024))))
    out.append(TaskCase("all empty B8192", 1, 8192, 32, 2, False, np.zeros((1, 8192))))
    return out


# ---- the further rounds' bookkeeping (msm_level_kernels.h) ----------------------------------------------------------------------------------
def level_count_cases():
    """(total, T, initial maxv, seed)"""
    return [(1, 32, 0, 1), (1023, 7, 0, 2), (1024, 32, 0, 3), (1025, 1, 5, 4), (3 * 1024 + 5, 2048, 1 << 30, 5)]


def level_scan_cases():
    """(W, B, threads): the scalar path (a lane's run is no multiple of four) and the vector path of scan_row"""
    return [(3, 2, 1024), (2, 16, 1024), (3, 256, 1024), (2, 1100, 1024), (2, 1024, 1024), (3, 4096, 1024), (2, 8192, 1024), (1, 1 << 16, 1024), (2, 4096, 256)]
