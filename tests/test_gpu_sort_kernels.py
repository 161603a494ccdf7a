"""The integer kernels of the long MSM's scalar side ON THE DEVICE, one at a time (tests/device/devprobe_sort.h: the product's msm_sort_kernels.h,
msm_task_kernels.h and msm_level_kernels.h, included unchanged): scalars -> biased words -> signed digits -> per-bucket lists -> the task table.

The rest of the suite reaches these kernels only through whole MSMs whose affine sum is compared with the oracle: that sees neither the outputs
the sum does not depend on (the order of the task list, the length histogram and cursors, the four words the host reads back, the hot list,
MULTI_SEG) nor a write outside the owned range, and its inputs do not put exactly SEGN or 32 T + 1 entries anywhere.  Here every kernel reads
tables built by the reference of tests/sort_cases.py (never the output of an earlier launch), every comparison is exact, and every output
buffer has a guard region behind it that must come back untouched."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import primitive_cases as PC
import sort_cases as SC
from sort_cases import OBuf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devlib():
    """tests/device/libdevprobe.so, as tests/test_gpu_primitives.py takes it: rebuilt when stale if hipcc is here, a FAILURE when there is neither"""
    from kogarashi_amd import build as kb, lib as KL
    KL.load()                                   # torch and the product library first: the process has one HIP runtime (lib.py load())
    if shutil.which("hipcc") is not None:
        kb.build_devprobe()
    elif not os.path.exists(kb.DEVPROBE_OUT):
        pytest.fail(f"{kb.DEVPROBE_OUT} is missing and there is no hipcc to build it (python -m kogarashi_amd.build --devprobe)")
    dev = C.CDLL(kb.DEVPROBE_OUT)
    missing = [e for e in PC.DEV_EXPORTS if not hasattr(dev, e)]
    assert not missing, missing
    return dev


def call(dev, name, bufs, params):
    """a HIP error ends the session: nothing more is started on a device that may have faulted"""
    try:
        SC.call(dev, name, bufs, params)
    except SC.DeviceError as e:
        pytest.exit(f"{e}: stopping, no further launches", returncode=3)


@functools.lru_cache(maxsize=None)
def digits(field, c, n, kind, seed):
    return SC.Digits(SC.scalar_set(field, c, n, seed, kind), c)


def abi_scalars(oracle, field, dg):
    """the chosen integers through the ORACLE's to_mont: the expected integer is the chosen one, no Montgomery constant here"""
    return SC.scalars_to_words(dg.ks, lambda a: oracle.f_to_mont(field, a))


def ids(cases):
    return ["-".join(str(v) for v in x) for x in cases]


# ---- prep ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.prep_cases(), ids=ids(SC.prep_cases()))
def test_prep_scalars(devlib, oracle, case):
    """kt plane j of scalar i = word j of k + H, for the edge scalars of both fields at every n around the 256-thread workgroup and beyond"""
    field, c, n, kind, seed = case
    dg = digits(field, c, n, kind, seed)
    out = {"kt": OBuf(8 * n)}
    call(devlib, "dp_sort_prep", [abi_scalars(oracle, field, dg), SC.bias_words(c), out["kt"], None], [field, n, 0])
    SC.check_prep(out, dg)


@pytest.mark.parametrize("case", SC.prep_count_cases(), ids=ids(SC.prep_count_cases()))
def test_prep_scalars_count(devlib, oracle, case):
    """the same kt, and cnt[w][chunk][group] = the histogram of (|d| - 1) >> FB over the chunk's scalars (zero digits skipped), for 4096 and
    1024 scalars per workgroup"""
    field, c, fb, n, chunk_len, nch, kind, seed = case
    dg = digits(field, c, n, kind, seed)
    G = (1 << (c - 1)) >> fb
    sc = abi_scalars(oracle, field, dg)
    for per_wg in (4096, 1024):
        out = {"kt": OBuf(8 * n), "cnt": OBuf(dg.W * nch * G, init=np.zeros(dg.W * nch * G))}
        call(devlib, "dp_sort_prep", [sc, SC.bias_words(c), out["kt"], out["cnt"]], [field, n, 1, c, dg.W, fb, G, nch, chunk_len, per_wg])
        SC.check_prep_count(out, dg, fb, nch, chunk_len, f"prep_count per_wg {per_wg}")


# ---- one-pass sort ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.onepass_cases(), ids=ids(SC.onepass_cases()))
def test_onepass_count_scan_scatter(devlib, case):
    """k_count = the per-(window, chunk, bucket) histogram; k_scan_chunks leaves the exclusive prefix over chunks and bsize; after k_scatter
    every bucket's slice of its window's row is the right multiset of (index | sign << 31) and the rest of the row is untouched.  Each kernel
    reads the reference's tables."""
    field, c, n, nch, kind, seed = case
    op = SC.OnePass(digits(field, c, n, kind, seed), nch)
    W, B = op.W, op.B
    p = [0, n, c, W, op.chunk_len, nch]
    kt = op.dg.kt
    out = {"cnt": OBuf(W * nch * B)}
    call(devlib, "dp_sort_onepass", [kt, out["cnt"], None, None, None], p)
    op.check_count(out)
    out = {"cnt": OBuf(W * nch * B, init=op.hist), "bsize": OBuf(W * B)}
    call(devlib, "dp_sort_onepass", [kt, out["cnt"], out["bsize"], None, None], [1] + p[1:])
    op.check_scan(out)
    out = {"sorted": OBuf(W * n)}
    call(devlib, "dp_sort_onepass", [kt, SC.u32(op.prefix), None, SC.u32(op.bstart), out["sorted"]], [2] + p[1:])
    op.check_scatter(out)


@pytest.mark.parametrize("offset,nbytes,words", [(0, 0, 64), (0, 16, 64), (16, 20, 64), (256, 4096, 2048), (1024, 5 * 1024 * 1024 + 64, 1400000)])
def test_zero_fill(devlib, offset, nbytes, words):
    """zero_fill clears the bytes it is given, rounded up to 16 (the last case is more than the 1024 workgroups cover in one step), nothing else"""
    out = {"buf": OBuf(words)}
    call(devlib, "dp_sort_zero_fill", [out["buf"]], [offset, nbytes])
    SC.check_guards(out, "zero_fill")
    lo, hi = offset // 4, (offset + (nbytes + 15) // 16 * 16) // 4
    a = out["buf"].own
    assert not a[lo:hi].any() and (a[:lo] == SC.FILL).all() and (a[hi:] == SC.FILL).all()


# ---- two-pass sort: tables ----------------------------------------------------------------------------------------------------------------
GSC = SC.group_scan_cases()


@pytest.mark.parametrize("i", range(len(GSC)), ids=[g.name for g in GSC])
def test_group_scan(devlib, i):
    """prefix over chunks in place (chunk counts that are no multiple of 8), gsize, gstart, segbase, the segment total with MULTI_SEG iff a
    group exceeds the segment length (groups of exactly seg and seg + 1 entries), the window's bsize and the zero words cleared, nothing else"""
    gc = GSC[i]
    out = gc.buffers()
    call(devlib, "dp_sort_group_scan", [out[k] for k in ("cnt", "gsize", "gstart", "segbase", "bsize", "zero")], [gc.W, gc.nch, gc.G, gc.B, gc.zwords, gc.seg, gc.nt])
    gc.check(out)


MGC = SC.merge_cases()


@pytest.mark.parametrize("i", range(len(MGC)), ids=[m.name for m in MGC])
def test_merge_groups(devlib, i):
    mc = MGC[i]
    out = mc.buffers()
    call(devlib, "dp_sort_merge_groups", [SC.u32(mc.gsize)] + [out[k] for k in ("woff", "gsize_m", "gstart_m", "segbase_m")], [mc.W, mc.G])
    mc.check(out)


# ---- two-pass sort: first pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.group_scatter_cases(), ids=ids(SC.group_scatter_cases()))
def test_group_scatter_big(devlib, case):
    """every group's run of tmp is the multiset of Ent<FB>(index | window tag, fine bits, sign) of the reference: all six (c, FB, G) shapes, all six
    (TILE, NT) kernels for both entry widths, a window group (w0 > 0, a grid narrower than W: the other windows' rows stay untouched), and the
    merged form (one run per group, the window above the index at mshift)"""
    field, c, fb, G, n, nch, chunk_len, merged, w0, gridw, tile, nt, kind, seed = case
    gs = SC.GroupScatter(digits(field, c, n, kind, seed), fb, G, nch, chunk_len, merged, w0, gridw)
    out = {"tmp": OBuf(gs.W * n, dtype=SC.ent_dtype(fb), fill=SC.ent_fill(fb))}
    call(devlib, "dp_sort_group_scatter_big", [gs.dg.kt, SC.u32(gs.cnt), SC.u32(gs.gstart), None, out["tmp"], SC.u32(gs.woff) if merged else None],
         [fb, tile, nt, gridw, nch, n, c, gs.W, chunk_len, G, gs.mshift, w0])
    gs.check(out)


# ---- two-pass sort: fine pass -------------------------------------------------------------------------------------------------------------
FC = SC.fine_cases()


@pytest.mark.parametrize("i", range(len(FC)), ids=[f.name for f in FC])
def test_fine_local(devlib, i):
    """groups of 0, 1, SEGN - 1 and SEGN entries are sorted by one workgroup (bsize exact, every bucket's slice the right multiset with the fine
    bits stripped); groups of SEGN + 1, 2 SEGN, 2 SEGN + 1 and 3 SEGN + 7 are counted per (segment, fine bucket) and their segments' places
    tile every bucket; workgroups past the last segment write nothing"""
    fc = FC[i]
    out = fc.local_buffers()
    call(devlib, "dp_sort_fine_local", [fc.tmp, SC.u32(fc.gstart), SC.u32(fc.gsize), SC.u32(fc.segbase)] + [out[k] for k in ("bsize", "segcnt", "segoff", "sorted")],
         [fc.fb, fc.Wg, fc.maxseg, fc.n, fc.G, fc.B, fc.maxseg])
    fc.check_local(out)


@pytest.mark.parametrize("i", range(len(FC)), ids=[f.name for f in FC])
def test_fine_scatter(devlib, i):
    """given the reference's bstart and segcnt and a valid segoff (the segments of a group in ascending, then in descending order), the lists of
    the larger groups are the right multisets; windows without MULTI_SEG and groups of one segment are left untouched.  With and without the
    extra columns of the last window, few and many rows of segment walkers."""
    fc = FC[i]
    # the tables hold garbage wherever k_fine_local would not have written them: only the segments of the larger groups are filled in
    own = (fc.seg_group >= 0) & np.take_along_axis(fc.big, np.maximum(fc.seg_group, 0), axis=1)
    own = np.repeat(own[:, :, None], fc.FINE, axis=2)
    segcnt = np.where(own, fc.segcnt, SC.FILL)
    for reverse, extra, rows in ((False, True, 2), (True, False, min(fc.maxseg, 64)), (False, False, 1)):
        segoff = np.where(own, fc.segoff_ref(reverse), SC.FILL)
        out = fc.scatter_buffers()
        gridx, extra_w = (fc.Wg + 3, fc.Wg - 1) if extra else (fc.Wg, -1)
        call(devlib, "dp_sort_fine_scatter", [fc.tmp, SC.u32(fc.gstart), SC.u32(fc.gsize), SC.u32(fc.segbase), SC.u32(fc.bstart), SC.u32(segcnt), SC.u32(segoff), out["sorted"]],
             [fc.fb, gridx, rows, fc.n, fc.G, fc.B, fc.maxseg, fc.Wg, extra_w])
        fc.check_scatter(out, f"k_fine_scatter (grid {gridx} x {rows})")


# ---- task tables --------------------------------------------------------------------------------------------------------------------------
TC = SC.task_cases()
TIDS = [t.name for t in TC]


@pytest.mark.parametrize("i", range(len(TC)), ids=TIDS)
def test_bucket_tables(devlib, i):
    """bstart, ntask, rel, row_total, the three maxima and the length histogram equal the reference; hot_list holds distinct members of the hot
    set up to a cap of 8, with the true count beyond it.  k_bucket_rows for B <= 4096 (scalar and vector rows), k_bucket_part + k_bucket_fill
    from B = 8192 up; buckets at T - 1, T, T + 1, 32 T, 32 T + 1 for hot shifts 0, 1, 2, with and without a top window of length 2 T."""
    tc = TC[i]
    out = tc.table_buffers()
    call(devlib, "dp_task_bucket_tables", [SC.u32(tc.bsize)] + [out[k] for k in ("bstart", "ntask", "rel", "row_total", "maxv", "ghist", "hot_list", "part")],
         [tc.Wg, tc.B, tc.T0, tc.T_top, tc.top_w, tc.hot_cap, tc.nsplit])
    tc.check_tables(out)


@pytest.mark.parametrize("i", range(len(TC)), ids=TIDS)
def test_task_bases(devlib, i):
    """base, info, the four words the host reads back and the descending-key cursors, from the reference's row totals, maxima and histogram"""
    tc = TC[i]
    out = tc.bases_buffers()
    call(devlib, "dp_task_bases", [SC.u32(tc.row_total), out["base"], SC.u32(tc.maxv), out["info"], SC.u32(tc.ghist), out["cursor"], out["host_info"]], [tc.Wg])
    tc.check_bases(out)


@pytest.mark.parametrize("i", range(len(TC)), ids=TIDS)
def test_len_scatter(devlib, i):
    """task_id[:ntasks] is a permutation, every id lies in its bucket's range, the keys of the task lengths never rise (a bucket's last task
    has the remainder length, the others T_b), nothing is written behind ntasks: plain buckets, buckets above BIG full tasks, and more than
    BIG_CAP of those in one workgroup"""
    tc = TC[i]
    out = tc.scatter_buffers()
    call(devlib, "dp_task_len_scatter", [SC.u32(tc.bsize), SC.u32(tc.ntask), SC.u32(tc.rel), SC.u32(tc.base), out["cursor"], out["task_bkt"], out["task_id"]],
         [tc.Wg, tc.B, tc.T0, tc.T_top, tc.top_w, tc.ntasks])
    tc.check_scatter(out)


@pytest.mark.parametrize("i", [i for i, t in enumerate(TC) if t.ntasks], ids=[t.name for t in TC if t.ntasks])
def test_locate_task(devlib, i):
    """task number -> (window, bucket, segment) over runs of empty buckets and empty windows: every task of the table"""
    tc = TC[i]
    out = {"loc": OBuf(3 * tc.ntasks)}
    call(devlib, "dp_level_ops", [SC.u32(tc.base), SC.u32(tc.rel), out["loc"], None], [3, tc.Wg, tc.B, tc.ntasks])
    SC.check_guards(out, "locate_task")
    SC.same(out["loc"].own, tc.locate_expected(), f"locate_task {tc.name}")


# ---- the further rounds' bookkeeping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,T,maxv0,seed", SC.level_count_cases())
def test_level_task_count(devlib, total, T, maxv0, seed):
    v = np.random.RandomState(seed).randint(0, 5 * T + 2, total).astype(np.int64)
    v[total // 2] = 0
    out = {"ntask": OBuf(total), "maxv": OBuf(1, init=[maxv0])}
    call(devlib, "dp_level_ops", [SC.u32(v), out["ntask"], out["maxv"], None], [0, total, T])
    SC.check_guards(out, "k_task_count")
    SC.same(out["ntask"].own, (v + T - 1) // T, "k_task_count: ntask")
    assert int(out["maxv"].own[0]) == max(maxv0, int(v.max()))


@pytest.mark.parametrize("W,B,nt", SC.level_scan_cases())
def test_level_scan_rows_and_row_bases(devlib, W, B, nt):
    v = np.random.RandomState(B + W).randint(0, 9, (W, B)).astype(np.int64)
    v[W - 1, B // 2:] = 0
    out = {"rel": OBuf(W * B), "row_total": OBuf(W)}
    call(devlib, "dp_level_ops", [SC.u32(v), out["rel"], out["row_total"], None], [1, W, B, nt])
    SC.check_guards(out, "k_scan_rows")
    SC.same(out["rel"].own, SC.excl(v, axis=1), "k_scan_rows: rel")
    SC.same(out["row_total"].own, v.sum(axis=1), "k_scan_rows: row_total")
    rt = v.sum(axis=1)
    for maxv in (None, np.array([77], dtype=np.uint32)):
        out = {"base": OBuf(W + 1), "info": OBuf(2)}
        call(devlib, "dp_level_ops", [SC.u32(rt), out["base"], maxv, out["info"]], [2, W])
        SC.check_guards(out, "k_row_bases")
        SC.same(out["base"].own, np.concatenate([SC.excl(rt), [rt.sum()]]), "k_row_bases: base")
        SC.same(out["info"].own, [rt.sum(), 0 if maxv is None else 77], "k_row_bases: info")
