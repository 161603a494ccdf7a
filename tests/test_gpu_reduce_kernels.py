"""The point-side kernels of the long MSM ON THE DEVICE, one at a time (tests/device/devprobe_reduce.h: the product's msm_bases.h,
msm_acc_kernels.h and msm_reduce_kernels.h, included unchanged): bases -> resident forms and window tables; sorted lists -> partial sums ->
(hot-bucket trees | a further partial-sum round) -> the dense bucket array -> halving levels -> the fused tail and its exported slot.

The rest of the suite reaches these kernels only through whole MSMs whose single affine sum is compared with the oracle: that sees neither a
write outside a kernel's owned range (the buffer descriptors clip nothing) nor the outputs the sum barely depends on, and small inputs never
produce an empty hot-sum share, a split above 16, the strided hot-sum loop, fused sets, a merged row or a run-time tail of two items.  Here every kernel reads points and
tables built by the reference of tests/reduce_cases.py (never the output of an earlier launch), every output point is compared exactly with
the expected multiple of the generator, and every output buffer has a guard region behind it that must come back untouched."""
import ctypes as C
import os
import shutil

import pytest

import primitive_cases as PC
import reduce_cases as RC
import sort_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devlib():
    """tests/device/libdevprobe.so, as tests/test_gpu_sort_kernels.py takes it: rebuilt when stale if hipcc is here, a FAILURE when there is neither"""
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


def run(dev, case):
    """one launch; a HIP error ends the session: nothing more is started on a device that may have faulted"""
    out = case.fresh()
    bufs, params = case.call_args(out)
    try:
        SC.call(dev, case.entry, bufs, params)
    except SC.DeviceError as e:
        pytest.exit(f"{case.name}: {e}: stopping, no further launches", returncode=3)
    case.check(out)


def cases(make):
    cs = make()
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


@cases(RC.prep_cases)
def test_prep_bases(devlib, case):
    """the resident words equal the packer's, word for word: both forms, three fields, n = 1, 255, 256, 257, with and without an identity
    array (flagged points carry arbitrary coordinates), coordinates 0, 1, p - 1 and the special points of acc_abi_cases"""
    run(devlib, case)


@cases(RC.table_cases)
def test_table_next(devlib, case):
    """next[i] = the packer applied to 2^c * prev[i] in canonical values (c = 1, 2, 13; n = 1, 63, 64, 65; both forms, three fields); a flagged
    identity goes through as zeros with the flag"""
    run(devlib, case)


@cases(RC.acc_cases)
def test_acc_tasks(devlib, case):
    """slot task_id[p] of set k holds the group sum of that task's entries of that set: ntasks = 1, 63, 64, 65, 130 (ragged last waves, per set
    when fused), a bucket cut into tasks with a remainder of one entry, a hot bucket cut at T >> 2, the top window at T_top; every base form;
    chains P, P and P, -P, P, the sign bit on the first and on the last entry, a flagged identity first, in the middle and last; nsets = 2, 3
    over one sort (entries below idx_off skipped, the identity where a task has none left, a partial buffer per set); the merged form over a
    table of windows x tab_n rows; two valid orders of the task list.  Slots behind ntasks stay untouched."""
    run(devlib, case)


@cases(RC.gather_cases)
def test_gather(devlib, case):
    """k_gather_buckets (cnt 0 / 1; B = 2, 64, 512): bucket (w, b) is its partial sum or the identity.  k_gather_halve (B = 2 TL, 4 TL; W = 2):
    array 0 of a window holds the pair sums of buckets 2i, 2i + 1 and array 1 the odd buckets, over nodes empty + empty, empty + P, P + empty,
    P + P, P + (-P) and ordinary.  k_gather_sum (cnt 0, 1, 2, 31, 32, 33, 100): a bucket's partial sums added up -- equal ones (the running
    sum doubles), alternating ones (identities on the way) -- and above 32 the first partial sum alone."""
    run(devlib, case)


@cases(RC.sum_tasks_cases)
def test_sum_tasks(devlib, case):
    """slot base[w] + rel[bucket] + seg of the new round holds the seg-th run of T2 previous partial sums of the bucket (buckets of T2 - 1, T2,
    T2 + 1, 2 T2, 2 T2 + 1, 3 T2, 1 and 0 of them; T2 = 2, 16); the launch covers the previous round's task count and its surplus threads
    write nothing"""
    run(devlib, case)


@cases(RC.halve_cases)
def test_halve(devlib, case):
    """(w, a, i) of the output = items 2i + (2i + 1) of array a, and the new array narr_in = the odd items of array 0: narr_in = 1, 2, 3,
    n_out = 1, 2, 64, TL, W = 3; all items equal, alternating P / -P, identities on one or both sides, pool points"""
    run(devlib, case)


@cases(RC.tail_cases)
def test_reduce_tail(devlib, case):
    """the exported slot of W * c points, c = narr + log2(len): arr a < narr = the sum of array a, arr narr - 1 + j = the sum of the items of
    array 0 whose index has bit j - 1 set.  k_reduce_tail<TL> at len = TL (narr 1, 2, 3), k_reduce_tail<0> at len = 2, 4, 8, TL / 4, TL / 2
    (64 threads, the stride of the longest short array), k_reduce_tail_coop at len = 2, 4, TL / 2, TL (narr 1, 3)"""
    run(devlib, case)


@cases(RC.hot_cases)
def test_hot(devlib, case):
    """k_hot_sum: scratch point i * split + y = the y-th share of hot bucket i, the identity for an empty share (cnt = 33 .. 49 in 16 shares,
    40 in 17, 300 in 100, 40 and 2 max + 1 in the largest split, and 16 NT + 16 in 16: the strided loop), nothing behind nhot * split.
    k_hot_fold, from a reference scratch: the bucket's first partial slot holds the total and every other word of part is as it was.  One
    and three hot buckets, in different windows and out of bucket order, between buckets that are not hot."""
    run(devlib, case)
