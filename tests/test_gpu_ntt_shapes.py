"""Every compiled NTT tile kernel of both shells (k_ntt_tile, k_ntt_tile_batch) on the device, at the smallest plan that runs it: the rows
of tests/ntt_shape_cases.py.  What the host emulation (tests/test_host_ntt.py, the same rows) cannot see shows only here: a missing barrier,
a wave-private pass that is not private on real waves, the dynamic-LDS attribute, a miscompiled instantiation, the batched shell's strides.

The plan knobs are read once per process, so each knob environment runs in a fresh child process; the one-step kernels need no knob and run
here.  Per row: kg_ntt_plan reports the tabled plan (a knob that fell back to the automatic shape fails, before any transform); the single
call, all four variants, against the oracle's Fft<Fr> (fft.rs:92-127); the batched call with gaps of three elements (gaps untouched) and
dense, against the oracle up to 2^18 and against the single call on a copy of the same data above; the extreme inputs (every element p - 1,
alternating p - 1 / 0, a lone p - 1), single and as one batch.  Every comparison is exact.

Wall time per case on an MI355X (one run; a child's time includes its interpreter start, imports and twiddle tables):
  tile11 (2^14, 2^16, 2^18) 3.9 s    tile10 (2^20, 2^21) 6.8 s    steps2_tile10 (2^22) 8.1 s    steps2 (2^22) 8.3 s
  steps3_tile11 (2^21) 5.1 s         steps3 (2^18) 3.2 s          one-step kernels, in process: 0.01-0.05 s each, 1.5 s to open the context
A 2^22 row itself takes 6.1 s, 4.3 s of them in the oracle's six transforms (the children print this per row); the 2^22 cases of
test_gpu_ntt_big.py::test_every_plan_knob_gives_the_same_transform, the same mechanism with five oracle transforms, took 5.7-5.9 s in the
same run, so nothing was cut from the rows from 2^20 up."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ntt_shape_cases as T

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ORACLE_S = [0.0]                          # seconds this process spent in the oracle's transforms (printed per row by the children)


def _oracle(fo, name, v):
    t0 = time.perf_counter()
    want = getattr(fo, name)(v, threads=8)
    ORACLE_S[0] += time.perf_counter() - t0
    return want


def _dev(arr):
    """a host array of uint64 words as an int64 tensor on the device"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    return t.contiguous().cpu().numpy().view(np.uint64)


def _single(ctx, x, k, inv, coset):
    """the single-transform entry on every transform of a copy of x (count, stride, 4)"""
    import torch
    ref = x.clone()
    torch.cuda.synchronize()
    for b in range(x.shape[0]):
        ctx.ntt(ref.data_ptr() + b * x.shape[1] * 32, k, inv, coset)
    ctx.sync()
    return ref


def _batched(ctx, x, k, inv, coset):
    import torch
    work = x.clone()
    torch.cuda.synchronize()
    ctx.ntt_batch(work.data_ptr(), k, x.shape[0], x.shape[1], inv, coset)
    ctx.sync()
    return work


def _strided(vs, stride):
    """(count, n, 4) host vectors -> a (count, stride, 4) device tensor, every gap word = SENTINEL"""
    buf = np.full((vs.shape[0], stride, 4), T.SENTINEL, dtype=np.uint64)
    buf[:, :vs.shape[1]] = vs
    return _dev(buf)


def check_batch(ctx, k, vs, want, names, stride, what):
    """the batched call over vs (count, n, 4) with the given stride: gaps untouched; want[name] is the (count, n, 4) host reference or
    None for the single call on a copy of the same data, compared on the device"""
    import torch
    n = 1 << k
    x = _strided(vs, stride)
    for name in names:
        inv, coset = T.VARIANTS[name]
        got = _batched(ctx, x, k, inv, coset)
        assert torch.equal(got[:, n:], x[:, n:]), (k, what, stride - n, name, "a gap was written")
        if want[name] is None:
            assert torch.equal(got, _single(ctx, x, k, inv, coset)), (k, what, stride - n, name, "batched differs from the single call")
        else:
            h = _host(got[:, :n])
            for b in range(len(vs)):
                assert (h[b] == want[name][b]).all(), (k, what, stride - n, name, b, "batched differs from the oracle")


def check_single(ctx, k, v, want, name, what):
    inv, coset = T.VARIANTS[name]
    d = ctx.upload(v)
    ctx.ntt(d.ptr, k, inv, coset)
    assert (d.numpy() == want).all(), (k, what, name, "single call differs from the oracle")


def check_extremes(ctx, O, k, names, only_first=False):
    """the extreme vectors in the given variants against the oracle, each through the single call and all as one batch (gaps of three)"""
    vs = T.extreme_vectors(O, k)
    if only_first:
        vs = vs[:1]
    fo = O.Fft(k)
    want = {name: np.stack([_oracle(fo, name, v) for v in vs]) for name in names}
    for name in names:
        for b, v in enumerate(vs):
            check_single(ctx, k, v, want[name][b], name, ("extreme", b))
    check_batch(ctx, k, vs, want, names, (1 << k) + 3, "extreme")


def check_row(ctx, O, k, count):
    """steps 2-4 of a row; step 1, the plan, is checked by child_main before the device is opened"""
    n = 1 << k
    names = list(T.VARIANTS)
    vs = np.stack([O.gen_scalars(0, T.seed_of(k) + b, 0, n) for b in range(count)])
    fo = O.Fft(k)
    with_oracle = k <= T.ORACLE_MAX_LOG
    want = {name: [_oracle(fo, name, vs[b]) for b in range(count if with_oracle else 1)] for name in names}
    for name in names:                                                                         # 2: single call against the oracle
        check_single(ctx, k, vs[0], want[name][0], name, "random")
    ref = want if with_oracle else dict.fromkeys(names)                                        # 3: batched, with gaps and dense
    check_batch(ctx, k, vs, ref, names, n + 3, "random")
    check_batch(ctx, k, vs, ref, ["dft", "coset_idft"], n, "random")
    if with_oracle:                                                                            # 4: extreme inputs, single and batched
        check_extremes(ctx, O, k, names)
    else:
        check_extremes(ctx, O, k, ["dft", "coset_idft"], only_first=True)


def child_main(index):
    """the rows of knob environment `index` (the environment is already this process's)"""
    import kogarashi_amd as K
    from oracle import oracle as O
    env = T.environments()[index]
    assert all(os.environ.get(key) == val for key, val in env.items()), env
    for _, k, plan, _ in T.rows_of(env):                   # 1: every row hits its kernels -- checked before the device is opened
        assert K.lib.ntt_plan(k) == plan, (k, "kg_ntt_plan reports", K.lib.ntt_plan(k), "the table expects", plan)
    ctx = K.Context(0)
    for _, k, _, count in T.rows_of(env):
        t0, o0 = time.perf_counter(), ORACLE_S[0]
        check_row(ctx, O, k, count)
        print(f"2^{k}: {time.perf_counter() - t0:.2f} s, {ORACLE_S[0] - o0:.2f} s of them in the oracle")
    ctx.close()
    print("ok")


_CHILD_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r]
import test_gpu_ntt_shapes
test_gpu_ntt_shapes.child_main(%d)
"""


@pytest.mark.parametrize("index", range(len(T.environments())), ids=[T.env_id(e) for e in T.environments()])
def test_knob_shapes(index):
    """one fresh child process per knob environment; no retry"""
    env = T.environments()[index]
    clean = {key: val for key, val in os.environ.items() if not key.startswith("KG_NTT_")}
    r = subprocess.run([sys.executable, "-c", _CHILD_SCRIPT % (os.path.dirname(TESTS), TESTS, index)], env=dict(clean, **env),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout, end="")
    assert r.returncode == 0 and "ok" in r.stdout.split(), (env, r.returncode, r.stderr[-2000:])


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("k", T.ONE_STEP)
def test_one_step_kernels_on_extreme_inputs(ctx, oracle, k):
    """2^1..2^11: the three extreme vectors, all four variants, single and as one batch of three, against the oracle"""
    from kogarashi_amd import lib as L
    assert L.ntt_plan(k) == [(k, k)]
    check_extremes(ctx, oracle, k, list(T.VARIANTS))
