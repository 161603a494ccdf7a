"""kg_ntt_bn254_fr_batch / kg_fr_divide_by_z_on_coset_batch on the device: many transforms of one size in one launch per plan step.
Every comparison is exact.  References: the oracle's Fft<Fr> (fft.rs:92-127) up to 2^16, the single-transform entry on a copy of the
same data (checked against the oracle by tests/test_gpu_parity.py, test_gpu_large.py and test_gpu_ntt_big.py) at every size, and Python
integers where the map is small enough to write out.  The sizes are the smallest that reach each code path: every one-step kernel
(2^1..2^11), the column / row tile shapes the automatic two-step plans use (2^12..2^21: six of the eleven column and five of the nine
two-step row shapes; no plan knob is set here, the shapes only a knob or a size from 2^22 up reaches are run by
tests/test_gpu_ntt_shapes.py), a three-step plan whose middle step runs in
place on two scratch slabs (2^22 x 2), a batch past the grid's y limit (65537 x 2^1) and one past a scratch group's edge (2049 x 2^12).
Large inputs are generated on the device and compared there; only what is compared with a host reference is read back."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x4B6F676172617368
SENTINEL = 0x0DEADBEEF0DEADBE            # every word of every gap element
VARIANTS = {"dft": (False, False), "idft": (True, False), "coset_dft": (False, True), "coset_idft": (True, True)}


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _fill(ctx, k, count, stride, seed):
    """a device tensor of count * stride elements (int64 words): transform b = gen_scalars(seed + b) -- the same data whatever the
    stride --, every gap word = SENTINEL"""
    import torch
    import kogarashi_amd as K
    n = 1 << k
    x = torch.full((count, stride, 4), SENTINEL, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for b in range(count):
        ctx.gen_scalars(K.KG_FR, seed + b, 0, n, x.data_ptr() + b * stride * 32)
    ctx.sync()
    return x


def _random(ctx, nelems, seed):
    """nelems elements of gen_scalars(seed) on the device, as (nelems, 4) int64 words"""
    import torch
    import kogarashi_amd as K
    x = torch.empty((nelems, 4), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.gen_scalars(K.KG_FR, seed, 0, nelems, x.data_ptr())
    ctx.sync()
    return x


def _single(ctx, x, k, inv, coset):
    """the single-transform entry on every transform of a copy of x"""
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


def _host(t):
    return t.contiguous().cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _oracle_rows(k, seed, name):
    """the oracle's transform of gen_scalars(seed) -- computed once per (size, data, variant) and shared by the strides"""
    from oracle import oracle as O
    want = getattr(O.Fft(k), name)(O.gen_scalars(0, seed, 0, 1 << k), threads=8)
    want.setflags(write=False)
    return want


def _check(ctx, k, count, stride, names, oracle_too):
    import torch
    n = 1 << k
    seed = SEED + 7000 + 16 * k
    x = _fill(ctx, k, count, stride, seed)
    for name in names:
        inv, coset = VARIANTS[name]
        got = _batched(ctx, x, k, inv, coset)
        assert torch.equal(got[:, n:], x[:, n:]), (k, stride, name, "a gap was written")
        assert torch.equal(got, _single(ctx, x, k, inv, coset)), (k, stride, name, "differs from the single call")
        if oracle_too:
            h = _host(got[:, :n])
            for b in range(count):
                assert (h[b] == _oracle_rows(k, seed + b, name)).all(), (k, stride, name, b, "differs from the oracle")


@pytest.mark.parametrize("k", range(1, 12))
def test_single_step_shapes(ctx, k):
    """2^1..2^11: every one-step instantiation, all four variants, three transforms with their own data, gaps of five elements"""
    _check(ctx, k, 3, (1 << k) + 5, list(VARIANTS), True)


@pytest.mark.parametrize("k", range(12, 22))
def test_two_step_shapes(ctx, k):
    """2^12..2^21 walk every column and row tile shape of the automatic plans -- (6,4), (7,3), (8,2), (9,1), (10,1), (11,1) --; dense
    (stride = n) and with gaps of three elements, so that step A reads and step C writes with a stride other than the scratch's"""
    from kogarashi_amd import lib as L
    plan = L.ntt_plan(k)
    assert len(plan) == 2 and all((m, t - m) in ((6, 4), (7, 3), (8, 2), (9, 1), (10, 1), (11, 1)) for m, t in plan), plan
    for stride in ((1 << k), (1 << k) + 3):
        if k <= 16:
            _check(ctx, k, 2, stride, list(VARIANTS), True)
        else:
            _check(ctx, k, 2, stride, ["dft", "coset_idft"], False)


def test_three_step_plan_inside_one_launch(ctx):
    """2^22 x 2: per_launch is 2, so both transforms share every launch and step B runs in place on two scratch slabs"""
    from kogarashi_amd import lib as L
    assert len(L.ntt_plan(22)) == 3 and L.ntt_batch_plan(22, 2) == (1, 2)
    _check(ctx, 22, 2, 1 << 22, ["dft", "coset_idft"], False)


def test_more_transforms_than_a_grid_carries(ctx, pyoracle):
    """65535 + 2 transforms of two elements (two launch groups): (a, b) -> (a + b, a - b) mod r in Python integers; the data stay in
    Montgomery form because the map is linear"""
    import torch
    from kogarashi_amd import lib as L
    count, stride = 65535 + 2, 3
    assert L.ntt_batch_plan(1, count) == (2, 65535)
    x = _random(ctx, count * stride, SEED + 7100).view(count, stride, 4)
    x[:, 2:] = SENTINEL                                            # every third element is a gap
    torch.cuda.synchronize()
    got, src = _host(_batched(ctx, x, 1, False, False)), _host(x)
    assert (got[:, 2] == src[:, 2]).all(), "a gap was written"
    r = pyoracle.R_MOD

    def ints(a):                                                    # (count, 4) little-endian limbs -> Python integers
        raw = np.ascontiguousarray(a).tobytes()
        return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(a))]
    a, b, s, d = ints(src[:, 0]), ints(src[:, 1]), ints(got[:, 0]), ints(got[:, 1])
    bad = [i for i in range(count) if s[i] != (a[i] + b[i]) % r or d[i] != (a[i] - b[i]) % r]
    assert not bad, (len(bad), bad[:8])


def test_group_edge_with_scratch(ctx):
    """2049 transforms of 2^12 elements: per_launch is 2048, the last transform is a launch group of its own on the same scratch;
    transforms 0, 2047 and 2048 against the single call"""
    import torch
    from kogarashi_amd import lib as L
    k, count = 12, 2049
    n = 1 << k
    assert L.ntt_batch_plan(k, count) == (2, 2048)
    x = _random(ctx, count * n, SEED + 7200).view(count, n, 4)
    picks = [0, 2047, 2048]
    for name in ("coset_dft", "coset_idft"):
        inv, coset = VARIANTS[name]
        ref = x[picks].clone()
        work = x.clone()
        torch.cuda.synchronize()
        for i in range(len(picks)):
            ctx.ntt(ref.data_ptr() + i * n * 32, k, inv, coset)
        ctx.ntt_batch(work.data_ptr(), k, count, n, inv, coset)
        ctx.sync()
        assert torch.equal(work[picks], ref), name
        del work


def test_stream_order(ctx):
    """the input is produced by kg_field_vec_op on the same context immediately before the batch, with no synchronisation between"""
    import torch
    import kogarashi_amd as K
    k, count = 10, 64
    n = 1 << k
    a, b = _random(ctx, count * n, SEED + 7300), _random(ctx, count * n, SEED + 7301)
    got, ref = torch.zeros_like(a), torch.zeros_like(a)
    torch.cuda.synchronize()
    ctx.field_vec_op(K.KG_FR, "mul", a.data_ptr(), b.data_ptr(), got.data_ptr(), count * n)
    ctx.ntt_batch(got.data_ptr(), k, count, n, False, True)
    ctx.sync()
    ctx.field_vec_op(K.KG_FR, "mul", a.data_ptr(), b.data_ptr(), ref.data_ptr(), count * n)
    ctx.sync()
    for i in range(count):
        ctx.ntt(ref.data_ptr() + i * n * 32, k, False, True)
    ctx.sync()
    assert torch.equal(got, ref)


def test_errors_leave_the_context_usable(ctx):
    import torch
    so, h = ctx._lib, ctx._h
    k, count, stride = 4, 3, 16 + 5
    x = _fill(ctx, k, count, stride, SEED + 7400)
    work = x.clone()
    torch.cuda.synchronize()
    p = C.c_void_p(work.data_ptr())
    for args in ((h, p, k, count, 15), (h, p, 0, count, stride), (h, p, 29, 1, 1 << 29), (h, None, k, count, stride), (None, p, k, count, stride)):
        assert so.kg_ntt_bn254_fr_batch(*args, 0, 0) == -2, args[2:]
        assert so.kg_fr_divide_by_z_on_coset_batch(*args) == -2, args[2:]
    assert so.kg_ntt_bn254_fr_batch(h, p, k, 0, stride, 0, 0) == 0 and so.kg_fr_divide_by_z_on_coset_batch(h, p, k, 0, stride) == 0    # count == 0: KG_OK
    ctx.sync()
    assert torch.equal(work, x), "a refused or empty call touched the data"
    ctx.ntt_batch(work.data_ptr(), k, count, stride, False, False)
    ctx.sync()
    assert torch.equal(work, _single(ctx, x, k, False, False))


@pytest.mark.parametrize("k", [3, 10, 13])
def test_divide_by_z_batched(ctx, pyoracle, k):
    """every element of every transform * (7^n - 1)^-1, gaps untouched: against the single call per transform, and for 2^3 against
    Python integers"""
    import torch
    n, count = 1 << k, 3
    stride = n + 5
    x = _fill(ctx, k, count, stride, SEED + 7500 + k)
    got, ref = x.clone(), x.clone()
    torch.cuda.synchronize()
    ctx.divide_by_z_on_coset_batch(got.data_ptr(), k, count, stride)
    for b in range(count):
        ctx.divide_by_z_on_coset(ref.data_ptr() + b * stride * 32, k)
    ctx.sync()
    assert torch.equal(got[:, n:], x[:, n:]), "a gap was written"
    assert torch.equal(got, ref)
    if k == 3:
        from helpers import I
        r = pyoracle.R_MOD
        zinv = pow(pow(7, 8, r) - 1, -1, r)
        g, s = _host(got), _host(x)
        for b in range(count):
            for i in range(n):
                assert I(g[b, i]) == I(s[b, i]) * zinv % r, (b, i)       # Montgomery form in and out: the factor is a plain constant


@pytest.mark.parametrize("k", [5, 12])
def test_python_wrappers(ctx, k):
    """api.Fft.batch / divide_by_z_on_coset_batch against the per-row methods; ragged rows are zero-padded per row"""
    import kogarashi_amd as K
    from oracle import oracle as O
    n = 1 << k
    rows = [O.gen_scalars(0, SEED + 7600 + k + b, 0, n - b) for b in range(3)]            # lengths n, n - 1, n - 2
    f = K.Fft(k, ctx=ctx)
    for name, (inv, coset) in VARIANTS.items():
        got = f.batch(rows, inverse=inv, coset=coset)
        assert got.shape == (3, n, 4)
        for b, v in enumerate(rows):
            assert (got[b] == getattr(f, name)(v)).all(), (k, name, b)
    got = f.divide_by_z_on_coset_batch(rows)
    for b, v in enumerate(rows):
        assert (got[b] == f.divide_by_z_on_coset(v)).all(), (k, b)
    assert f.batch([]).shape == (0, n, 4)
