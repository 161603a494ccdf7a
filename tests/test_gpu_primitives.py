"""The field, curve and digit primitives of csrc/ ON THE DEVICE, one at a time (tests/device/devprobe.hip: test kernels around the product's own
templates, the case lines shared with the host build through tests/host/arith_cases.h).

The rest of the GPU suite reaches this arithmetic only through whole MSMs, transforms and provers on random data; tests/test_host_arith.py checks
the edges, but of the HOST build: there the column sums of fp29.h are a C loop (on the device chains of v_mad_u64_u32 / v_mad_i64_i32, the modulus
in scalar registers), and the lane-cooperative formulas move values by array indexing (on the device by DPP quad_perm).  Here the same operand
arrays as in the CPU twins go through the GPU; every output is checked with Python integers (primitive_cases.py: congruence and documented
postcondition, no tolerance) and must equal the host's output bit for bit."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import primitive_cases as PC
from helpers import CURVES, U8P, np_to_pt, p32, pt_to_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devlib():
    """tests/device/libdevprobe.so: rebuilt when missing or older than its sources if hipcc is here, used as it is when hipcc is not, and a
    FAILURE when there is neither a library nor a compiler"""
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


@pytest.fixture(scope="module")
def raw_batches(hostlib):
    B = {fd: PC.raw_batches(fd) for fd in (0, 1)}
    for fd in (0, 1):
        for b in B[fd]["mulc"]:
            PC.mulc_constants(hostlib, fd, b)   # make_const on the host, passed in
    return B


@pytest.mark.parametrize("fd", [0, 1])
def test_raw_limb_primitives(devlib, hostlib, raw_batches, fd):
    """every raw-limb primitive of fp29.h, every operand class (canonical specials, limb patterns, non-canonical values, lazy limbs and K at each
    primitive's stated maximum, the double products' relations): postcondition by exact integers, bits equal to the host's"""
    for prim, batches in raw_batches[fd].items():
        for b in batches:
            out = PC.dev_raw(devlib, fd, prim, b)
            PC.check_batch(fd, prim, b, out)
            assert (out == PC.host_raw(hostlib, fd, 0, prim, b)).all(), (prim, b.name)


def test_fq2_raw_primitives(devlib, hostlib):
    for op, batches in PC.raw2_batches().items():
        for b in batches:
            out = PC.dev_raw2(devlib, op, b)
            PC.check_batch2(op, b, out)
            assert (out == PC.host_raw2(hostlib, 0, op, b)).all(), (op, b.name)


def dev_field_ops(D, fd, op, a, b):
    o = np.zeros_like(a)
    st = D.dp_field_ops(fd, op, p32(a.view(np.uint32)), p32(b.view(np.uint32)), p32(o.view(np.uint32)), C.c_size_t(a.shape[0]))
    assert st == 0, f"HIP status {st}"
    return o


@pytest.mark.parametrize("fd,n", [(0, 4096), (1, 4096), (2, 1024)])
def test_both_inversions(devlib, hostlib, oracle, fd, n):
    """inv_fast and the Fermat inv on ABI-form elements: all specials and n oracle-seeded elements; 0 -> 0, both equal pow(a, -1, p), a * a^-1 = 1"""
    a = PC.inversion_operands(oracle, fd, n)
    want = PC.inversion_expected(fd, a)
    assert (dev_field_ops(devlib, fd, 9, a, a) == want).all()
    assert (dev_field_ops(devlib, fd, 6, a, a) == want).all()
    prod = dev_field_ops(devlib, fd, 0, a, want)
    one = np.zeros_like(a[0]); one[:4] = oracle.f_consts(1 if fd == 2 else fd)["r"]
    nz = a.any(axis=1)
    assert (prod[nz] == one).all() and not prod[~nz].any()


@pytest.mark.parametrize("fd", [0, 1, 2])
def test_abi_form_field_ops_equal_the_host(devlib, hostlib, oracle, fd):
    """the per-element switch of ht_field_ops (mul, sqr, add, sub, neg, dbl, the lazy chain, the round trip) on the specials: the host's bits"""
    a = PC.inversion_operands(oracle, fd, 256)
    b = np.ascontiguousarray(a[::-1])
    for op in (0, 1, 2, 3, 4, 5, 7, 8):
        assert (dev_field_ops(devlib, fd, op, a, b) == PC.host_field_ops(hostlib, fd, 0, op, a, b)).all(), op


def dev_curve_ops(D, cid, op, p, q):
    o = np.zeros((p.shape[0], p.shape[1] // 2), dtype=np.uint64)
    inf = np.zeros(p.shape[0], dtype=np.uint8)
    st = D.dp_curve_ops(cid, op, p32(p.view(np.uint32)), p32(q.view(np.uint32)), p32(o.view(np.uint32)), inf.ctypes.data_as(U8P), C.c_size_t(p.shape[0]))
    assert st == 0, f"HIP status {st}"
    return o, inf


@pytest.mark.parametrize("name", ["g1", "gk", "g2"])
def test_one_lane_point_formulas(devlib, hostlib, pyoracle, name):
    """double_affine, double_xyzz, add_mixed, add_mixed_signed (both signs), add_xyzz, the _stream forms in place, neg_xyzz, to_affine: A+B, A+A,
    A+(-A), O+A, A+O, O+O, 2A+(-A) against the big-integer oracle, and the host's bits"""
    cid, cur, _ = CURVES[name]
    for opname, op in PC.CURVE_OPS.items():
        p, q, want, names = PC.curve_case_arrays(cur, opname)
        o, inf = dev_curve_ops(devlib, cid, op, p, q)
        for i in range(len(want)):
            assert np_to_pt(cur, o[i], inf[i]) == want[i], (name, opname, names[i], i)
        ho, hinf = PC.host_curve_ops(hostlib, cid, 0, op, p, q)
        assert (o == ho).all() and (inf == hinf).all(), (name, opname)


@pytest.mark.parametrize("name", ["g1", "gk", "g2"])
def test_cooperative_levels_over_mixed_waves(devlib, hostlib, pyoracle, name):
    """coop_add_level then coop_dbl_level over an LDS image, one wave per workgroup: every wave holds ordinary, copy, doubling, cancelling and
    idle quads at once (asserted), plus one all-ordinary and one all-exceptional wave; results in a third item and in place, 0..3 doublings"""
    cid, cur, _ = CURVES[name]
    items, params, want, kinds = PC.coop_waves(cur)
    PC.assert_coop_waves_are_mixed(kinds)
    n = items.shape[0]
    o = np.zeros((n, items.shape[1] // 2), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    st = devlib.dp_coop_ops(cid, p32(items.view(np.uint32)), p32(params), C.c_size_t(n // PC.COOP_ITEMS), p32(o.view(np.uint32)), inf.ctypes.data_as(U8P))
    assert st == 0, f"HIP status {st}"
    for i in range(len(want)):
        assert np_to_pt(cur, o[i], inf[i]) == want[i], (name, "wave", i // PC.COOP_ITEMS, "quad", (i % PC.COOP_ITEMS) // 3, "item", i % 3)
    ho, hinf = PC.host_coop_ops(hostlib, cid, 0, items, params)
    assert (o == ho).all() and (inf == hinf).all()


def test_signed_window_digits(devlib, hostlib):
    """small_bias / small_window_digit for c = 2..16: the digits recompose the scalar, |digit| <= 2^(c-1), the host's bits"""
    import random
    rnd = random.Random(16)
    r_mod, q_mod = PC.MODS[0], PC.MODS[1]
    for c in range(2, 17):
        ks = [0, 1, 2, r_mod - 1, q_mod - 1, 1 << (c - 1), (1 << (c - 1)) - 1, (1 << c) - 1, (1 << 253) + 12345, (1 << 254) - 1]
        ks += [rnd.randrange(q_mod) for _ in range(150)] + [sum(((1 << (c - 1)) - (j & 1)) << (j * c) for j in range(254 // c)) % q_mod]
        kw = PC.kwords(ks)
        dig = np.zeros((len(ks), 128), dtype=np.int32)
        hdig = np.zeros_like(dig)
        st = devlib.dp_small_digits(p32(kw), C.c_size_t(len(ks)), c, dig.ctypes.data_as(C.POINTER(C.c_int32)))
        assert st == 0, f"HIP status {st}"
        W = (255 + c - 1) // c
        for k, row in zip(ks, dig):
            assert sum(int(row[w]) << (w * c) for w in range(W)) == k and not row[W:].any(), (c, hex(k))
            assert all(abs(int(row[w])) <= 1 << (c - 1) for w in range(W)) and row[W - 1] >= 0, (c, hex(k))
        hostlib.ht_small_digits(p32(kw), C.c_size_t(len(ks)), c, hdig.ctypes.data_as(C.POINTER(C.c_int32)))
        assert (dig == hdig).all(), c


def dev_glv_decompose(D):
    def call(fd, kw, n, k1, k2, neg):
        st = D.dp_glv_decompose(fd, kw, n, k1, k2, neg)
        assert st == 0, f"HIP status {st}"
    return call


@pytest.mark.parametrize("fd", [0, 1])
def test_glv_decomposition_and_digit_path(devlib, hostlib, pyoracle, fd):
    """glv_decompose_with for both lattices at the edge scalars, the rounding boundaries of c_i and 2000 random scalars: k1 + k2 lambda = k (mod n),
    both halves below 3 * 2^125, the halved digit path recomposes with |digit| <= 2^(c-1), all bits equal to ht_glv_decompose / ht_glv_digits"""
    curve = pyoracle.G1 if fd == 0 else pyoracle.GRUMPKIN
    n, lam = curve.n, PC.glv_module().consts(curve)[0]
    edges, bound, rand = PC.glv_edge_scalars(fd, n, lam)
    ks = edges + bound + rand
    k1, k2, neg = PC.glv_decompose(dev_glv_decompose(devlib), fd, ks)
    PC.check_glv_halves(ks, k1, k2, neg, lam, n)
    h1, h2, hneg = PC.glv_decompose(hostlib.ht_glv_decompose, fd, ks)
    assert (k1 == h1).all() and (k2 == h2).all() and (neg == hneg).all()
    kw = PC.kwords(ks)
    for c in (2, 3, 4, 5, 8, 10, 13, 16):
        dig = np.zeros((len(ks), 2, 64), dtype=np.int32)
        hdig = np.zeros_like(dig)
        st = devlib.dp_glv_digits(fd, p32(kw), C.c_size_t(len(ks)), c, dig.ctypes.data_as(C.POINTER(C.c_int32)))
        assert st == 0, f"HIP status {st}"
        W = (128 + c - 1) // c
        PC.check_glv_digits(ks, dig, W, c, lam, n)
        hostlib.ht_glv_digits(fd, p32(kw), C.c_size_t(len(ks)), c, hdig.ctypes.data_as(C.POINTER(C.c_int32)))
        assert (dig == hdig).all(), c


@pytest.mark.parametrize("name", ["g1", "gk", "g2"])
def test_endomorphism_is_multiplication_by_lambda(devlib, pyoracle, name):
    """msm::SmEndo<F, SP>::apply (msm_small_kernels.h) on the generator, 16 random subgroup points and their negatives: (beta x, y) = lambda P; and
    with the decomposition on the device, +-|k1| P +- |k2| (beta x, y) = k P at the edge scalars, all four sign combinations met"""
    import random
    cid, cur, sfd = CURVES[name]
    lam = PC.glv_module().consts(pyoracle.GRUMPKIN if name == "gk" else pyoracle.G1)[0]
    rnd = random.Random(31 + cid)
    base = [cur.gen] + [cur.mul(cur.gen, rnd.randrange(1, cur.n)) for _ in range(16)]
    base += [cur.neg(b) for b in base]
    pts = np.stack([pt_to_np(cur, b) for b in base])
    o = np.zeros_like(pts)
    st = devlib.dp_endo(cid, p32(pts.view(np.uint32)), p32(o.view(np.uint32)), C.c_size_t(len(base)))
    assert st == 0, f"HIP status {st}"
    endo = [np_to_pt(cur, o[i], 0) for i in range(len(base))]
    for b, e in zip(base, endo):
        assert e == cur.mul(b, lam), name
    edges, bound, _ = PC.glv_edge_scalars(sfd, cur.n, lam)
    ks = edges + bound[::3]
    k1, k2, neg = PC.glv_decompose(dev_glv_decompose(devlib), sfd, ks)
    val4 = lambda w: sum(int(w[j]) << (32 * j) for j in range(4))
    signs = set()
    for i, k in enumerate(ks):
        b, e = base[i % len(base)], endo[i % len(base)]
        t1, t2 = cur.mul(b, val4(k1[i])), cur.mul(e, val4(k2[i]))
        got = cur.add(cur.neg(t1) if neg[i, 0] else t1, cur.neg(t2) if neg[i, 1] else t2)
        assert got == cur.mul(b, k), (name, hex(k))
        if val4(k1[i]) and val4(k2[i]):
            signs.add((int(neg[i, 0]), int(neg[i, 1])))
    assert len(signs) == 4, signs
