"""Cases for kg_r1cs_check_batch and kg_groth16_witness_check_batch, shared by the host test (tests/test_r1cs_check_batch_host.py: the
self-checks of the case set) and the GPU tests (tests/test_gpu_r1cs_check_batch.py, tests/test_gpu_witness_check_batch.py).  Built on
tests/r1cs_cases.py: a case is one Shape and a list of vectors (z, u, E); what a vector must give comes from RC.expected() on Python integers.

Every vector of a case has its own summary pair (bad rows, first bad row), so an implementation that ignores the vector index, or folds two
vectors into one pair, cannot pass -- and so that this also holds when the same z array is checked with d_u = d_e = NULL (u = 1, E = 0: what a
row gives then depends on z alone), the vectors differ in z as well: z with its tail zeroed at different places.  m = 1 is the exception: a
single row has only the summaries (0, 1) and (1, 0); both occur."""
import types

import numpy as np

import r1cs_cases as RC

GUARD8 = np.uint8(0xA5)
GUARD32 = np.uint32(0xA5A5A5A5)
GUARD64 = np.uint64(0xA5A5A5A5A5A5A5A5)
SMALL_SIZES = (1, 13, 64, 65, 257)          # a single row; the first size with long rows; a full wave; one row more; a workgroup and one row
YMAX_COUNT = 65537                          # chunks of 65535 and 2 vectors


class Vec:
    """one vector of a batch: z and its row sums, u as the entry takes it and as an integer, E as integers"""

    def __init__(self, name, z, prods, u, ui, e, long_bad=False):
        self.name, self.z, self.prods, self.u, self.ui, self.e, self.long_bad = name, z, prods, u, ui, e, long_bad

    def want(self, sh, plain=False):
        """(status, bad, first) from Python integers; plain: what d_u = d_e = NULL gives on the same z"""
        return RC.expected(sh, 1 if plain else self.ui, None if plain else self.e, self.prods)


def masked(sh, keep):
    """sh.z with the entries from index `keep` on zeroed, and the row sums that go with it"""
    z = sh.z.copy()
    z[keep:] = 0
    return z, sh.row_sums(z)


_CACHE = {}


def case300(O, fd):
    """(Shape at m = 300, six vectors): satisfied; E perturbed at perturbed_rows(m); flip_z() under an E made for the old z (bad through the
    long row and two short rows); every row bad; u = 0; u = p - 1"""
    if ("c300", fd) not in _CACHE:
        sh = RC.Shape(O, fd, 300)
        us = {name: (u, ui) for name, u, ui in RC.u_values(O, fd)}
        n, m, p = sh.nvars, sh.m, sh.p
        vecs = []
        z, pr = masked(sh, n // 2)
        vecs.append(Vec("satisfied", z, pr, *us["random"], RC.satisfying_e(sh, us["random"][1], pr)))
        z, pr = masked(sh, n // 4)
        vecs.append(Vec("E perturbed", z, pr, *us["one"], RC.perturb(sh, RC.satisfying_e(sh, 1, pr), RC.perturbed_rows(m)), long_bad=True))
        z, pr = sh.flip_z()
        vecs.append(Vec("flip_z", z, pr, *us["random"], RC.satisfying_e(sh, us["random"][1]), long_bad=True))
        z, pr = masked(sh, 3 * n // 4)
        vecs.append(Vec("every row bad", z, pr, *us["one"], [(x + 1) % p for x in RC.satisfying_e(sh, 1, pr)], long_bad=True))
        z, pr = masked(sh, n // 8)
        vecs.append(Vec("u = 0", z, pr, *us["zero"], RC.perturb(sh, RC.satisfying_e(sh, 0, pr), [RC.LONG_ROW + 3, 20, RC.HUGE_ROW, m - 1]), long_bad=True))
        z, pr = masked(sh, 0)
        vecs.append(Vec("u = p - 1", z, pr, *us["p-1"], RC.perturb(sh, RC.satisfying_e(sh, p - 1, pr), [RC.EDGE48, RC.EDGE49]), long_bad=True))
        _CACHE[("c300", fd)] = (sh, vecs)
    return _CACHE[("c300", fd)]


def small_case(O, fd, m):
    """(Shape, three vectors) at a wave or workgroup edge: satisfied; E perturbed at perturbed_rows(m); the last row alone"""
    if ("small", fd, m) not in _CACHE:
        sh = RC.Shape(O, fd, m)
        us = {name: (u, ui) for name, u, ui in RC.u_values(O, fd)}
        vecs = [Vec("satisfied", sh.z, sh.prods, *us["random"], RC.satisfying_e(sh, us["random"][1])),
                Vec("E perturbed", sh.z, sh.prods, *us["one"], RC.perturb(sh, RC.satisfying_e(sh, 1), RC.perturbed_rows(m)), long_bad=m > 12),
                Vec("last row", sh.z, sh.prods, *us["p-1"], RC.perturb(sh, RC.satisfying_e(sh, sh.p - 1), [m - 1]))]
        _CACHE[("small", fd, m)] = (sh, vecs)
    return _CACHE[("small", fd, m)]


def distinct_summaries(sh, vecs, plain=False):
    s = [v.want(sh, plain)[1:] for v in vecs]
    return len(set(s)) == len(s)


def pack(sh, vecs, z_stride=None, e_stride=None, seed=1):
    """(z[count, z_stride, 4], u[count, 4], E[count, e_stride, 4]) with random words (not canonical: never to be read) in the gaps"""
    z_stride, e_stride = z_stride or sh.nvars, e_stride or sh.m
    rng = np.random.default_rng(seed)
    z = rng.integers(0, 1 << 63, (len(vecs), z_stride, 4), dtype=np.uint64) | np.uint64(1 << 63)
    e = rng.integers(0, 1 << 63, (len(vecs), e_stride, 4), dtype=np.uint64) | np.uint64(1 << 63)
    for b, v in enumerate(vecs):
        z[b, :sh.nvars] = v.z
        e[b, :sh.m] = RC.to_mont(v.e, sh.p)
    u = np.stack([v.u for v in vecs])
    return z, u, e


def upload_shape(ctx, sh):
    """the three matrices on the device: (arrays to keep alive, [(row_ptr, col, val) pointers])"""
    dev = [tuple(ctx.upload(np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], dtype=np.uint64))) for a in t) for t in sh.mats]
    return dev, [tuple(d.ptr for d in t) for t in dev]


def ymax_case(O):
    """The grid's y limit: a 3-row shape over 8 variables (Fr) whose row 1 has 49 entries in A only, so that it alone goes on the work list, and
    four z vectors: one that satisfies the plain relation (u = 1, E = 0) and three that break one row each.  Returns (shape, base, {vector
    index: Vec}) for a batch of YMAX_COUNT copies of the base with vectors 65534, 65535, 65536 replaced: the last of the first chunk and both
    of the second, bad at rows 2, 0 and 1 -- row 1 through the list the first chunk built.
      row 0: z1 * z2 = z3      row 1: (24 z4 - 24 z4 + z1) * z2 = z6      row 2: z5 * z0 = z5      with z0 = 1, z3 = z6 = z1 z2"""
    if "ymax" not in _CACHE:
        fd, p = 0, RC.MODULI[0]
        one = O.f_consts(fd)["r"]
        neg = O.f_neg(fd, one)

        def csr(rows):
            rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
            col = np.array([c for r in rows for c, _ in r], dtype=np.uint64)
            val = np.ascontiguousarray(np.stack([v for r in rows for _, v in r]))
            return rp, col, val
        a = csr([[(1, one)], [(4, one), (4, neg)] * 24 + [(1, one)], [(5, one)]])
        b = csr([[(2, one)], [(2, one)], [(0, one)]])
        c = csr([[(3, one)], [(6, one)], [(5, one)]])
        sh = types.SimpleNamespace(O=O, fd=fd, m=3, p=p, nvars=8, mats=[a, b, c])
        sh.row_sums = lambda z: [RC.to_ints(O.matrix_prod(fd, t, z), p) for t in sh.mats]
        sh.row_lengths = lambda: np.stack([np.diff(t[0].astype(np.int64)) for t in sh.mats])
        r = RC.to_ints(O.gen_scalars(fd, RC.SEED + 4700, 0, 5), p)
        ints = [1, r[0], r[1], r[0] * r[1] % p, r[2], r[3], r[0] * r[1] % p, r[4]]

        def vec(name, change):
            zi = list(ints)
            for k, v in change.items():
                zi[k] = v
            z = RC.to_mont(zi, p)
            return Vec(name, z, sh.row_sums(z), one, 1, None, long_bad=6 in change)
        base = vec("base", {})
        sh.z, sh.prods = base.z, base.prods
        special = {65534: vec("row 2", {0: 2}), 65535: vec("row 0", {3: (ints[3] + 1) % p}), 65536: vec("row 1", {6: (ints[6] + 1) % p})}
        _CACHE["ymax"] = (sh, base, special)
    return _CACHE["ymax"]
