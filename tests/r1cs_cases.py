"""Cases for kg_r1cs_check, shared by the host test (tests/test_r1cs_check_host.py) and the GPU test (tests/test_gpu_r1cs_check.py).

A case is a random R1CS shape with every row class the kernels tell apart, a vector z, a scalar u and an error vector E.  The row sums
A z, B z, C z come from the oracle's SparseMatrix::prod; everything after them is Python integers: E := Az o Bz - u Cz makes every row hold,
then a chosen row set is perturbed, and the expected status byte of a row is (Az_i Bz_i - u Cz_i - E_i) mod p != 0 on the final inputs."""
import struct

import numpy as np

from oracle import pyoracle as P

SEED = 0x4B6F676172617368
MODULI = {0: P.R_MOD, 1: P.Q_MOD}
KG_ROW_UNSAT = 1
LONG_ROW, EDGE48, EDGE49, HUGE_ROW = 7, 8, 9, 61        # rows of 200 (all matrices), exactly 48 (A only), exactly 49 (C only), 5000 (B only) entries
EMPTY_A, EMPTY_B = 3, 5                                 # rows with no entry in any matrix
FLIP_SHORT_B, FLIP_SHORT_C = 11, 12                     # short rows that read the z entry flip_z() changes, beside LONG_ROW (through A)


def to_ints(arr, p):
    """(n, 4) Montgomery limbs -> canonical Python integers"""
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    rinv = pow(1 << 256, -1, p)
    return [int.from_bytes(b[i:i + 32], "little") * rinv % p for i in range(0, len(b), 32)]


def to_mont(vals, p):
    """Python integers -> (n, 4) Montgomery limbs"""
    r = (1 << 256) % p
    return np.frombuffer(b"".join((v % p * r % p).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def random_shape(O, fd, m, nvars, seed, max_row=6):
    """three random sparse matrices over z = (u | x | w) (tests/test_gpu_nova.py runs the cross term and the product on them as well): empty
    rows -- two of them empty in all three matrices --, repeated columns, coefficients +-1, a row of 200 entries, rows of exactly 48 and 49
    entries in one matrix only, rows of 254 entries at different constraints in A, B and C, one row of 5000 entries"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(3):
        counts = rng.integers(0, max_row + 1, m)
        counts[EMPTY_A % m] = 0
        if m > 12:
            counts[EMPTY_B] = 0
            counts[LONG_ROW] = 200                       # past 48 entries a row gets a wave of its own (work list)
            counts[EDGE48] = 48 if j == 0 else counts[EDGE48]
            counts[EDGE49] = 49 if j == 2 else counts[EDGE49]
            counts[[FLIP_SHORT_B, FLIP_SHORT_C]] = np.maximum(counts[[FLIP_SHORT_B, FLIP_SHORT_C]], 1)
        if m > 100:
            counts[20 + j:60:7] = 254                    # range-check-like rows, at different constraints in A, B and C
            counts[HUGE_ROW] = 5000 if j == 1 else counts[HUGE_ROW]
        rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        col = rng.integers(0, nvars, int(rp[-1])).astype(np.uint64)
        val = O.gen_scalars(fd, seed + 10 + j, 0, max(int(rp[-1]), 1))[: int(rp[-1])]
        one = O.f_consts(fd)["r"]
        val[::5] = one                                   # R1CS coefficients are mostly +-1
        val[1::7] = O.f_neg(fd, one)
        if m > 12:                                       # one z entry read by the long row (A) and by two short rows (B, C)
            col[int(rp[(LONG_ROW, FLIP_SHORT_B, FLIP_SHORT_C)[j]])] = nvars - 1
        out.append((rp, col, np.ascontiguousarray(val)))
    return out


class Shape:
    """a shape, a z vector and the three row-sum vectors as Python integers (computed once per z)"""

    def __init__(self, O, fd, m, seed=SEED + 4000):
        self.O, self.fd, self.m, self.p = O, fd, m, MODULI[fd]
        self.nvars = 1 + 3 + max(m // 2, 4)
        self.mats = random_shape(O, fd, m, self.nvars, seed + 16 * m + fd)
        self.z = O.gen_scalars(fd, seed + 16 * m + fd + 5, 0, self.nvars)
        self.prods = self.row_sums(self.z)

    def row_sums(self, z):
        return [to_ints(self.O.matrix_prod(self.fd, t, z), self.p) for t in self.mats]

    def row_lengths(self):
        return np.stack([np.diff(t[0].astype(np.int64)) for t in self.mats])

    def flip_z(self):
        """z with its last entry changed (+1), and the row sums that go with it"""
        z = self.z.copy()
        z[-1] = to_mont([to_ints(z[-1:], self.p)[0] + 1], self.p)[0]
        return z, self.row_sums(z)


def u_values(O, fd):
    """[(name, what the entry is handed (None: NULL), the integer)]"""
    p = MODULI[fd]
    rnd = O.gen_scalars(fd, SEED + 4100 + fd, 0, 1)
    return [("null", None, 1), ("one", to_mont([1], p)[0], 1), ("zero", to_mont([0], p)[0], 0), ("p-1", to_mont([p - 1], p)[0], p - 1),
            ("random", rnd[0].copy(), to_ints(rnd, p)[0])]


def satisfying_e(sh, ui, prods=None):
    az, bz, cz = prods or sh.prods
    return [(a * b - ui * c) % sh.p for a, b, c in zip(az, bz, cz)]


def perturbed_rows(m):
    """row 0, the last row, the last lane of a wave and the first of the next, the last lane of a workgroup and the first of the next, a row
    empty in all matrices, a work-list row, an ordinary row after a work-list row"""
    return sorted({r for r in (0, m - 1, 63, 64, 255, 256, EMPTY_A, LONG_ROW, LONG_ROW + 3) if 0 <= r < m})


def perturb(sh, e, rows):
    """E with the given rows changed: +1, -1 and replaced by 0 in turn; a true value of 0 always becomes 1"""
    e, k = list(e), 0
    for r in rows:
        if e[r] == 0:
            e[r] = 1
        else:
            e[r] = ((e[r] - 1) % sh.p, 0, (e[r] + 1) % sh.p)[k % 3]
            k += 1
    return e


def expected(sh, ui, e, prods=None):
    """(status bytes, bad, first_bad) from Python integers; e: integers or None (E = 0)"""
    az, bz, cz = prods or sh.prods
    e = e if e is not None else [0] * sh.m
    st = np.array([KG_ROW_UNSAT if (a * b - ui * c - x) % sh.p else 0 for a, b, c, x in zip(az, bz, cz, e)], dtype=np.uint8)
    bad = np.flatnonzero(st)
    return st, len(bad), int(bad[0]) if len(bad) else sh.m


def write_record(f, sh, z, u, e):
    """one case for tests/host/r1cs_check_host.cpp: u32 field | u32 flags (1: u given, 2: E given) | u64 m | u64 nvars | per matrix u64 nnz,
    row_ptr (m + 1), col (nnz), val (4 nnz) | z (4 nvars) | u (4, when given) | E (4 m, when given)"""
    f.write(struct.pack("<IIQQ", sh.fd, (1 if u is not None else 0) | (2 if e is not None else 0), sh.m, sh.nvars))
    for rp, col, val in sh.mats:
        f.write(struct.pack("<Q", len(col)))
        for a in (rp, col, val):
            f.write(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
    f.write(np.ascontiguousarray(z, dtype=np.uint64).tobytes())
    if u is not None:
        f.write(np.ascontiguousarray(u, dtype=np.uint64).tobytes())
    if e is not None:
        f.write(np.ascontiguousarray(e, dtype=np.uint64).tobytes())
