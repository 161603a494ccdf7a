"""Operands, exact-integer references and checkers of the primitive-level tests: the SAME arrays go through the host build of the csrc/ templates
(tests/host/hosttest.cpp: plain types, then the bound-tracking FpChecked types) and through the GPU (tests/device/devprobe.hip), and every output
is checked here with Python integers.  The value of a limb vector is sum l[i] 2^(29 i); there are no tolerances.

Where a limit appears (a limb maximum, a K) it is the one the comments of csrc/fp29.h state for the primitive, never something a kernel returned."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np

from helpers import I, L, U8P, np_to_pt, p32
from oracle import pyoracle as P

M29 = (1 << 29) - 1
R261 = 1 << 261
MODS = {0: P.R_MOD, 1: P.Q_MOD}                 # field id of the host library: 0 Fr, 1 Fq
KS = [29 * j for j in range(1, 9)] + [28, 30, 57, 58, 253]
FATZ = [(2, 1), (3, 1), (4, 1), (8, 1), (16, 1), (32, 1), (4, 3), (8, 3), (16, 3), (32, 3)]
U32P = C.POINTER(C.c_uint32)
RAW_OUT = 18

OPS = {"mul": 0, "sqr": 1, "mul2add": 2, "mul2sub": 3, "mul2pm_pos": 4, "mul2pm_neg": 5, "mulc": 6, "add": 7, "dbl": 8, "norm": 9, "vred": 10,
       "reduce_2p": 11, "reduce": 12, "is_zero_2p": 13, "is_zero": 14, "same_limbs": 15, "limbs_from_words": 16, "words_from_limbs": 17,
       "from_ref": 18, "to_ref": 19, "ref_to_int": 20, "int_to_ref": 21, "from_int": 22, "make_const": 23}
OPS.update({f"sub_{c}_{t}": 30 + i for i, (c, t) in enumerate(FATZ)})
WORD_OPS = ("limbs_from_words", "from_ref", "ref_to_int", "int_to_ref", "from_int")     # the operand is 8 words, not 9 limbs


def val(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def limbs(x):
    """normalised limbs: 0..7 below 2^29, the rest in the top limb"""
    assert 0 <= x < 1 << 264
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def words(x):
    assert 0 <= x < 1 << 256
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


def wval(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w[:8]))


def lazy(lo, top):
    """limbs 0..7 all `lo` (may exceed 29 bits), top limb `top`"""
    return [lo] * 8 + [top]


def fat_z(p, c, t):
    """the limbs of C p that sub<C, T> adds: normalised limbs of C p with T 2^29 lent to every limb below the top by the one above it"""
    z = limbs(c * p)
    return [z[0] + (t << 29)] + [z[i] + (t << 29) - t for i in range(1, 8)] + [z[8] - t]


def ptop(p):
    return p >> 232


# ---------------------------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------------------------
def specials(p):
    r256 = (1 << 256) % p
    v = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, r256, pow(r256, -1, p)]
    for k in KS:
        v += [1 << k, (1 << k) - 1, p - (1 << k)]
    return v


def patterns(p):
    """limb patterns below p: one limb 2^29 - 1, low j limbs zero, alternating limbs, every limb below the top 2^29 - 1"""
    rnd = random.Random(0x29)
    t = ptop(p) - 1                                             # a top limb below p's keeps the value below p
    v = [M29 << (29 * i) for i in range(8)] + [t << 232]
    for j in range(1, 9):
        v.append(rnd.randrange(p) >> (29 * j) << (29 * j))
    v.append(val([M29 if i % 2 == 0 else 0 for i in range(8)] + [t]))
    v.append(val([M29 if i % 2 == 1 else 0 for i in range(8)] + [0]))
    v.append(val(lazy(M29, t)))
    v.append(val(lazy(M29, 0)))
    return v


def canon(p):
    return specials(p) + patterns(p)


def noncanon(p):
    return [p, p + 1, 2 * p - 1, 2 * p, (1 << 256) - 1]


class Batch:
    """rows of up to four operands (limb lists) of ONE class: K[j] bounds operand j's value (value < K p), lb / tb its limbs 0..7 / top limb
    (None: normalised, what FpChecked::wrap assumes).  checked=False: beyond what the bound-tracking type admits (run unchecked only)."""

    def __init__(self, name, rows, K, lb=None, tb=None, checked=True, kc=None):
        self.name, self.rows, self.checked = name, [tuple(list(o) for o in r) for r in rows], checked
        n, ar = len(rows), len(rows[0])
        self.K = [Fraction(str(k)) for k in K] + [Fraction(1)] * (4 - len(K))
        self.arr = [np.zeros((n, 9), dtype=np.uint32) for _ in range(4)]
        for i, r in enumerate(self.rows):
            assert len(r) == ar
            for j, o in enumerate(r):
                self.arr[j][i] = o
        self.kc = np.zeros((n, 18), dtype=np.uint32) if kc is None else np.ascontiguousarray(kc, dtype=np.uint32)
        self.bnd = np.zeros((4, 3), dtype=np.float64)
        for j in range(4):
            self.bnd[j] = ((lb[j] if lb and j < len(lb) and lb[j] else 0), (tb[j] if tb and j < len(tb) and tb[j] else 0), float(self.K[j]))
        self.lb = [(lb[j] if lb and j < len(lb) and lb[j] else M29) for j in range(4)]

    def __len__(self):
        return len(self.rows)

    def assert_declared(self, p, word_op=False):
        """the class's own declaration holds for every operand: limbs within lb / tb, value below K p"""
        for r in self.rows:
            for j, o in enumerate(r):
                if word_op:
                    continue
                assert all(v <= self.lb[j] for v in o[:8]), (self.name, j)
                if self.bnd[j][1]:
                    assert o[8] <= self.bnd[j][1], (self.name, j)
                assert val(o) < self.K[j] * p, (self.name, j, hex(val(o)))


def _pairs(vs, shifts):
    n = len(vs)
    return [(vs[i], vs[(i + s) % n]) for s in shifts for i in range(n)]


def _L(rows):
    return [tuple(limbs(x) for x in r) for r in rows]


def raw_batches(fd):
    """primitive -> [Batch]: the operand classes of every raw-limb primitive of fp29.h for field fd"""
    p = MODS[fd]
    rnd = random.Random(1000 + fd)
    V, N = canon(p), noncanon(p)
    R = [rnd.randrange(p) for _ in range(24)]
    T = ptop(p)
    B = {}
    # a value at the top of a K class, and the lazy operands of fp29.h's column rules
    kmax = lambda k: int(Fraction(k) * p) - 1                               # the largest value below K p
    lz31 = lazy((1 << 31) - 1, T - 6)                                       # "limbs 0..7 up to 2^31 - 1 against a normalised partner"
    lz15 = lazy(3 << 30, T - 8)                                             # 9 * 1.5 * 2^31 * 2^29 + 9 * 2^58 + 2^36 = 15.75 * 2^60 < 2^64
    lz30 = lazy(1 << 30, T - 3)
    ones8 = limbs(val(lazy(M29, T - 1)))
    few = [0, 1, p - 1, p - 2, (p + 1) // 2, (1 << 253), val(ones8)] + R[:6]

    B["mul"] = [
        Batch("canonical", _L(_pairs(V, (0, 1, 7))), (1, 1)),
        Batch("non-canonical", _L(_pairs(N + V[:8], (0, 1, 2))), ("5.4", "5.4")),
        Batch("K 13 x 12.99", _L([(kmax(13), kmax("12.99")), (kmax(13), p - 1), (kmax(13), 0)]), (13, "12.99")),
        Batch("K 12.99 x 13", _L([(kmax("12.99"), kmax(13)), (0, kmax(13))]), ("12.99", 13)),
        Batch("K 168 x canonical", _L([(kmax(168), x) for x in few]), (168, 1)),
        Batch("every limb below the top 2^29 - 1, top limb at 168 p", [(lazy(M29, 168 * T - 1), limbs(x)) for x in few], (168, 1)),
        Batch("lazy 2^31 - 1 x normalised", [(lz31, limbs(x)) for x in few + V[:20]], (2, 1), lb=[(1 << 31) - 1, 0], tb=[T, 0]),
        Batch("lazy 3 * 2^30 x normalised", [(lz15, limbs(x)) for x in few], (2, 1), lb=[3 << 30, 0], tb=[T, 0]),
        Batch("lazy 2^30 x lazy 2^30", [(lz30, lz30), (lz30, lazy(1 << 30, 0)), (lazy(1 << 30, 0), lz30)], (2, 2), lb=[1 << 30, 1 << 30], tb=[T, T]),
    ]
    lz12 = lazy(int(1.2 * (1 << 30)), T - 3)                                # 9 * 1.44 * 2^60 + 9 * 2^58 + 2^36 < 2^64, doubled limb < 2^32
    B["sqr"] = [
        Batch("canonical", _L([(x,) for x in V]), (1,)),
        Batch("non-canonical", _L([(x,) for x in N]), ("5.4",)),
        Batch("K 12.99", _L([(kmax("12.99"),), (kmax(12),)]), ("12.99",)),
        Batch("lazy 2^30", [(lz30,), (lazy(1 << 30, 0),)], (2,), lb=[1 << 30], tb=[T]),
        Batch("lazy 1.2 * 2^30", [(lz12,)], (2,), lb=[int(1.2 * (1 << 30))], tb=[T]),
    ]
    quads = [(V[i], V[(i + 1) % len(V)], V[(i + 5) % len(V)], V[(i + 11) % len(V)]) for i in range(len(V))]
    rq = [tuple(rnd.randrange(p) for _ in range(4)) for _ in range(60)]
    # the relations of a double product: a b = c d exactly, one unit apart, one product zero with the other maximal
    u, v, w = [rnd.randrange(1 << 120) for _ in range(3)]
    xs = [x for x in R[:8] if 1 < x < p - 1]
    rel = [(x, y, y, x) for x, y in zip(R[:8], R[8:16])] + [(u * v, w, u, v * w), (u, v * w, u * v, w)]
    rel += [(x + 1, x - 1, x, x) for x in xs] + [(x, x, x + 1, x - 1) for x in xs]
    rel += [(0, x, p - 1, p - 1) for x in R[:4]] + [(x, 0, p - 1, p - 1) for x in R[:4]] + [(p - 1, p - 1, 0, x) for x in R[:4]]
    rel += [(p - 1, p - 1, x, 0) for x in R[:4]] + [(0, 0, 0, 0), (p - 1, p - 1, p - 1, p - 1), (1, 1, 1, 1), (p - 1, 1, 1, p - 1)]
    B["mul2add"] = [
        Batch("canonical", _L(quads + rq + rel), (1, 1, 1, 1)),
        Batch("non-canonical", _L([(N[i], N[(i + 1) % 5], N[(i + 2) % 5], N[(i + 3) % 5]) for i in range(5)]), ("5.4",) * 4),
        Batch("K 9 9 9 9 (162 < 169)", _L([(kmax(9),) * 4, (kmax(9), kmax(9), 0, 0)]), (9, 9, 9, 9)),
        Batch("lazy 2^30 x normalised, twice", [(lz30, limbs(x), lz30, limbs(y)) for x, y in zip(few, few[1:] + few[:1])], (2, 1, 2, 1),
              lb=[1 << 30, 0, 1 << 30, 0], tb=[T, 0, T, 0]),
    ]
    # signed columns: 9 A B + 9 * 2^58 + 2^36 < 2^63 and 9 C D < 2^63 (mul2sub); 9 (A B + C D) + ... < 2^63 (mul2pm)
    lz125 = lazy(5 << 28, T - 3)                                            # 1.25 * 2^30: 9 * 0.625 * 2^60 + 2.25 * 2^60 + 2^36 < 2^63
    lz175 = lazy(7 << 28, T - 4)                                            # 1.75 * 2^30: 9 * 0.875 * 2^60 + 2^36 < 2^63
    lz06 = lazy(int(0.6 * (1 << 30)), T - 2)                                # 9 * 2 * 0.3 * 2^60 + 2.25 * 2^60 + 2^36 < 2^63
    ksub = _L([(kmax(13), kmax("12.99"), kmax(13), kmax("12.99")), (kmax(13), kmax("12.99"), 0, 0), (0, 0, kmax(13), kmax("12.99")),
               (kmax(13), kmax("12.99"), kmax(13) - 5, kmax("12.99") - 7), (kmax(13), 1, kmax(13), 1), (kmax(13), p, kmax(13) - 1, p)])
    B["mul2sub"] = [
        Batch("canonical", _L(quads + rq + rel), (1, 1, 1, 1)),
        Batch("non-canonical", _L([(N[i], N[(i + 1) % 5], N[(i + 2) % 5], N[(i + 3) % 5]) for i in range(5)] + [(x, x, x, x) for x in N]), ("5.4",) * 4),
        Batch("K 13 x 12.99 on both sides", ksub, (13, "12.99", 13, "12.99")),
        # the quotient left by the signed columns is negative when m p < c d - a b for the m < 2^261 that clears the low limbs: one case in 169
        # for canonical operands, nearly every case for a subtrahend near 169 p^2
        Batch("small minuend, subtrahend near 169 p^2", _L([(x % (1 << 64), y, kmax(13) - x, kmax("12.99") - y) for x, y in zip(R[:12], R[12:24])]),
              (1, 1, 13, "12.99")),
        Batch("lazy 1.25 * 2^30 minuend, 1.75 * 2^30 subtrahend",
              [(lz125, limbs(x), lz175, limbs(y)) for x, y in zip(few, few[1:] + few[:1])] + [(lz125, ones8, lz175, ones8)], (2, 1, 2, 1),
              lb=[5 << 28, 0, 7 << 28, 0], tb=[T, 0, T, 0]),
    ]
    pm = [
        Batch("canonical", _L(quads + rq + rel), (1, 1, 1, 1)),
        Batch("non-canonical", _L([(N[i], N[(i + 1) % 5], N[(i + 2) % 5], N[(i + 3) % 5]) for i in range(5)]), ("5.4",) * 4),
        Batch("K 9 9 9 9", _L([(kmax(9),) * 4, (kmax(9), kmax(9), 0, 0), (0, 0, kmax(9), kmax(9)), (kmax(9), 1, 1, kmax(9))]), (9, 9, 9, 9)),
        Batch("lazy 0.6 * 2^30 on both sides", [(lz06, limbs(x), lz06, limbs(y)) for x, y in zip(few, few[1:] + few[:1])] + [(lz06, ones8, lz06, ones8)],
              (2, 1, 2, 1), lb=[int(0.6 * (1 << 30)), 0, int(0.6 * (1 << 30)), 0], tb=[T, 0, T, 0]),
    ]
    B["mul2pm_pos"], B["mul2pm_neg"] = pm, pm
    ws = [0, 1, p - 1] + R[:8]
    mc = lambda name, ops, K, **kw: Batch(name, [(o,) for o in ops for _ in ws], K, **kw)      # every operand against every constant
    B["mulc"] = [
        mc("canonical", [limbs(x) for x in V[:40] + R[:8]], (1,)),
        mc("non-canonical", [limbs(x) for x in N], ("5.4",)),
        mc("K 168.99", [limbs(kmax("168.99")), lazy(M29, 168 * T)], ("168.99",)),
        mc("lazy 2^31 - 1", [lz31, lazy((1 << 31) - 1, 168 * T)], ("168.99",), lb=[(1 << 31) - 1], tb=[168 * T]),
        mc("2^261 - 1 (fp29.h: a < 2^261; above the checker's K < 169)", [[M29] * 9], (170,), checked=False),
    ]
    for b in B["mulc"]:
        b.w = [ws[i % len(ws)] for i in range(len(b))]
    # the quotient estimate drops columns 0..6 of a q: it is one short of floor(a q / 2^261) when a q lies a few units above a multiple of 2^261
    near, near_w = [], []
    for w in ws[1:]:
        q = (w << 261) // p
        for eps in (1, 2, 5):
            a_ = eps * pow(q, -1, R261) % R261 if q % 2 else None
            if a_ is not None and a_ <= kmax("168.99"):
                near.append((limbs(a_),)); near_w.append(w)
    B["mulc"].append(Batch("a q a few units above a multiple of 2^261", near, ("168.99",)))
    B["mulc"][-1].w = near_w
    # the same with a canonical a (K = 1): the output is then a w mod p plus p, within one p of the bound (2 + 1/169) p
    small, small_w = [], []
    for w in R:
        q = (w << 261) // p
        if q % 2 == 0 or len(small) >= 8:
            continue
        qi = pow(q, -1, R261)
        hits = [eps * qi % R261 for eps in range(1, 6000) if eps * qi % R261 < p][:2]
        small += [(limbs(a_),) for a_ in hits]; small_w += [w] * len(hits)
    B["mulc"].append(Batch("canonical a, a q a few units above a multiple of 2^261", small, (1,)))
    B["mulc"][-1].w = small_w
    B["add"] = [
        Batch("canonical", _L(_pairs(V, (0, 3))), (1, 1)),
        Batch("lazy 2^31 - 1 + lazy 2^31 - 1", [(lazy((1 << 31) - 1, (1 << 31) - 1),) * 2, (lz31, lazy((1 << 31) - 1, 0))], (700, 700),
              lb=[(1 << 31) - 1] * 2, tb=[(1 << 31) - 1] * 2),
    ]
    B["dbl"] = [
        Batch("canonical", _L([(x,) for x in V]), (1,)),
        Batch("lazy 2^31 - 1", [(lazy((1 << 31) - 1, (1 << 31) - 1),), (lz31,)], (700,), lb=[(1 << 31) - 1], tb=[(1 << 31) - 1]),
    ]
    big = (1 << 32) - 10                                                    # norm: limb + carry + 1 < 2^32
    B["norm"] = [
        Batch("normalised already", _L([(x,) for x in V + N]), ("5.4",)),
        Batch("lazy 2^32 - 10", [(lazy(big, 1 << 31),), (lazy(big, 0),), ([big if i % 2 else 0 for i in range(8)] + [5],),
                                 ([0 if i % 2 else big for i in range(8)] + [5],), ([M29] * 7 + [big, 7],), ([1 << 29] * 8 + [0],),
                                 ([M29 + 1] + [M29] * 7 + [0],)], (1500,), lb=[big], tb=[1 << 31]),
    ]
    mult = [k * p + d for k in range(0, 40) for d in (0, 1, p // 2, p - 1)]
    B["vred"] = [
        Batch("canonical and below 5.4 p", _L([(x,) for x in V + N]), ("5.4",)),
        Batch("multiples of p up to 40 p", _L([(x,) for x in mult]), (41,), tb=[(1 << 27) - 1]),
        Batch("top limb 2^27 - 1", [(lazy(M29, (1 << 27) - 1),), (lazy(0, (1 << 27) - 1),)], (43,), tb=[(1 << 27) - 1]),
    ]
    two_p = [x for x in V] + [p + x for x in V if p + x < 2 * p] + [p, p + 1, 2 * p - 1]
    B["reduce_2p"] = [Batch("[0, 2p)", _L([(x,) for x in two_p]), (2,))]
    B["reduce"] = [
        Batch("canonical", _L([(x,) for x in V]), (1,)),
        Batch("non-canonical", _L([(x,) for x in N]), ("5.4",)),
        Batch("K 168", _L([(kmax(168),), (168 * p - p,), (167 * p,)]) + [(lazy(M29, 168 * T - 1),)], (168,)),
        Batch("lazy 2^31 - 1", [(lz31,), (lazy((1 << 31) - 1, 0),)], (2,), lb=[(1 << 31) - 1], tb=[T]),
    ]
    flip = [limbs(p)[:i] + [limbs(p)[i] ^ (1 << b)] + limbs(p)[i + 1:] for i in range(9) for b in (0, 28 if i < 8 else 21)]
    flip = [o for o in flip if val(o) < 2 * p]
    B["is_zero_2p"] = [Batch("[0, 2p)", [(limbs(0),)] * 8 + [(limbs(p),)] * 8 + [(o,) for o in flip] +
                             _L([(x,) for x in [1, p - 1, p + 1, 2 * p - 1] + patterns(p)]), (2,))]
    kp = [k * p for k in list(range(0, 12)) + [100, 167]]
    B["is_zero"] = [
        Batch("multiples of p and their neighbours", _L([(x,) for x in kp] + [(x + 1,) for x in kp] + [(x - 1,) for x in kp[1:]]), (168,)),
        Batch("canonical", _L([(x,) for x in V]), (1,)),
        Batch("p with a carry left in limb 3", [(limbs(k * p)[:3] + [limbs(k * p)[3] + (1 << 29), limbs(k * p)[4] - 1] + limbs(k * p)[5:],)
                                                for k in (1, 2, 3, 7)], (8,), lb=[1 << 30], tb=[8 * (T + 1)]),
    ]
    eq = [(limbs(x), limbs(x)) for x in V[:30]]
    ne = [(limbs(p - 1), limbs(p - 1)[:i] + [limbs(p - 1)[i] ^ (1 << b)] + limbs(p - 1)[i + 1:]) for i in range(9) for b in (0, 21)]
    B["same_limbs"] = [Batch("canonical", eq + ne + _L(_pairs(V[:30], (1,))), (2, 2))]
    w256 = V + N + [1 << k for k in range(256)] + [(1 << 256) - 1 - (1 << k) for k in range(0, 256, 5)]
    B["limbs_from_words"] = [Batch("any 256-bit value", [(words(x),) for x in w256], ("5.4",))]
    B["words_from_limbs"] = [Batch("normalised, below 2^256", _L([(x,) for x in w256]), ("5.4",))]
    for name in ("from_ref", "ref_to_int", "int_to_ref", "from_int"):
        B[name] = [Batch("any 256-bit value", [(words(x),) for x in V + N + R], ("5.4",))]
    # from_ref / from_int promise a value below 2p: inputs whose exact Montgomery quotient (w C + m p) / 2^261 lies above p, so that the
    # result is within one p of that bound (C: the conversion constant, 2^266 resp. 2^522 mod p)
    minv = (-pow(p, -1, R261)) % R261
    for name, cst in (("from_ref", (1 << 266) % p), ("from_int", (1 << 522) % p)):
        quot = lambda w: (w * cst + (w * cst * minv % R261) * p) >> 261
        above = [w for w in (rnd.randrange(1 << 256) for _ in range(4000)) if quot(w) >= p][:6]
        B[name].append(Batch("any 256-bit value, result above p", [(words(w),) for w in above], ("5.4",)))
    B["to_ref"] = [
        Batch("canonical", _L([(x,) for x in V + R]), (1,)),
        Batch("non-canonical", _L([(x,) for x in N]), ("5.4",)),
        Batch("K 168", _L([(kmax(168),), (167 * p,)]), (168,)),
        Batch("lazy 2^31 - 1", [(lz31,)], (2,), lb=[(1 << 31) - 1], tb=[T]),
    ]
    B["make_const"] = [Batch("canonical", _L([(x,) for x in V + R]), (1,))]
    for c, t in FATZ:
        z = fat_z(p, c, t)
        bmax = [(t << 29) - t] * 8 + [z[8]]                                 # fp29.h: limbs 0..7 of b <= T 2^29 - T, top limb <= the constant's
        amax = [(1 << 32) - 2 - max(z[:8])] * 8 + [(1 << 32) - 2 - z[8]]    # the sum a + Z stays below 2^32 in every limb
        bk = Fraction(val(bmax), p) + 1
        B[f"sub_{c}_{t}"] = [
            Batch("canonical", _L(_pairs(V[:40], (0, 1))), (1, 1)),
            Batch("b at its limits, a normalised", [(limbs(x), bmax) for x in few] + [(limbs(x), [0] * 8 + [z[8]]) for x in few[:3]] +
                  [(limbs(x), [(t << 29) - t] * 8 + [0]) for x in few[:3]], (1, bk), lb=[0, (t << 29) - t], tb=[0, z[8]]),
            Batch("a and b at their limits", [(amax, bmax), (amax, [0] * 9), ([0] * 9, bmax)], (Fraction(val(amax), p) + 1, bk),
                  lb=[amax[0], (t << 29) - t], tb=[amax[8], z[8]]),
        ]
    return B


# ---------------------------------------------------------------------------------------------------------------------------------------
# checkers: raise AssertionError unless `out` (18 words) is what the primitive promises for the row
# ---------------------------------------------------------------------------------------------------------------------------------------
def _normalised(o):
    return all(v <= M29 for v in o[:9])


def _mont(p, o, num, kk):
    """o 2^261 = num (mod p), limbs below 2^29, value below (kk / 169 + 1) p"""
    assert _normalised(o), "limbs not below 2^29"
    x = val(o[:9])
    assert (x * R261 - num) % p == 0, "congruence"
    assert x * 169 < (kk + 169) * p, "value above (K / 169 + 1) p"


def mulc_quotients(p, a, w):
    """(floor(a q / 2^261), the estimate mulc forms from columns 7..16 of a q): census only"""
    q = limbs((w << 261) // p)
    cols = [sum(a[i] * q[k - i] for i in range(9) if 0 <= k - i < 9) for k in range(17)]
    est = sum(cols[k] << (29 * (k - 7)) for k in range(7, 17)) >> 58
    return (val(a) * val(q)) >> 261, est


def check_raw(fd, prim, batch, i, o):
    p = MODS[fd]
    r = batch.rows[i]
    K = batch.K
    o = [int(v) for v in o]
    v = [val(x) for x in r]
    if prim == "mul":
        _mont(p, o, v[0] * v[1], K[0] * K[1])
    elif prim == "sqr":
        _mont(p, o, v[0] * v[0], K[0] * K[0])
    elif prim == "mul2add":
        _mont(p, o, v[0] * v[1] + v[2] * v[3], K[0] * K[1] + K[2] * K[3])
    elif prim in ("mul2sub", "mul2pm_neg", "mul2pm_pos"):
        num = v[0] * v[1] + (v[2] * v[3] if prim == "mul2pm_pos" else -v[2] * v[3])
        assert _normalised(o), "limbs not below 2^29"
        assert (val(o[:9]) * R261 - num) % p == 0, "congruence"
        assert 0 <= val(o[:9]) < 2 * p, "value outside [0, 2p)"
    elif prim == "mulc":
        assert _normalised(o), "limbs not below 2^29"
        assert (val(o[:9]) - v[0] * batch.w[i]) % p == 0, "congruence"
        assert val(o[:9]) * 169 < (2 * 169 + K[0]) * p, "value above (2 + K / 169) p"
    elif prim == "add":
        assert o[:9] == [x + y for x, y in zip(r[0], r[1])]
    elif prim == "dbl":
        assert o[:9] == [2 * x for x in r[0]]
    elif prim == "norm":
        assert val(o[:9]) == v[0], "value changed"
        assert all(x <= M29 for x in o[:8]), "limbs 0..7 not below 2^29"
    elif prim == "vred":
        assert _normalised(o) and (val(o[:9]) - v[0]) % p == 0, "congruence / limbs"
        assert val(o[:9]) * 100 < 106 * p, "value above 1.06 p"
    elif prim == "reduce_2p":
        assert o[:9] == limbs(v[0] % p)
    elif prim == "reduce":
        assert o[:9] == limbs(v[0] % p)                                  # (a * one / 2^261: the value itself, canonical)
    elif prim == "is_zero_2p":
        assert o[0] == (1 if v[0] in (0, p) else 0) and not any(o[1:])
    elif prim == "is_zero":
        assert o[0] == (1 if v[0] % p == 0 else 0) and not any(o[1:])
    elif prim == "same_limbs":
        assert o[0] == (1 if r[0] == r[1] else 0) and not any(o[1:])
    elif prim == "limbs_from_words":
        assert o[:9] == limbs(wval(r[0]))
    elif prim == "words_from_limbs":
        assert o[:8] == words(v[0])[:8]
    elif prim == "from_ref":                                                # x 2^256 -> x 2^261, normalised, below 2p
        assert _normalised(o) and (val(o[:9]) - 32 * wval(r[0])) % p == 0 and val(o[:9]) < 2 * p
    elif prim == "to_ref":
        assert o[:8] == words(v[0] * pow(32, -1, p) % p)[:8]
    elif prim == "ref_to_int":
        assert o[:8] == words(wval(r[0]) * pow(1 << 256, -1, p) % p)[:8]
    elif prim == "int_to_ref":
        assert o[:8] == words((wval(r[0]) << 256) % p)[:8]
    elif prim == "from_int":
        assert _normalised(o) and (val(o[:9]) - wval(r[0]) * R261) % p == 0 and val(o[:9]) < 2 * p
    elif prim == "make_const":
        assert o[:9] == r[0] and o[9:18] == limbs((v[0] << 261) // p)
    elif prim.startswith("sub_"):
        c, t = (int(s) for s in prim.split("_")[1:])
        z = fat_z(p, c, t)
        want = [x + zz - y for x, y, zz in zip(r[0], r[1], z)]
        assert all(0 <= x < 1 << 32 for x in want), "the reference itself wraps: not a legal operand"
        assert o[:9] == want, "a + C p - b limb-wise"
        assert val(o[:9]) == v[0] + c * p - v[1], "value"
    else:
        raise KeyError(prim)
    if prim not in ("make_const",) and not prim.startswith("is_") and prim != "same_limbs":
        assert not any(o[9:]), "words beyond the result written"


NORMALISED_OUT = ("mul", "sqr", "mul2add", "mul2sub", "mul2pm_pos", "mul2pm_neg", "mulc", "vred", "reduce_2p", "reduce", "from_ref", "from_int")
CARRY_FREE_OUT = NORMALISED_OUT + ("norm",)                                 # limbs 0..7 below 2^29 promised


def value_bound(prim, batch, p):
    """the value bound the primitive's comment in fp29.h promises for a row of this class (None: no bound on the value)"""
    K = batch.K
    if prim == "mul":
        return (K[0] * K[1] / 169 + 1) * p
    if prim == "sqr":
        return (K[0] * K[0] / 169 + 1) * p
    if prim == "mul2add":
        return ((K[0] * K[1] + K[2] * K[3]) / 169 + 1) * p
    if prim in ("mul2sub", "mul2pm_pos", "mul2pm_neg", "from_ref", "from_int"):
        return 2 * p
    if prim == "mulc":
        return (2 + K[0] / 169) * p
    if prim == "vred":
        return Fraction(106, 100) * p
    if prim in ("reduce_2p", "reduce"):
        return p
    return None


def header_constant(fd, name):
    """a scalar constant of FrParams / FqParams, read from csrc/fp_consts.h"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "kogarashi_amd", "csrc", "fp_consts.h")).read()
    blk = txt.split("struct %s {" % ("FrParams" if fd == 0 else "FqParams"))[1]
    return int(re.search(r"uint32_t %s = (0x[0-9a-fA-F]+)u;" % name, blk).group(1), 16)


def census(fd, B):
    """branch classes met by the operands, from the exact integers alone"""
    p = MODS[fd]
    inv = (-pow(p, -1, R261)) % R261
    cnt = {k: 0 for k in ("mul2sub negative", "mul2sub non-negative", "reduce_2p borrow", "reduce_2p no borrow", "vred q exact", "vred q one short",
                          "mulc estimate exact", "mulc estimate one less", "is_zero_2p by 0", "is_zero_2p by p")}
    mu = header_constant(fd, "MU")                                          # the estimate vred forms is the header's, whatever its comment says
    for b in B["mul2sub"]:
        for r in b.rows:
            num = val(r[0]) * val(r[1]) - val(r[2]) * val(r[3])
            t = (num + (num * inv % R261) * p) >> 261                       # the exact quotient the signed columns leave before the fix-up
            cnt["mul2sub negative" if t < 0 else "mul2sub non-negative"] += 1
    for b in B["reduce_2p"]:
        for r in b.rows:
            cnt["reduce_2p borrow" if val(r[0]) < p else "reduce_2p no borrow"] += 1
    for b in B["vred"]:
        for r in b.rows:
            q = (r[0][8] * mu) >> 32
            d = val(r[0]) // p - q
            assert d in (0, 1), "fp29.h: q is short of floor(value / p) by at most one"
            cnt["vred q exact" if d == 0 else "vred q one short"] += 1
    for b in B["mulc"]:
        for i, r in enumerate(b.rows):
            exact, est = mulc_quotients(p, r[0], b.w[i])
            assert exact - est in (0, 1), "fp29.h: the estimate is floor(a q / 2^261) or one less"
            cnt["mulc estimate exact" if exact == est else "mulc estimate one less"] += 1
    for b in B["is_zero_2p"]:
        for r in b.rows:
            if val(r[0]) == 0:
                cnt["is_zero_2p by 0"] += 1
            if val(r[0]) == p:
                cnt["is_zero_2p by p"] += 1
    return cnt


# ---------------------------------------------------------------------------------------------------------------------------------------
# Fp2<Fq> on raw limbs: op 0 mul, 1 sqr, 2 mul2sub, 3 inv; an operand is (c0 limbs, c1 limbs)
# ---------------------------------------------------------------------------------------------------------------------------------------
class Batch2:
    def __init__(self, name, rows, K):
        self.name, self.rows = name, rows
        self.K = [Fraction(str(k)) for k in K] + [Fraction(1)] * (4 - len(K))
        n = len(rows)
        self.arr = [np.zeros((n, 18), dtype=np.uint32) for _ in range(4)]
        for i, r in enumerate(rows):
            for j, (c0, c1) in enumerate(r):
                self.arr[j][i, :9], self.arr[j][i, 9:] = limbs(c0), limbs(c1)
        self.bnd = np.zeros((4, 3), dtype=np.float64)
        self.bnd[:, 2] = [float(k) for k in self.K]

    def __len__(self):
        return len(self.rows)


def raw2_batches():
    p = P.Q_MOD
    rnd = random.Random(2002)
    V = canon(p)
    R = [rnd.randrange(p) for _ in range(40)]
    el = [(V[i], V[(i + 9) % len(V)]) for i in range(len(V))] + [(R[i], R[i + 1]) for i in range(0, 40, 2)]
    pairs = [(el[i], el[(i + 3) % len(el)]) for i in range(len(el))]
    xs = R[:8]
    rel = [((x, y), (y, x)) for x, y in zip(R[:8], R[8:16])]                # a0 b0 = a1 b1 exactly
    rel += [((x + 1, x), (x - 1, x)) for x in xs] + [((x, x + 1), (x, x - 1)) for x in xs]      # one unit apart, either way
    rel += [((0, p - 1), (x, p - 1)) for x in xs[:4]] + [((p - 1, 0), (p - 1, x)) for x in xs[:4]]   # one product zero, the other maximal
    rel += [((0, 0), (0, 0)), ((p - 1, p - 1), (p - 1, p - 1)), ((1, 0), (R[2], R[3])), ((R[2], 0), (R[3], 0)), ((0, R[2]), (0, R[3]))]
    k6 = 6 * p - 1
    quad = [(el[i], el[(i + 3) % len(el)], el[(i + 5) % len(el)], el[(i + 8) % len(el)]) for i in range(len(el))]
    quad += [(a, b, b, a) for a, b in pairs[:10]] + [(a, b, a, b) for a, b in pairs[:10]]
    nonc = noncanon(p)
    inv_el = el + [(0, 0), (1, 0), (0, 1), (p - 1, 0), (0, p - 1)]
    return {
        0: [Batch2("canonical", pairs + rel, (1, 1)), Batch2("non-canonical", [((nonc[i], nonc[(i + 1) % 5]), (nonc[(i + 2) % 5], nonc[(i + 3) % 5])) for i in range(5)], ("5.4", "5.4")),
            Batch2("K 9", [((9 * p - 1, 9 * p - 1), (9 * p - 1, 9 * p - 1)), ((9 * p - 1, 0), (0, 9 * p - 1))], (9, 9))],
        1: [Batch2("canonical", [(a,) for a in el], (1,)), Batch2("K 6 (fp29.h: K <= 6)", [((k6, k6),), ((k6, 0),), ((0, k6),), ((k6, 1),), ((5 * p, k6),)], (6,)),
            Batch2("non-canonical", [((nonc[i], nonc[(i + 1) % 5]),) for i in range(5)], ("5.4",))],
        2: [Batch2("canonical", quad, (1, 1, 1, 1))],
        3: [Batch2("canonical", [(a,) for a in inv_el], (1,))],
    }


def check_raw2(op, batch, i, o):
    p = P.Q_MOD
    r = batch.rows[i]
    K = batch.K
    o = [int(v) for v in o]
    c0, c1 = val(o[:9]), val(o[9:18])
    assert _normalised(o[:9]) and _normalised(o[9:18]), "limbs not below 2^29"
    F2 = lambda a: P.Fq2(a[0] % p, a[1] % p)
    red = lambda x: P.Fq2(x.a % p, x.b % p)
    if op == 0:
        (a0, a1), (b0, b1) = r
        assert (c0 * R261 - (a0 * b0 - a1 * b1)) % p == 0 and (c1 * R261 - (a0 * b1 + a1 * b0)) % p == 0, "congruence"
        assert c0 < 2 * p and c1 * 169 < (2 * K[0] * K[1] + 169) * p, "bounds"
    elif op == 1:
        ((a0, a1),) = r
        assert (c0 * R261 - (a0 * a0 - a1 * a1)) % p == 0 and (c1 * R261 - 2 * a0 * a1) % p == 0, "congruence"
        assert c0 * 169 < (2 * K[0] * (K[0] + 8) + 169) * p and c1 * 169 < (2 * K[0] * K[0] + 169) * p, "bounds"
    elif op == 2:
        a, b, c, d = (F2(x) for x in r)
        want = red(a * b - c * d)
        assert (c0 * R261 - want.a) % p == 0 and (c1 * R261 - want.b) % p == 0, "congruence"
        assert c0 * 100 < 106 * p and c1 * 100 < 106 * p, "value above 1.06 p"
    elif op == 3:
        a = F2(r[0])
        if a.is_zero():
            assert c0 == 0 and c1 == 0
        else:
            prod = red(a * P.Fq2(c0 % p, c1 % p))                           # a = x 2^261, out = x^-1 2^261: the product is 2^522
            assert prod.a == (R261 * R261) % p and prod.b == 0, "a * inv(a) != 1"
            assert c0 * 169 < (2 + 169) * p and c1 * 169 < (2 * 17 + 169) * p, "bounds"


# ---------------------------------------------------------------------------------------------------------------------------------------
# runners: one call per batch; out is (n, 18) uint32
# ---------------------------------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(U32P)


def mulc_constants(H, fd, batch):
    """FpConst of every row's w by make_const on the host (fp29.h: table construction), checked against floor(w 2^261 / p)"""
    p = MODS[fd]
    wl = np.array([limbs(w) for w in batch.w], dtype=np.uint32)
    z = np.zeros_like(wl)
    kc = np.zeros((len(batch), 18), dtype=np.uint32)
    out = np.zeros((len(batch), RAW_OUT), dtype=np.uint32)
    H.ht_raw_ops(fd, 0, OPS["make_const"], _p(wl), _p(z), _p(z), _p(z), _p(kc), None, _p(out), C.c_size_t(len(batch)))
    for w, row in zip(batch.w, out):
        assert [int(v) for v in row[9:]] == limbs((w << 261) // p) and [int(v) for v in row[:9]] == limbs(w)
    batch.kc = np.ascontiguousarray(out)
    return batch.kc


def host_raw(H, fd, checked, prim, b):
    out = np.full((len(b), RAW_OUT), 0xA5A5A5A5, dtype=np.uint32)
    bnd = b.bnd.ctypes.data_as(C.POINTER(C.c_double))
    H.ht_raw_ops(fd, checked, OPS[prim], _p(b.arr[0]), _p(b.arr[1]), _p(b.arr[2]), _p(b.arr[3]), _p(b.kc), bnd, _p(out), C.c_size_t(len(b)))
    return out


def dev_raw(D, fd, prim, b):
    out = np.full((len(b), RAW_OUT), 0xA5A5A5A5, dtype=np.uint32)
    st = D.dp_raw_ops(fd, OPS[prim], _p(b.arr[0]), _p(b.arr[1]), _p(b.arr[2]), _p(b.arr[3]), _p(b.kc), _p(out), C.c_size_t(len(b)))
    assert st == 0, f"HIP status {st}"
    return out


def host_raw2(H, checked, op, b):
    out = np.full((len(b), RAW_OUT), 0xA5A5A5A5, dtype=np.uint32)
    bnd = b.bnd.ctypes.data_as(C.POINTER(C.c_double))
    H.ht_raw2_ops(checked, op, _p(b.arr[0]), _p(b.arr[1]), _p(b.arr[2]), _p(b.arr[3]), bnd, _p(out), C.c_size_t(len(b)))
    return out


def dev_raw2(D, op, b):
    out = np.full((len(b), RAW_OUT), 0xA5A5A5A5, dtype=np.uint32)
    st = D.dp_raw2_ops(op, _p(b.arr[0]), _p(b.arr[1]), _p(b.arr[2]), _p(b.arr[3]), _p(out), C.c_size_t(len(b)))
    assert st == 0, f"HIP status {st}"
    return out


def check_batch(fd, prim, b, out):
    for i in range(len(b)):
        try:
            check_raw(fd, prim, b, i, out[i])
        except AssertionError as e:
            raise AssertionError(f"{prim} field {fd} class '{b.name}' row {i}: {e}; operands {[[hex(v) for v in o] for o in b.rows[i]]}, "
                                 f"out {[hex(int(v)) for v in out[i]]}") from None


def check_batch2(op, b, out):
    for i in range(len(b)):
        try:
            check_raw2(op, b, i, out[i])
        except AssertionError as e:
            raise AssertionError(f"Fq2 op {op} class '{b.name}' row {i}: {e}; operands {b.rows[i]}, out {[hex(int(v)) for v in out[i]]}") from None


# ---------------------------------------------------------------------------------------------------------------------------------------
# curves: points in the ABI form, XYZZ with a chosen Z (X = x z^2, Y = y z^3, ZZ = z^2, ZZZ = z^3)
# ---------------------------------------------------------------------------------------------------------------------------------------
CURVE_OPS = {"double_affine": 0, "double_xyzz": 1, "add_mixed": 2, "add_mixed_pos": 3, "add_mixed_neg": 4, "add_xyzz": 5, "add_xyzz_stream": 6,
             "double_xyzz_stream": 7, "neg_xyzz": 8, "to_affine": 9}


def _fe(cur, x):
    """field element -> ABI words (uint64 limbs as in helpers.pt_to_np)"""
    p = cur.p
    if cur.ext:
        return P.limbs(P.to_mont(x.a % p, p)) + P.limbs(P.to_mont(x.b % p, p))
    return P.limbs(P.to_mont(x % p, p))


def xyzz_np(cur, pt, z):
    """the point as X | Y | ZZ | ZZZ with denominator z (z = 1: the affine point itself); None -> zeros, the identity"""
    W = 8 if cur.ext else 4
    if pt is None:
        return np.zeros(4 * W, dtype=np.uint64)
    p = cur.p
    if cur.ext:
        zz = z * z
        zzz = zz * z
        return np.array(_fe(cur, pt[0] * zz) + _fe(cur, pt[1] * zzz) + _fe(cur, zz) + _fe(cur, zzz), dtype=np.uint64)
    zz, zzz = z * z % p, z * z * z % p
    return np.array(_fe(cur, pt[0] * zz) + _fe(cur, pt[1] * zzz) + _fe(cur, zz) + _fe(cur, zzz), dtype=np.uint64)


def curve_points(cur, seed=5):
    rnd = random.Random(seed)
    if cur.ext:
        return [cur.mul(cur.gen, rnd.randrange(1, cur.n)) for _ in range(4)]
    return [P.base_at(cur, P.SEED_BASE + 100, i) for i in range(4)]


def rand_z(cur, rnd):
    if cur.ext:
        return P.Fq2(rnd.randrange(1, cur.p), rnd.randrange(cur.p))
    return rnd.randrange(1, cur.p)


def one_z(cur):
    return P.Fq2(1, 0) if cur.ext else 1


def group_cases(cur):
    """(A, B) operand pairs: the list of _check_point_formulas plus 2A + (-A)"""
    A, B = curve_points(cur)[:2]
    nA = cur.neg(A)
    return [("A+B", A, B), ("A+A", A, A), ("A+(-A)", A, nA), ("O+A", None, A), ("A+O", A, None), ("O+O", None, None), ("2A+(-A)", cur.add(A, A), nA),
            ("B+A", B, A), ("(-A)+(-A)", nA, nA), ("(A+B)+(-B)", cur.add(A, B), cur.neg(B))]


def curve_case_arrays(cur, opname):
    """p, q arrays and the expected affine results of one formula over the group cases, each with z = 1 and random z on either side"""
    rnd = random.Random(77)
    ps, qs, want, names = [], [], [], []
    affine_q = opname in ("double_affine", "add_mixed", "add_mixed_pos", "add_mixed_neg")
    for name, A, B in group_cases(cur):
        for za, zb in ((one_z(cur), one_z(cur)), (rand_z(cur, rnd), one_z(cur)), (rand_z(cur, rnd), rand_z(cur, rnd))):
            if affine_q:
                if B is None:
                    continue                                                # an affine operand is never the identity (curve.h)
                zb = one_z(cur)
            if opname == "double_xyzz_stream" and A is None:
                continue                                                    # its callers filter the identity
            ps.append(xyzz_np(cur, A, za)); qs.append(xyzz_np(cur, B, zb)); names.append(name)
            want.append({"double_affine": lambda: cur.add(B, B), "double_xyzz": lambda: cur.add(A, A), "double_xyzz_stream": lambda: cur.add(A, A),
                         "add_mixed": lambda: cur.add(A, B), "add_mixed_pos": lambda: cur.add(A, B), "add_mixed_neg": lambda: cur.add(A, cur.neg(B)),
                         "add_xyzz": lambda: cur.add(A, B), "add_xyzz_stream": lambda: cur.add(A, B), "neg_xyzz": lambda: cur.neg(A),
                         "to_affine": lambda: A}[opname]())
    return np.stack(ps), np.stack(qs), want, names


COOP_ITEMS, COOP_QUADS = 48, 16


def coop_kind(cur, A, B, active):
    if not active:
        return "inactive"
    if A is None or B is None:
        return "copy"
    if A == B:
        return "doubling"
    if A == cur.neg(B):
        return "cancelling"
    return "ordinary"


def coop_waves(cur):
    """items (nwg * 48, 4W), params (nwg * 16, 5), the expected affine point of every item, the kinds of every wave's quads.
    Quad t owns items 3t, 3t + 1, 3t + 2; the result goes to 3t + 2, or in place to 3t / 3t + 1."""
    rnd = random.Random(4242)
    cases = group_cases(cur)
    A, B = curve_points(cur)[:2]
    C_, D_ = curve_points(cur)[2:4]
    ordinary = [("A+B", A, B), ("B+A", B, A), ("C+D", C_, D_), ("A+C", A, C_), ("2A+(-A)", cur.add(A, A), cur.neg(A)), ("D+B", D_, B)]
    exceptional = [c for c in cases if coop_kind(cur, c[1], c[2], True) != "ordinary"]
    waves = []
    k = 0
    for wv in range(3):                                                     # mixed waves: the cases dealt round-robin
        quads = []
        for t in range(COOP_QUADS):
            name, a, b = cases[k % len(cases)]
            quads.append((a, b, (k // len(cases) + t) % 3, 0 if (t % 8 == 7) else 1, (k + wv) % 4))
            k += 1
        waves.append(quads)
    waves.append([(ordinary[t % len(ordinary)][1], ordinary[t % len(ordinary)][2], t % 3, 1, t % 4) for t in range(COOP_QUADS)])
    waves.append([(exceptional[t % len(exceptional)][1], exceptional[t % len(exceptional)][2], t % 3, 1, t % 4) for t in range(COOP_QUADS)])
    items, params, want, kinds = [], [], [], []
    for quads in waves:
        kd = []
        for t, (a, b, where, active, dbl) in enumerate(quads):
            spare = curve_points(cur)[(t + 1) % 4]
            ia, ib = 3 * t, 3 * t + 1
            io = (3 * t + 2, ia, ib)[where]
            pts = [a, b, spare]
            za, zb, zs = ((one_z(cur) if rnd.random() < 0.3 else rand_z(cur, rnd)) for _ in range(3))
            items += [xyzz_np(cur, a, za), xyzz_np(cur, b, zb), xyzz_np(cur, spare, zs)]
            params.append([ia, ib, io, active, dbl])
            res = list(pts)
            r = cur.add(a, b) if active else pts[io - 3 * t]
            res[io - 3 * t] = cur.mul(r, 1 << dbl) if r is not None else None
            want += res
            kd.append(coop_kind(cur, a, b, active))
        kinds.append(kd)
    return np.stack(items), np.array(params, dtype=np.uint32), want, kinds


# ---------------------------------------------------------------------------------------------------------------------------------------
# digits
# ---------------------------------------------------------------------------------------------------------------------------------------
def glv_module():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("glv_consts", os.path.join(root, "tools", "gen", "glv_consts.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


def lattice_g(fd):
    """G_1, G_2 of csrc/glv_consts.h for scalar field fd, read as integers from the header (the rounding boundaries are theirs)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "kogarashi_amd", "csrc", "glv_consts.h")).read()
    blk = txt.split("GlvLattice<%s>" % ("FrParams" if fd == 0 else "FqParams"))[1]
    out = []
    for nm in ("G1", "G2"):
        ws = re.search(nm + r"\[\d\] = \{([^}]*)\}", blk).group(1)
        out.append(sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(ws.split(","))))
    return out


def glv_edge_scalars(fd, n, lam, count_random=2000):
    """(edge scalars, rounding-boundary scalars, random scalars) for the lattice of scalar field fd"""
    edges = [0, 1, 2, n - 1, n - 2, n // 2, n // 3, lam, lam + 1, lam - 1, n - lam, lam * lam % n]
    for e in (126, 127, 128):
        edges += [(1 << e) - 1, 1 << e, (1 << e) + 1]
    edges += [1 << 253, n - 3]
    bound = []
    for g in lattice_g(fd):
        last = (g * (n - 1) + (1 << 255)) >> 256                            # the largest c_i a scalar below n reaches
        for j in (0, 1, 2, 12345, last - 1):
            k = -((-(2 * j + 1) << 255) // g)                               # ceil((2 j + 1) 2^255 / G_i): the first k whose c_i is j + 1
            bound += [x for x in (k - 1, k, k + 1) if 0 <= x < n]
    rnd = random.Random(900 + fd)
    return edges, bound, [rnd.randrange(n) for _ in range(count_random)]


def kwords(ks):
    return np.array([[(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for k in ks], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# helpers both test modules use: calls into the host library, ABI-form operands of the inversions, the GLV checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def host_field_ops(H, field, checked, op, a, b):
    o = np.empty_like(a)
    H.ht_field_ops(field, checked, op, p32(a.view(np.uint32)), p32(b.view(np.uint32)), p32(o.view(np.uint32)), C.c_size_t(a.shape[0]))
    return o


def inversion_operands(O, fd, n, seed=0x4B6F676172617368):
    """ABI-form elements: every special value of the field, then oracle-seeded ones up to n rows (fd 2: Fq2, both coordinates)"""
    p = MODS[1 if fd == 2 else fd]
    sp = [L(P.to_mont(v, p)) for v in canon(p)]
    if fd == 2:
        a = np.concatenate([O.gen_scalars(1, seed + 31, 0, n), O.gen_scalars(1, seed + 32, 0, n)], axis=1)
        m = len(sp)
        a[:m, :4], a[:m, 4:] = sp, sp[::-1]
        a[m:2 * m, :4], a[m:2 * m, 4:] = sp, 0
        a[2 * m:3 * m, :4], a[2 * m:3 * m, 4:] = 0, sp
        return a
    a = O.gen_scalars(fd, seed + 30, 0, n)
    a[:len(sp)] = sp
    return a


def inversion_expected(fd, a):
    p = MODS[1 if fd == 2 else fd]
    rows = []
    for r in a:
        if fd == 2:
            x = P.Fq2(P.from_mont(I(r[:4]), p), P.from_mont(I(r[4:]), p))
            y = x.inv() if not x.is_zero() else x
            rows.append(np.concatenate([L(P.to_mont(y.a % p, p)), L(P.to_mont(y.b % p, p))]))
        else:
            x = P.from_mont(I(r), p)
            rows.append(L(P.to_mont(pow(x, -1, p), p)) if x else np.zeros(4, dtype=np.uint64))
    return np.stack(rows)


def host_curve_ops(H, cid, chk, op, p, q):
    o = np.zeros((p.shape[0], p.shape[1] // 2), dtype=np.uint64)
    inf = np.zeros(p.shape[0], dtype=np.uint8)
    H.ht_curve_ops(cid, chk, op, p32(p.view(np.uint32)), p32(q.view(np.uint32)), p32(o.view(np.uint32)), inf.ctypes.data_as(U8P), C.c_size_t(p.shape[0]))
    return o, inf


def host_coop_ops(H, cid, chk, items, params):
    n = items.shape[0]
    o = np.zeros((n, items.shape[1] // 2), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    r = H.ht_coop_ops(cid, chk, p32(items.view(np.uint32)), p32(params), C.c_size_t(n // COOP_ITEMS), p32(o.view(np.uint32)), inf.ctypes.data_as(U8P))
    assert r == 0
    return o, inf


def assert_coop_waves_are_mixed(kinds):
    """every wave but the last two holds ordinary, copy, doubling and cancelling quads together; then one all-ordinary, one all-exceptional"""
    for kd in kinds[:-2]:
        assert all(kd.count(k) >= 1 for k in ("ordinary", "copy", "doubling", "cancelling", "inactive")), kd
    assert set(kinds[-2]) == {"ordinary"} and "ordinary" not in kinds[-1] and len(set(kinds[-1])) == 3


def glv_decompose(lib_call, fd, ks):
    kw = kwords(ks)
    k1 = np.zeros((len(ks), 4), dtype=np.uint32); k2 = np.zeros_like(k1); neg = np.zeros((len(ks), 2), dtype=np.uint8)
    lib_call(fd, p32(kw), C.c_size_t(len(ks)), p32(k1), p32(k2), neg.ctypes.data_as(U8P))
    return k1, k2, neg


def check_glv_halves(ks, k1, k2, neg, lam, n):
    val4 = lambda w: sum(int(w[j]) << (32 * j) for j in range(4))
    for i, k in enumerate(ks):
        a, b = val4(k1[i]), val4(k2[i])
        assert a < 3 << 125 and b < 3 << 125, hex(k)
        assert ((-a if neg[i, 0] else a) + (-b if neg[i, 1] else b) * lam - k) % n == 0, hex(k)


def check_glv_digits(ks, dig, W, c, lam, n):
    for k, row in zip(ks, dig):
        h1 = sum(int(row[0][w]) << (w * c) for w in range(W))
        h2 = sum(int(row[1][w]) << (w * c) for w in range(W))
        assert (h1 + h2 * lam - k) % n == 0, hex(k)
        assert all(abs(int(row[e][w])) <= 1 << (c - 1) for e in range(2) for w in range(W)), hex(k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Fp2S<Fq>, the lane-pair Fq2 of csrc/fp2s.h (device only): element i on lanes 2i (c0) and 2i + 1 (c1)
#
# operand table of dp_fp2s_raw_ops (Batch2 rows, 18 raw limbs per operand):
#   mul         raw2_batches()[0] (canonical specials and the a0 b0 = a1 b1 (+-1) relations, non-canonical, K 9) + the half classes below
#   sqr         raw2_batches()[1]: canonical, K 6, non-canonical (5.4) -- fp2s.h asks for normalised limbs and K <= 6, the SAME class fp29.h
#               states for the one-lane square, so nothing of that table had to be left out; + the half classes below
#   mul2sub     raw2_batches()[2] + rows of the half classes
#   is_zero     every pairing of {0, p, 2p, 3p, 167p} and non-multiples on the two halves (K 168)
#   is_zero_2p  every pairing of {0, p} and values of [0, 2p) that differ from 0 / p in one bit of one limb
#   one         Fp2S::one() on every lane pair of two waves
# half classes: exactly one half zero, both zero, one half equal to p or to 2p (zero as a value, not as limbs)
# ---------------------------------------------------------------------------------------------------------------------------------------
FP2S_OPS = {"mul": 0, "sqr": 1, "mul2sub": 2, "is_zero": 3, "is_zero_2p": 4, "one": 5}
Q = P.Q_MOD
R261_INV_Q = pow(R261, -1, Q)


def fp2s_half_elements():
    rnd = random.Random(2929)
    nz = [1, Q - 1, (Q + 1) // 2] + [rnd.randrange(1, Q) for _ in range(3)]
    el = [(0, 0)] + [(0, x) for x in nz] + [(x, 0) for x in nz]
    el += [(Q, x) for x in nz[:3]] + [(x, Q) for x in nz[:3]] + [(2 * Q, x) for x in nz[:3]] + [(x, 2 * Q) for x in nz[:3]]
    el += [(Q, 0), (0, Q), (Q, Q), (2 * Q, Q), (Q, 2 * Q), (2 * Q, 2 * Q), (2 * Q, 0), (0, 2 * Q)]
    return el


def fp2s_batches():
    rnd = random.Random(2930)
    B2 = raw2_batches()
    H = fp2s_half_elements()
    full = [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(6)]
    others = H + full
    hp = [(H[i], others[(i * 7 + s) % len(others)]) for s in (0, 1, 5) for i in range(len(H))] + [(f, h) for f in full[:2] for h in H]
    hq = [(H[i], others[(i * 3 + 1) % len(others)], others[(i * 5 + 2) % len(others)], H[(i + 4) % len(H)]) for i in range(len(H))]
    hq += [(a, b, a, b) for a, b in hp[:12]] + [(a, b, b, a) for a, b in hp[:12]]
    mult, nonm = [0, Q, 2 * Q, 3 * Q, 167 * Q], [1, Q - 1, Q + 1, 2 * Q - 1, 2 * Q + 1, 167 * Q + 1, rnd.randrange(1, Q)]
    z_all = [((a, b),) for a in mult + nonm for b in mult + nonm]
    pl = limbs(Q)
    flip = [val(pl[:i] + [pl[i] ^ (1 << b)] + pl[i + 1:]) for i in range(9) for b in (0, 28 if i < 8 else 21)]
    flip = [x for x in flip if x < 2 * Q] + [1 << (29 * i) for i in range(9)]
    z2, n2 = [0, Q], [1, Q - 1, Q + 1, 2 * Q - 1] + flip
    z2_all = [((a, b),) for a in z2 for b in z2] * 4 + [((a, b),) for a in z2 for b in n2] + [((b, a),) for a in z2 for b in n2]
    z2_all += [((n2[i], n2[(i + 3) % len(n2)]),) for i in range(len(n2))]
    return {
        "mul": B2[0] + [Batch2("one half zero / p / 2p", hp, ("5.4", "5.4"))],
        "sqr": B2[1] + [Batch2("one half zero / p / 2p (K <= 6, normalised: the class fp2s.h states)", [(h,) for h in H], ("5.4",))],
        "mul2sub": B2[2] + [Batch2("one half zero / p / 2p", hq, ("5.4",) * 4)],
        "is_zero": [Batch2("multiples of p and their neighbours on either half", z_all, (168,))],
        "is_zero_2p": [Batch2("[0, 2p): 0, p and one-bit neighbours on either half", z2_all, (2,))],
        "one": [Batch2("no operand", [((0, 0),)] * 70, (1,))],
    }


def check_fp2s(prim, batch, i, o):
    """the lane pair's 18 output words against Python integers: the congruence of both halves, normalised limbs, and the bound fp29.h documents
    for the primitive that PRODUCES each half (mul2pm: [0, 2p); mul: (Ka Kb / 169 + 1) p; vred: 1.06 p).  Verdicts: both lanes, equal and right."""
    r, K = batch.rows[i], batch.K
    o = [int(v) for v in o]
    if prim in ("is_zero", "is_zero_2p"):
        ((a0, a1),) = r
        want = 1 if (a0 % Q == 0 and a1 % Q == 0) else 0
        assert o[0] == o[9], "the two lanes of the pair disagree"
        assert o[0] == want and not any(o[1:9]) and not any(o[10:]), "verdict"
        return
    if prim == "one":
        assert o[:9] == limbs(R261 % Q) and not any(o[9:]), "one() is (1, 0) in the internal form"
        return
    c0, c1 = val(o[:9]), val(o[9:18])
    assert _normalised(o[:9]) and _normalised(o[9:18]), "limbs not below 2^29"
    if prim == "mul":
        (a0, a1), (b0, b1) = r
        assert (c0 * R261 - (a0 * b0 - a1 * b1)) % Q == 0, "congruence of c0"
        assert (c1 * R261 - (a0 * b1 + a1 * b0)) % Q == 0, "congruence of c1"
        assert c0 < 2 * Q and c1 < 2 * Q, "mul2pm: [0, 2p)"
    elif prim == "sqr":
        ((a0, a1),) = r
        assert (c0 * R261 - (a0 * a0 - a1 * a1)) % Q == 0, "congruence of c0"
        assert (c1 * R261 - 2 * a0 * a1) % Q == 0, "congruence of c1"
        assert c0 * 169 < (2 * K[0] * (K[0] + 8) + 169) * Q and c1 * 169 < (2 * K[0] * K[0] + 169) * Q, "bounds"
    elif prim == "mul2sub":
        a, b, c, d = (P.Fq2(x[0], x[1]) for x in r)
        want = a * b - c * d
        assert (c0 * R261 - want.a) % Q == 0, "congruence of c0"
        assert (c1 * R261 - want.b) % Q == 0, "congruence of c1"
        assert c0 * 100 < 106 * Q and c1 * 100 < 106 * Q, "value above 1.06 p"
    else:
        raise KeyError(prim)


def fp2s_expected(prim, batch, i):
    """one output the checker accepts (canonical halves): what the self-test mutates"""
    r = batch.rows[i]
    if prim in ("is_zero", "is_zero_2p"):
        f = 1 if (r[0][0] % Q == 0 and r[0][1] % Q == 0) else 0
        return [f] + [0] * 8 + [f] + [0] * 8
    if prim == "one":
        return limbs(R261 % Q) + [0] * 9
    e = [P.Fq2(x[0], x[1]) for x in r]
    v = {"mul": lambda: e[0] * e[1], "sqr": lambda: e[0] * e[0], "mul2sub": lambda: e[0] * e[1] - e[2] * e[3]}[prim]()
    return limbs(v.a * R261_INV_Q % Q) + limbs(v.b * R261_INV_Q % Q)


def check_fp2s_batch(prim, b, out):
    for i in range(len(b)):
        try:
            check_fp2s(prim, b, i, out[i])
        except AssertionError as e:
            raise AssertionError(f"Fp2S {prim} class '{b.name}' row {i}: {e}; operands {b.rows[i]}, out {[hex(int(v)) for v in out[i]]}") from None


def dev_fp2s(D, prim, b):
    out = np.full((len(b), RAW_OUT), 0xA5A5A5A5, dtype=np.uint32)
    st = D.dp_fp2s_raw_ops(FP2S_OPS[prim], _p(b.arr[0]), _p(b.arr[1]), _p(b.arr[2]), _p(b.arr[3]), _p(out), C.c_size_t(len(b)))
    assert st == 0, f"HIP status {st}"
    return out


def canonical_halves(out):
    return [(val(r[:9]) % Q, val(r[9:18]) % Q) for r in out]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stream formulas on XYZZ<Fp2S<Fq>> through the reduction's accessors (dp_fp2s_curve_ops).  A point is 72 raw limbs in the order of the
# one-lane PointAoS<Fp2<Fq>>: x.c0 x.c1 y.c0 y.c1 zz.c0 zz.c1 zzz.c0 zzz.c1; a limb vector holds value * 2^261 mod p.  The reference is the
# XYZZ formulas themselves (add-2008-s, dbl-2008-s-1) over pyoracle.Fq2 integers: every coordinate must agree, not only the affine point.
# ---------------------------------------------------------------------------------------------------------------------------------------
S_ROUTES = {"AosSrc -> AosDst": 0, "AosSrc -> SoaDst": 1, "SoaSrc -> SoaDst": 2}
S_ACTIVE, S_P_EMPTY, S_Q_EMPTY = 1, 2, 4
S_PAIRS = 32                                                                # lane pairs of a wave = of a workgroup of the probe
S_KINDS = ("ordinary", "doubling", "cancelling", "O+A", "A+O", "O+O", "P=(0,x)", "P=(x,0)", "P=0 R=(0,x)", "P=0 R=(x,0)", "ZZ half zero")
F2_ZERO, F2_ONE = P.Fq2(0, 0), P.Fq2(1, 0)
O4 = (F2_ZERO,) * 4


def f2_raw(x):
    return limbs(x.a * R261 % Q) + limbs(x.b * R261 % Q)


def pt_raw(pt):
    return [w for x in pt for w in f2_raw(x)]


def raw_f2(w):
    return P.Fq2(val(w[:9]) * R261_INV_Q, val(w[9:18]) * R261_INV_Q)


def raw_pt(w):
    return tuple(raw_f2(w[18 * k:18 * k + 18]) for k in range(4))


def xyzz_dbl_ref(p):
    x, y, zz, zzz = p
    u = y * 2
    v = u * u
    w = u * v
    s = x * v
    m = x * x * 3
    x3 = m * m - s * 2
    return (x3, m * (s - x3) - w * y, v * zz, w * zzz)


def xyzz_add_ref(p, q):
    """(result, branch): 'copy q', 'copy p', 'doubling', 'identity' or 'generic'"""
    if p[2].is_zero():
        return q, "copy q"
    if q[2].is_zero():
        return p, "copy p"
    u1, u2, s1, s2 = p[0] * q[2], q[0] * p[2], p[1] * q[3], q[1] * p[3]
    pp_, r = u2 - u1, s2 - s1
    pp = pp_ * pp_
    if pp.is_zero():
        return (xyzz_dbl_ref(p), "doubling") if r.is_zero() else (O4, "identity")
    ppp = pp_ * pp
    qq = u1 * pp
    x3 = r * r - ppp - qq * 2
    return (x3, r * (qq - x3) - s1 * ppp, p[2] * q[2] * pp, p[3] * q[3] * ppp), "generic"


def _half(x):
    return None if x.is_zero() else ("(0,x)" if x.a == 0 else ("(x,0)" if x.b == 0 else None))


def s_kind(p, q):
    """the kind of an addition from the operands' VALUES"""
    zp, zq = p[2].is_zero(), q[2].is_zero()
    if zp or zq:
        return "O+O" if zp and zq else ("O+A" if zp else "A+O")
    pp_, r = q[0] * p[2] - p[0] * q[2], q[1] * p[3] - p[1] * q[3]
    if pp_.is_zero():
        if r.is_zero():
            return "doubling"
        return "P=0 R=" + _half(r) if _half(r) else "cancelling"
    if _half(pp_):
        return "P=" + _half(pp_)
    if _half(p[2]) or _half(q[2]):
        return "ZZ half zero"
    return "ordinary"


def _abi_f2(w):
    return P.Fq2(P.from_mont(I(w[:4]), Q), P.from_mont(I(w[4:8]), Q))


def _patch_p(raw, coord, half):
    """the same value with a zero half written as the limbs of p (the _2p form of zero)"""
    o = 18 * coord + 9 * half
    assert not any(raw[o:o + 9])
    return raw[:o] + limbs(Q) + raw[o + 9:]


def fp2s_curve_cases():
    """[(name, p raw, q raw, flags)] of the additions, before they are dealt into waves: the group cases of curve_case_arrays(P.G2, ...) and the
    half-zero operand sets (field values, not curve points)"""
    rnd = random.Random(7117)
    rf = lambda: P.Fq2(rnd.randrange(1, Q), rnd.randrange(1, Q))
    cases = []
    ps, qs, _, names = curve_case_arrays(P.G2, "add_xyzz_stream")
    for name, pr, qr in zip(names, ps, qs):
        pt, qt = (tuple(_abi_f2(r[8 * k:8 * k + 8]) for k in range(4)) for r in (pr, qr))
        cases.append((name, pt_raw(pt), pt_raw(qt), 0))
    A = curve_points(P.G2)[0]
    a1 = (A[0], A[1], F2_ONE, F2_ONE)
    cases += [("empty+A", [0xDEAD] * 72, pt_raw(a1), S_P_EMPTY), ("A+empty", pt_raw(a1), [0xBEEF] * 72, S_Q_EMPTY),
              ("empty+empty", [0xDEAD] * 72, [0xBEEF] * 72, S_P_EMPTY | S_Q_EMPTY)]
    for rep in range(2):
        for d in (P.Fq2(0, rnd.randrange(1, Q)), P.Fq2(rnd.randrange(1, Q), 0), P.Fq2(0, 1), P.Fq2(Q - 1, 0)):
            x1, y1, y2 = rf(), rf(), rf()
            cases.append(("P half zero, z = 1", pt_raw((x1, y1, F2_ONE, F2_ONE)), pt_raw((x1 + d, y2, F2_ONE, F2_ONE)), 0))
            zz1, zzz1, zz2, zzz2 = rf(), rf(), rf(), rf()
            cases.append(("P half zero, any z", pt_raw((x1, y1, zz1, zzz1)), pt_raw(((x1 * zz2 + d) * zz1.inv(), y2, zz2, zzz2)), 0))
            # the full-zero difference: R = d (half zero) must give the identity; R = 0 under unrelated denominators is a doubling
            cases.append(("P = 0, R half zero, z = 1", pt_raw((x1, y1, F2_ONE, F2_ONE)), pt_raw((x1, y1 + d, F2_ONE, F2_ONE)), 0))
            cases.append(("P = 0, R half zero, any z", pt_raw((x1, y1, zz1, zzz1)),
                          pt_raw((x1 * zz2 * zz1.inv(), (y1 * zzz2 + d) * zzz1.inv(), zz2, zzz2)), 0))
            cases.append(("P = 0, R = 0, any z", pt_raw((x1, y1, zz1, zzz1)), pt_raw((x1 * zz2 * zz1.inv(), y1 * zzz2 * zzz1.inv(), zz2, zzz2)), 0))
        for hz in (P.Fq2(0, rnd.randrange(1, Q)), P.Fq2(rnd.randrange(1, Q), 0)):
            half = 0 if hz.a == 0 else 1
            full = (rf(), rf(), rf(), rf())
            one_side = (rf(), rf(), hz, rf())
            cases.append(("ZZ1 half zero", pt_raw(one_side), pt_raw(full), 0))
            cases.append(("ZZ2 half zero", pt_raw(full), pt_raw(one_side), 0))
            cases.append(("ZZ1, ZZ2 half zero", pt_raw(one_side), pt_raw((rf(), rf(), hz, rf())), 0))
            cases.append(("ZZ1 half p", _patch_p(pt_raw(one_side), 2, half), pt_raw(full), 0))
            cases.append(("ZZ2 half p", pt_raw(full), _patch_p(pt_raw(one_side), 2, half), 0))
    # zero as limbs of p on one or both halves of ZZ: the identity
    ident = pt_raw((rf(), rf(), F2_ZERO, rf()))
    full = pt_raw((rf(), rf(), rf(), rf()))
    for halves in ((0,), (1,), (0, 1)):
        z = ident
        for h in halves:
            z = _patch_p(z, 2, h)
        cases += [("ZZ1 = 0 as p", z, full, 0), ("ZZ2 = 0 as p", full, z, 0), ("ZZ1 = ZZ2 = 0 as p", z, ident, 0)]
    return cases


def fp2s_curve_waves():
    """The additions dealt into waves of 32 lane pairs: full waves in which every kind of S_KINDS is present, one wave whose LAST pair alone is
    active, and a partial last workgroup.  Returns p, q (n, 72) uint32, flags (n,) uint8, kinds [n] (None: idle), names [n]."""
    cases = fp2s_curve_cases()
    by = {k: [] for k in S_KINDS}
    for c in cases:
        by[s_kind(*_case_values(c))].append(c)
    assert all(by[k] for k in S_KINDS), {k: len(v) for k, v in by.items()}
    order, used = [], {k: 0 for k in S_KINDS}
    tail = 11                                                               # pairs of the partial last workgroup
    while not all(used[k] >= len(by[k]) for k in S_KINDS) or len(order) % S_PAIRS:
        k = S_KINDS[len(order) % len(S_KINDS)]
        order.append(by[k][used[k] % len(by[k])])
        used[k] += 1
    lone = [by["P=(0,x)"][0]] * S_PAIRS
    rows = [(c, S_ACTIVE) for c in order] + [(c, S_ACTIVE if i == S_PAIRS - 1 else 0) for i, c in enumerate(lone)]
    rows += [(by[S_KINDS[i % len(S_KINDS)]][-1], S_ACTIVE) for i in range(tail)]
    p = np.array([c[1] for c, _ in rows], dtype=np.uint32)
    q = np.array([c[2] for c, _ in rows], dtype=np.uint32)
    flags = np.array([c[3] | a for c, a in rows], dtype=np.uint8)
    kinds = [s_kind(*_case_values(c)) if a else None for c, a in rows]
    return p, q, flags, kinds, [c[0] for c, _ in rows]


def fp2s_double_waves():
    """the first operands of fp2s_curve_waves for double_xyzz_stream (never the identity: its callers filter it), every fourth one replaced by a
    point with one half of X or of Y zero"""
    rnd = random.Random(7118)
    rf = lambda: P.Fq2(rnd.randrange(1, Q), rnd.randrange(1, Q))
    p, q, flags0, _, _ = fp2s_curve_waves()
    p, flags = p.copy(), flags0 & S_ACTIVE
    extra = [pt_raw((rf(), P.Fq2(0, rnd.randrange(1, Q)), rf(), rf())), pt_raw((rf(), P.Fq2(rnd.randrange(1, Q), 0), rf(), rf())),
             pt_raw((P.Fq2(0, rnd.randrange(1, Q)), rf(), rf(), rf())), pt_raw((P.Fq2(rnd.randrange(1, Q), 0), rf(), rf(), F2_ONE))]
    for i in range(len(p)):
        if i % 4 == 3 or flags0[i] & S_P_EMPTY or raw_pt(p[i])[2].is_zero():
            p[i] = extra[(i // 4) % 4]
    return p, q, flags


def _case_values(c):
    _, pr, qr, fl = c
    return (O4 if fl & S_P_EMPTY else raw_pt(pr)), (O4 if fl & S_Q_EMPTY else raw_pt(qr))


def assert_fp2s_waves_are_mixed(kinds, flags):
    """every full wave but the lone one holds every kind at once; the lone wave's last pair is its only active one; the last workgroup is partial"""
    n = len(kinds)
    nfull = n // S_PAIRS
    assert n % S_PAIRS != 0 and nfull >= 3
    lone = [w for w in range(nfull) if sum(1 for k in kinds[w * S_PAIRS:(w + 1) * S_PAIRS] if k) == 1]
    assert len(lone) == 1 and kinds[lone[0] * S_PAIRS + S_PAIRS - 1] is not None
    for w in range(nfull):
        if w not in lone:
            kd = kinds[w * S_PAIRS:(w + 1) * S_PAIRS]
            assert all(k in kd for k in S_KINDS), (w, kd)
    assert all(k for k in kinds[nfull * S_PAIRS:])
    assert all(bool(f & S_ACTIVE) == (k is not None) for f, k in zip(flags, kinds))


FILL = 0xA5A5A5A5


def fp2s_curve_expected(op, pr, qr, fl):
    """(kind of check, value): ('bits', 72 words) where the formula copies or writes zeros, ('value', 4 Fq2, computed X/Y?) where it computes"""
    p = O4 if fl & S_P_EMPTY else raw_pt(pr)
    q = O4 if fl & S_Q_EMPTY else raw_pt(qr)
    img = lambda raw, empty: [0] * 72 if empty else [int(v) for v in raw]
    if op == "copy":
        return "bits", img(pr, fl & S_P_EMPTY)
    if op == "double":
        return "value", xyzz_dbl_ref(p)
    res, branch = xyzz_add_ref(p, q)
    if branch == "copy q":
        return "bits", img(qr, fl & S_Q_EMPTY)
    if branch == "copy p":
        return "bits", img(pr, fl & S_P_EMPTY)
    if branch == "identity":
        return "bits", [0] * 72                                             # curve.h: every path that produces the identity writes zeros
    return "value", res


def check_fp2s_curve(op, pr, qr, fl, out):
    """one active pair's 72 output words"""
    how, want = fp2s_curve_expected(op, pr, qr, fl)
    out = [int(v) for v in out]
    if how == "bits":
        assert out == want, "a copied operand / the identity, bit for bit"
        return
    assert all(v <= M29 for v in out), "limbs not below 2^29"
    got = raw_pt(out)
    for k, nm in enumerate(("X", "Y", "ZZ", "ZZZ")):
        assert got[k] == want[k], f"{nm} differs from the formula over Fq2 integers"
        for h in (0, 1):
            v = val(out[18 * k + 9 * h:18 * k + 9 * h + 9])
            assert (v * 100 < 106 * Q) if k < 2 else (v < 2 * Q), f"{nm} half {h}: above the bound curve.h keeps for a stored coordinate"


def fp2s_curve_good_output(op, pr, qr, fl):
    """an output the checker accepts: what the self-test mutates"""
    how, want = fp2s_curve_expected(op, pr, qr, fl)
    return list(want) if how == "bits" else pt_raw(want)


def dev_fp2s_curve(D, op, route, inplace, p, q, flags):
    """runs the probe; SoA operands are transposed here.  Returns out (n, 72) in the array-of-structures order whatever the route"""
    n = p.shape[0]
    soa_in, soa_out = route == 2, route in (1, 2)
    if soa_in:                                                              # a structure-of-arrays source has no empty flag: the identity is zeros
        p, q = p.copy(), q.copy()
        p[(flags & S_P_EMPTY) != 0] = 0
        q[(flags & S_Q_EMPTY) != 0] = 0
    pa = np.ascontiguousarray(p.T) if soa_in else p
    qa = np.ascontiguousarray(q.T) if soa_in else q
    out = np.full((72, n) if soa_out else (n, 72), FILL, dtype=np.uint32)
    st = D.dp_fp2s_curve_ops({"add": 0, "double": 1, "copy": 2}[op], route, int(inplace), _p(pa), _p(qa), flags.ctypes.data_as(U8P), _p(out), C.c_size_t(n))
    assert st == 0, f"HIP status {st}"
    return np.ascontiguousarray(out.T) if soa_out else out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the probe library
# ---------------------------------------------------------------------------------------------------------------------------------------
DEV_EXPORTS = ["dp_raw_ops", "dp_raw2_ops", "dp_field_ops", "dp_curve_ops", "dp_coop_ops", "dp_small_digits", "dp_glv_decompose", "dp_glv_digits",
               "dp_endo", "dp_fp2s_raw_ops", "dp_fp2s_curve_ops",
               # the sort and task kernels of the long MSM, one at a time (tests/device/devprobe_sort.h, tests/sort_cases.py)
               "dp_sort_prep", "dp_sort_onepass", "dp_sort_zero_fill", "dp_sort_group_scan", "dp_sort_merge_groups", "dp_sort_group_scatter_big",
               "dp_sort_fine_local", "dp_sort_fine_scatter", "dp_task_bucket_tables", "dp_task_bases", "dp_task_len_scatter", "dp_level_ops",
               # the point-side kernels of the long MSM, one at a time (tests/device/devprobe_reduce.h, tests/reduce_cases.py)
               "dp_bases_prep", "dp_bases_table_next", "dp_acc_tasks", "dp_gather", "dp_sum_tasks", "dp_halve", "dp_reduce_tail", "dp_hot"]
