"""References, layout coders, case builders and checkers for the point-side kernels of the long MSM (csrc/msm_bases.h, msm_acc_kernels.h,
msm_reduce_kernels.h), which tests/device/devprobe_reduce.h launches one at a time (tests/test_gpu_reduce_kernels.py).

Pure numpy and Python integers, importable without a GPU (tests/test_reduce_cases_host.py runs the census of the cases, composes the references
into a whole MSM and feeds every checker mutated outputs).

  points    every point a case uses is a known multiple m * G of the curve's generator: the pool of tests/long_edge_cases.py (a dozen m_i * G
            and their negatives) and sums of those.  A reference works on the multipliers alone (integers modulo the group order, 0 = the
            identity), so the expected content of an output slot is ONE scalar multiplication, (sum of +-m_i mod n) * G, made with pyoracle.
  operands  a partial sum or bucket item is written as XYZZ = (x z^2, y z^3, z^2, z^3) with a chosen z (1, or one of three fixed random
            values); the identity is all-zero words.  A coordinate is in the internal form, value * 2^261 mod p as nine normalised limbs.
  outputs   every coordinate is reduced mod p; the point is the identity iff zz = 0, otherwise zz^3 = zzz^2 must hold and (x / zz, y / zzz)
            must be the expected affine point.  Exact: no tolerance anywhere.

Every table a kernel READS is built here, so each kernel is judged alone.  Output buffers are sort_cases.OBuf: FILL in the owned words and a
guard region behind them; every checker asserts the guard, that the words the kernel must not write still hold FILL (or the input), and
that every word it must write was written."""
import functools
import random

import numpy as np

import long_edge_cases as LE
import sort_cases as SC
from helpers import CURVES
from oracle import pyoracle as P
from primitive_cases import R261, limbs, val
from sort_cases import FILL, GATHER_SUM_MAX, OBuf, check_guards, excl, u32

REDUCE_EXPORTS = ["dp_bases_prep", "dp_bases_table_next", "dp_acc_tasks", "dp_gather", "dp_sum_tasks", "dp_halve", "dp_reduce_tail", "dp_hot"]
NAMES = ("g1", "gk", "g2")                        # the probe's curve number = the index
KEEP = None                                       # expected content of a slot the kernel must leave alone
NZ = 4                                            # denominators an operand is written with: z = 1 and three random ones


# ---------------------------------------------------------------------------------------------------------------------------------------------
# curves, coders
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Pt(int):
    """a multiplier that brings its affine point along (made by adding affine points: cheaper than a scalar multiplication per slot where a
    case has hundreds of different sums)"""

    def __new__(cls, m, pt):
        o = int.__new__(cls, m)
        o.pt = pt
        return o


class Cv:
    """one curve: its constants in the kernels (words per point, lanes per task, tail length), its pool and the coders of a point"""

    def __init__(self, name):
        self.name, self.id, self.cur = name, CURVES[name][0], CURVES[name][1]
        self.p, self.n, self.ext = self.cur.p, self.cur.n, self.cur.ext
        self.NE = 2 if self.ext else 1                       # base-field elements per coordinate
        self.NW, self.E64, self.LPT = 36 * self.NE, 4 * self.NE, self.NE
        self.TL = 128 if self.ext else 256                   # TailCfg<KF>::L
        self.NT = 256 // self.LPT                            # task lanes of a 256-thread workgroup = hot_split_max
        self.split_max = self.NT
        self.r261_inv, self.r256_inv = pow(R261, -1, self.p), pow(1 << 256, -1, self.p)
        pl = LE.pool(name)
        self.pool = [m for m, _ in pl]                       # POOL multipliers, then their negatives
        self._aff = {0: None}
        self._aff.update({m: pt for m, pt in pl})
        rnd = random.Random(0x7A11 + self.id)
        self.zs = [self.one()] + [self.el([rnd.randrange(1, self.p) for _ in range(self.NE)]) for _ in range(NZ - 1)]
        self._enc = {}

    # field elements: Python integers, or pyoracle.Fq2
    def el(self, c):
        return P.Fq2(c[0], c[1]) if self.ext else c[0] % self.p

    def comps(self, x):
        return (x.a, x.b) if self.ext else (x % self.p,)

    def one(self):
        return self.el([1, 0])

    def is_zero(self, x):
        return x.is_zero() if self.ext else x % self.p == 0

    def inv(self, x):
        return x.inv() if self.ext else pow(x, -1, self.p)

    def eq(self, x, y):
        return self.is_zero(x - y)

    def aff(self, m):
        """m * G as an affine pyoracle point (None: the identity)"""
        if isinstance(m, Pt):
            return m.pt
        m %= self.n
        if m not in self._aff:
            self._aff[m] = self.cur.mul(self.cur.gen, m)
        return self._aff[m]

    def xyzz(self, m, zi):
        """the four coordinates of m * G over the denominator zs[zi]; the identity: four zeros"""
        pt = self.aff(m)
        if pt is None:
            z = self.el([0, 0])
            return (z, z, z, z)
        z = self.zs[zi]
        zz = z * z
        zzz = zz * z
        return (pt[0] * zz, pt[1] * zzz, zz, zzz)

    # -- the internal form: value * 2^261 mod p, nine limbs per base-field element, x | y | zz | zzz (Fq2: c0 then c1 of each)
    def raw(self, coords):
        return np.array([w for x in coords for c in self.comps(x) for w in limbs(c * R261 % self.p)], dtype=np.uint32)

    def unraw(self, w):
        v = [val(w[9 * k:9 * k + 9]) * self.r261_inv % self.p for k in range(4 * self.NE)]
        return tuple(self.el(v[self.NE * k:self.NE * k + self.NE]) for k in range(4))

    def enc(self, m, zi=0):
        """NW words of the operand m * G written over zs[zi] (cached: a case is thousands of look-ups of a few dozen operands)"""
        if isinstance(m, Pt):
            return self.raw(self.xyzz(m, zi))
        key = (m % self.n, zi)
        if key not in self._enc:
            self._enc[key] = self.raw(self.xyzz(m, zi))
        return self._enc[key]

    # -- the exported form: value * 2^256 mod p, four 64-bit words per base-field element, x | y | zz | zzz
    def abi(self, coords):
        return np.array([(c * (1 << 256) % self.p >> (64 * j)) & (2**64 - 1) for x in coords for c in self.comps(x) for j in range(4)], dtype=np.uint64)

    def unabi(self, w):
        v = [sum(int(w[4 * k + j]) << (64 * j) for j in range(4)) * self.r256_inv % self.p for k in range(4 * self.NE)]
        return tuple(self.el(v[self.NE * k:self.NE * k + self.NE]) for k in range(4))

    def affine(self, coords):
        """XYZZ -> affine point or None; refuses a point whose zz and zzz do not belong together"""
        x, y, zz, zzz = coords
        if self.is_zero(zz):
            return None
        assert self.eq(zz * zz * zz, zzz * zzz), "zz^3 != zzz^2"
        return (x * self.inv(zz), y * self.inv(zzz))

    def same_point(self, a, b):
        if a is None or b is None:
            return a is None and b is None
        return self.eq(a[0], b[0]) and self.eq(a[1], b[1])


@functools.lru_cache(maxsize=None)
def cv(name):
    return Cv(name)


def aos(c, ms, zis=None):
    """(N, NW) words: point i = ms[i] * G over zs[zis[i]] -- the PointAoS layout when flattened"""
    zis = [0] * len(ms) if zis is None else zis
    return np.stack([c.enc(m, z) for m, z in zip(ms, zis)]) if len(ms) else np.zeros((0, c.NW), dtype=np.uint32)


def to_soa(rows, stride=None):
    """PointIO: word k of item i at [k * stride + i]"""
    n, nw = rows.shape
    stride = n if stride is None else stride
    out = np.full((nw, stride), FILL, dtype=np.uint32)
    out[:, :n] = rows.T
    return out.reshape(-1)


def from_soa(flat, nw, stride):
    """(stride, nw) rows, a VIEW of the buffer: row i = the words of item i"""
    return np.asarray(flat).reshape(nw, stride).T


def check_rows(c, rows, want, what, decode=None, before=None):
    """rows[i] holds want[i] * G (any denominator), or is untouched where want[i] is KEEP: still FILL, or still `before[i]`"""
    decode = c.unraw if decode is None else decode
    assert len(rows) == len(want), f"{what}: {len(rows)} slots against {len(want)} expected"
    for i, m in enumerate(want):
        r = rows[i]
        if m is KEEP:
            still = (r == FILL).all() if before is None else np.array_equal(r, before[i])
            assert still, f"{what}: slot {i} must stay as it was and was written"
            continue
        assert not (r == FILL).any(), f"{what}: slot {i} was not (fully) written"
        try:
            got = c.affine(decode(r))
        except AssertionError as e:
            raise AssertionError(f"{what}: slot {i}: {e}") from None
        assert c.same_point(got, c.aff(m)), f"{what}: slot {i} holds another point than the expected multiple of G"


class Level:
    """cnt [W][B] -> the round's tables: rel = exclusive prefix inside the window, base = first task of each window, base[W] = total"""

    def __init__(self, cnt):
        self.cnt = np.asarray(cnt, dtype=np.int64)
        self.W, self.B = self.cnt.shape
        self.rel = excl(self.cnt, axis=1)
        tot = self.cnt.sum(axis=1)
        self.base = np.concatenate([excl(tot), [int(tot.sum())]])
        self.total = int(tot.sum())

    def first(self, w, b):
        return int(self.base[w] + self.rel[w, b])

    def bufs(self):
        return [u32(self.cnt), u32(self.rel), u32(self.base)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references on multipliers (lists of integers mod n; 0 = the identity), written from the comments of the headers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_gather_buckets(part, L):
    return [part[L.first(w, b)] if L.cnt[w, b] else 0 for w in range(L.W) for b in range(L.B)]


def ref_gather_sum(part, L, n):
    """a bucket's partial sums added up; above GATHER_SUM_MAX the total already sits in the first one's place"""
    out = []
    for w in range(L.W):
        for b in range(L.B):
            k = int(L.cnt[w, b])
            k = 1 if k > GATHER_SUM_MAX else k
            out.append(sum(part[L.first(w, b):L.first(w, b) + k]) % n)
    return out


def ref_halve(items, W, narr, n_out, n):
    """W x narr arrays of 2 n_out items -> W x (narr + 1) arrays of n_out: array a = pair sums, the new array narr = the odd items of array 0"""
    out = [0] * (W * (narr + 1) * n_out)
    for w in range(W):
        for a in range(narr):
            for i in range(n_out):
                s = (w * narr + a) * 2 * n_out + 2 * i
                out[(w * (narr + 1) + a) * n_out + i] = (items[s] + items[s + 1]) % n
                if a == 0:
                    out[(w * (narr + 1) + narr) * n_out + i] = items[s + 1]
    return out


def ref_gather_halve(part, L, n):
    return ref_halve(ref_gather_buckets(part, L), L.W, 1, L.B // 2, n)


def ref_sum_tasks(part, Lin, T2, n):
    """(the new level, its partial sums): a bucket's previous partial sums in runs of T2"""
    L = Level((Lin.cnt + T2 - 1) // T2)
    out = [0] * L.total
    for w in range(L.W):
        for b in range(L.B):
            f, k = Lin.first(w, b), int(Lin.cnt[w, b])
            for seg in range(int(L.cnt[w, b])):
                out[L.first(w, b) + seg] = sum(part[f + seg * T2:f + min((seg + 1) * T2, k)]) % n
    return L, out


def ref_tail(items, W, narr, ln, n):
    """the slot of W * c sums, c = narr + log2(ln): array a < narr summed up; narr - 1 + j: the items of array 0 whose index has bit j - 1 set"""
    steps = ln.bit_length() - 1
    c = narr + steps
    out = [0] * (W * c)
    for w in range(W):
        for a in range(narr):
            out[w * c + a] = sum(items[(w * narr + a) * ln:(w * narr + a + 1) * ln]) % n
        for j in range(1, steps + 1):
            out[w * c + narr - 1 + j] = sum(items[w * narr * ln + i] for i in range(ln) if (i >> (j - 1)) & 1) % n
    return out


def ref_hot_sum(part, L, hot_list, split, n):
    """scratch point i * split + y: the y-th share of ceil(cnt / split) partial sums of hot bucket i (the identity for a share that is empty)"""
    out = []
    for t in hot_list:
        w, b = divmod(int(t), L.B)
        f, k = L.first(w, b), int(L.cnt[w, b])
        share = (k + split - 1) // split
        out += [sum(part[f + min(y * share, k):f + min((y + 1) * share, k)]) % n for y in range(split)]
    return out


def ref_hot_fold(part, L, hot_list, scratch, split, n):
    out = list(part)
    for i, t in enumerate(hot_list):
        w, b = divmod(int(t), L.B)
        out[L.first(w, b)] = sum(scratch[i * split:(i + 1) * split]) % n
    return out


def window_value(slot_w, n):
    """A + sum_l 2^l T_l of one window's c sums = sum_b (b + 1) bucket_b"""
    return (slot_w[0] + sum(t << l for l, t in enumerate(slot_w[1:]))) % n


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operand patterns
# ---------------------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("equal", "alternating", "identities", "random")


def pattern(c, kind, count, seed):
    """(multipliers, denominators) of `count` items.  equal: one point over varying denominators (every pair doubles); alternating: P, -P
    (every pair cancels; sums of pairs are identities); identities: empty items on one or both sides of a pair; random: six pool points"""
    rnd = random.Random(seed)
    m0, pl = c.pool[0], c.pool
    if kind == "equal":
        ms = [m0] * count
    elif kind == "alternating":
        ms = [m0 if i % 2 == 0 else c.n - m0 for i in range(count)]
    elif kind == "identities":
        cyc = [0, m0, pl[1], 0, 0, 0, pl[2], pl[3]]
        ms = [cyc[i % 8] for i in range(count)]
    else:
        six = [pl[0], pl[1], pl[2], c.n - pl[0], c.n - pl[1], pl[3]]
        ms = [rnd.choice(six) for _ in range(count)]
    return ms, [rnd.randrange(NZ) for _ in range(count)]


def node_kind(a, b, n):
    if a == 0 and b == 0:
        return "both empty"
    if a == 0:
        return "empty + P"
    if b == 0:
        return "P + empty"
    if a == b:
        return "doubling"
    return "cancelling" if (a + b) % n == 0 else "ordinary"


NODE_KINDS = ("both empty", "empty + P", "P + empty", "doubling", "cancelling", "ordinary")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases.  A case holds its inputs as arrays, `args()` = (entry, buffers, parameters) with fresh output buffers, `outputs` names the OBufs
# among them, `check(out)` judges them and `model()` returns outputs the checker accepts (what the self-test mutates).
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    entry = None

    def fresh(self):
        """{name: OBuf}"""
        raise NotImplementedError

    def call_args(self, out):
        raise NotImplementedError

    def expected(self):
        """{name: (want list, rows-of-buffer function, decoder or None, before rows or None)}"""
        raise NotImplementedError

    def check(self, out):
        what = f"{self.entry} {self.name}"
        check_guards(out, what)
        for k, (want, rows, decode, before) in self.expected().items():
            check_rows(self.c, rows(out[k].own), want, f"{what}: {k}", decode, before)

    def model(self):
        """outputs the checker accepts: every expected point over a random denominator, every other word as it was"""
        out = self.fresh()
        for k, (want, rows, decode, before) in self.expected().items():
            self.write_model(out[k], k, want)
        return out

    def write_model(self, buf, k, want):
        raise NotImplementedError


def _rows_aos(nw):
    return lambda own: own.reshape(-1, nw)


def _put_aos(buf, c, want, zi=1):
    r = buf.own.reshape(-1, c.NW)
    for i, m in enumerate(want):
        if m is not KEEP:
            r[i] = c.enc(m, zi if m % c.n else 0)


def _put_soa(buf, c, want, stride, zi=1):
    r = buf.own.reshape(c.NW, stride)
    for i, m in enumerate(want):
        if m is not KEEP:
            r[:, i] = c.enc(m, zi if m % c.n else 0)


class GatherCase(Case):
    """which: 0 k_gather_buckets, 1 k_gather_halve, 2 k_gather_sum.  part holds the buckets' partial sums where the level says, and points
    no bucket owns between them (SPARE in front of every window's run and behind the last), which no output may depend on"""
    entry = "dp_gather"
    SPARE = 3

    def __init__(self, name, which, W, B, cnt, seed, kinds="random"):
        self.c, self.which, self.W, self.B, self.npts = cv(name), which, W, B, W * B
        c = self.c
        self.name = f"{name} {('buckets', 'halve', 'sum')[which]} W{W} B{B} {kinds}"
        m0, m1, rnd = c.pool[0], c.pool[1], random.Random(seed)
        node = None
        if kinds == "nodes":                                                   # the level-1 nodes (buckets 2i, 2i + 1) of every kind, in turn
            pairs = [(0, 0), (0, m0), (m0, 0), (m0, m0), (m0, c.n - m0), (m0, m1)]
            node = np.array([[pairs[(i // 2 + w) % 6][i % 2] for i in range(B)] for w in range(W)], dtype=object)
            cnt = (node != 0).astype(np.int64)
        self.L = Level(np.asarray(cnt).reshape(W, B))
        self.L.base = self.L.base + self.SPARE * np.arange(1, W + 2)          # gaps the tables do not name: base is what the kernel must follow
        self.cap = int(self.L.base[W])
        six = [m0, m1, c.pool[2], c.n - m0, c.n - m1, c.pool[3]]
        self.part = [rnd.choice(six) for _ in range(self.cap)]
        for w in range(W):
            for b in range(B):
                f, k = self.L.first(w, b), int(self.L.cnt[w, b])
                if node is not None and k:
                    self.part[f] = int(node[w, b])
                elif kinds == "equal":
                    self.part[f:f + k] = [m0] * k
                elif kinds == "alternating":
                    self.part[f:f + k] = [m0 if j % 2 == 0 else c.n - m0 for j in range(k)]
        self.zis = [rnd.randrange(NZ) for _ in range(self.cap)]
        self.pin = aos(c, self.part, self.zis)
        ref = (lambda: ref_gather_buckets(self.part, self.L), lambda: ref_gather_halve(self.part, self.L, c.n), lambda: ref_gather_sum(self.part, self.L, c.n))
        self.want = ref[which]()

    def fresh(self):
        return {"out": OBuf(self.npts * self.c.NW)}

    def call_args(self, out):
        return [self.pin] + self.L.bufs() + [out["out"]], [self.c.id, self.which, self.W, self.B, self.cap]

    def expected(self):
        return {"out": (self.want, lambda own: from_soa(own, self.c.NW, self.npts), None, None)}

    def write_model(self, buf, k, want):
        _put_soa(buf, self.c, want, self.npts)

    def nodes(self):
        bk = ref_gather_buckets(self.part, self.L)
        return [node_kind(bk[w * self.B + 2 * i], bk[w * self.B + 2 * i + 1], self.c.n) for w in range(self.W) for i in range(self.B // 2)]


GATHER_SUM_CNTS = [0, 1, 2, 31, 32, 33, 100]


def gather_cases():
    out = []
    for name in NAMES:
        c = cv(name)
        for j, B in enumerate((2, 64, 512)):
            cnt = np.random.RandomState(40 + j).randint(0, 2, (3, B))
            cnt[0, 0], cnt[1, :], cnt[2, B - 1] = 0, [1] + [0] * (B - 2) + [1], 1          # an empty first bucket; a window of two buckets at its ends
            out.append(GatherCase(name, 0, 3, B, cnt, 50 + j))
        for j, B in enumerate((2 * c.TL, 4 * c.TL)):
            out.append(GatherCase(name, 1, 2, B, np.ones((2, B)), 60 + j, "nodes"))
        for kinds in ("random", "equal", "alternating"):
            cnt = np.array([GATHER_SUM_CNTS, GATHER_SUM_CNTS[::-1], [33, 0, 32, 1, 100, 2, 31]])
            out.append(GatherCase(name, 2, 3, 7, cnt, 70, kinds))
    return out


class SumTasksCase(Case):
    """k_sum_tasks: the previous round's partial sums of every bucket in runs of T2; launched over `bound` = the previous round's task count"""
    entry = "dp_sum_tasks"

    def __init__(self, name, T2, seed, kinds="random"):
        self.c, self.T2 = cv(name), T2
        c = self.c
        self.name = f"{name} T2={T2} {kinds}"
        sizes = [T2 - 1, T2, T2 + 1, 2 * T2, 0]
        self.Lin = Level(np.array([sizes, sizes[::-1], [0, 2 * T2 + 1, 0, 1, 3 * T2]]))
        self.W, self.B = self.Lin.W, self.Lin.B
        self.bound = self.Lin.total
        ms, self.zis = pattern(c, kinds, self.bound, seed)
        self.part = ms
        self.pin = aos(c, ms, self.zis)
        self.L, self.sums = ref_sum_tasks(ms, self.Lin, T2, c.n)
        assert self.L.total < self.bound
        self.want = self.sums + [KEEP] * (self.bound - self.L.total)          # surplus threads write nothing

    def fresh(self):
        return {"pout": OBuf(self.bound * self.c.NW)}

    def call_args(self, out):
        return ([self.pin] + self.Lin.bufs() + self.L.bufs() + [out["pout"]],
                [self.c.id, self.W, self.B, self.T2, self.bound, self.bound, self.bound])

    def expected(self):
        return {"pout": (self.want, _rows_aos(self.c.NW), None, None)}

    def write_model(self, buf, k, want):
        _put_aos(buf, self.c, want)


def sum_tasks_cases():
    return [SumTasksCase(name, T2, 80 + T2, kinds) for name in NAMES for T2 in (2, 16) for kinds in ("random", "equal", "alternating")]


class HalveCase(Case):
    entry = "dp_halve"
    W = 3

    def __init__(self, name, narr, n_out, kinds, seed):
        self.c, self.narr, self.n_out = cv(name), narr, n_out
        c = self.c
        self.name = f"{name} narr{narr} n_out{n_out} {kinds}"
        self.n_in, self.n_o = self.W * narr * 2 * n_out, self.W * (narr + 1) * n_out
        self.items, self.zis = pattern(c, kinds, self.n_in, seed)
        self.inp = to_soa(aos(c, self.items, self.zis))
        self.want = ref_halve(self.items, self.W, narr, n_out, c.n)

    def fresh(self):
        return {"out": OBuf(self.n_o * self.c.NW)}

    def call_args(self, out):
        return [self.inp, out["out"]], [self.c.id, self.W, self.narr, self.n_out, self.n_in, self.n_o]

    def expected(self):
        return {"out": (self.want, lambda own: from_soa(own, self.c.NW, self.n_o), None, None)}

    def write_model(self, buf, k, want):
        _put_soa(buf, self.c, want, self.n_o)

    def nodes(self):
        return [node_kind(self.items[2 * i], self.items[2 * i + 1], self.c.n) for i in range(self.n_in // 2)]


def halve_cases():
    out = []
    for name in NAMES:
        c = cv(name)
        k = 0
        for narr in (1, 2, 3):
            for n_out in (1, 2, 64, c.TL):
                out.append(HalveCase(name, narr, n_out, PATTERNS[k % 4], 90 + k))      # every pattern at every narr and at three of the four lengths
                k += 1
        out += [HalveCase(name, 2, 64, kinds, 99) for kinds in PATTERNS]
    return out


TAIL_FORMS = ("fixed", "runtime", "coop")


class TailCase(Case):
    """form 0: k_reduce_tail<.., TL>; 1: k_reduce_tail<.., 0>; 2: k_reduce_tail_coop.  c = narr + log2(len): the slot holds exactly W * c points"""
    entry = "dp_reduce_tail"
    W = 3

    def __init__(self, name, form, narr, ln, kinds, seed):
        self.c, self.form, self.narr, self.ln = cv(name), form, narr, ln
        c = self.c
        self.name = f"{name} {TAIL_FORMS[form]} narr{narr} len{ln} {kinds}"
        self.wc = narr + ln.bit_length() - 1
        self.n_in = self.W * narr * ln
        self.items, self.zis = pattern(c, kinds, self.n_in, seed)
        self.inp = to_soa(aos(c, self.items, self.zis))
        self.want = ref_tail(self.items, self.W, narr, ln, c.n)
        self.pw = 4 * c.E64                                                    # 64-bit words per exported point

    def fresh(self):
        return {"out": OBuf(self.W * self.wc * self.pw, dtype=np.uint64)}

    def call_args(self, out):
        return [self.inp, out["out"]], [self.c.id, self.form, self.W, self.narr, self.ln, self.wc, self.n_in]

    def expected(self):
        return {"out": (self.want, lambda own: own.reshape(-1, self.pw), self.c.unabi, None)}

    def write_model(self, buf, k, want):
        r = buf.own.reshape(-1, self.pw)
        for i, m in enumerate(want):
            r[i] = self.c.abi(self.c.xyzz(m, 1))


def tail_cases():
    out = []
    for name in NAMES:
        c = cv(name)
        k = 0
        for narr in (1, 2, 3):
            out.append(TailCase(name, 0, narr, c.TL, PATTERNS[k % 4], 110 + k))
            k += 1
        out.append(TailCase(name, 0, 2, c.TL, "equal", 113))
        out.append(TailCase(name, 0, 1, c.TL, "random", 114))
        for ln in (2, 4, 8, c.TL // 4, c.TL // 2):
            out.append(TailCase(name, 1, 1, ln, PATTERNS[k % 4], 120 + k))
            k += 1
        out.append(TailCase(name, 1, 1, c.TL // 2, "equal", 126))
        for narr in (1, 3):
            for ln in (2, 4, c.TL // 2, c.TL):
                out.append(TailCase(name, 2, narr, ln, PATTERNS[k % 4], 130 + k))
                k += 1
        out.append(TailCase(name, 2, 3, c.TL, "equal", 139))
    return out


class HotCase(Case):
    """hot buckets of (cnt, ...) partial sums in a level of W = 3 windows of B = 4 buckets, listed out of bucket order, between buckets that
    are not hot.  which 0: k_hot_sum (scratch out, SLACK untouched slots behind nhot * split); 1: k_hot_fold (part in place, reading a
    reference scratch)"""
    entry = "dp_hot"
    W, B, SLACK = 3, 4, 5

    def __init__(self, name, which, cnts, split, kinds, seed):
        self.c, self.which, self.split, self.cnts = cv(name), which, split, list(cnts)
        c = self.c
        self.name = f"{name} {('sum', 'fold')[which]} cnt{'+'.join(str(v) for v in cnts)} split{split} {kinds}"
        rs = np.random.RandomState(seed)
        cnt = rs.randint(0, 4, (self.W, self.B))
        where = [(2, 1), (0, 3), (1, 0)][:len(cnts)]                           # different windows, not in bucket order
        for (w, b), k in zip(where, cnts):
            cnt[w, b] = k
        self.L = Level(cnt)
        self.hot_list = [w * self.B + b for w, b in where]
        self.cap = self.L.total
        self.part, self.zis = pattern(c, kinds, self.cap, seed)
        self.pin = aos(c, self.part, self.zis)
        self.nsl = len(cnts) * split
        self.scr = ref_hot_sum(self.part, self.L, self.hot_list, split, c.n)
        if which == 0:
            self.want = self.scr + [KEEP] * self.SLACK
        else:
            rnd = random.Random(seed)
            self.scr_in = aos(c, self.scr, [rnd.randrange(NZ) for _ in self.scr])
            tot = ref_hot_fold(self.part, self.L, self.hot_list, self.scr, split, c.n)
            firsts = {self.L.first(w, b) for w, b in where}
            self.want = [tot[i] if i in firsts else KEEP for i in range(self.cap)]

    def fresh(self):
        if self.which == 0:
            return {"scratch": OBuf((self.nsl + self.SLACK) * self.c.NW)}
        return {"part": OBuf(self.cap * self.c.NW, init=self.pin)}

    def call_args(self, out):
        p = [self.c.id, self.which, self.B, len(self.cnts), self.split, self.W, self.cap]
        if self.which == 0:
            return [self.pin] + self.L.bufs() + [u32(self.hot_list), out["scratch"]], p
        return [out["part"]] + self.L.bufs() + [u32(self.hot_list), self.scr_in], p

    def expected(self):
        if self.which == 0:
            return {"scratch": (self.want, _rows_aos(self.c.NW), None, None)}
        return {"part": (self.want, _rows_aos(self.c.NW), None, self.pin)}

    def write_model(self, buf, k, want):
        _put_aos(buf, self.c, want)

    def empty_shares(self):
        return sum(1 for k in self.cnts for y in range(self.split) if y * ((k + self.split - 1) // self.split) >= k)


def hot_shapes(c):
    """(cnts of the hot buckets, split)"""
    sm = c.split_max
    return [([33], 16), ([47, 33, 48], 16), ([48], 16), ([49, 40, 34], 16), ([40], 17), ([300, 33, 101], 100), ([40], sm), ([2 * sm + 1, 40, sm], sm),
            ([16 * c.NT + 16], 16)]


def hot_cases():
    out = []
    for name in NAMES:
        c = cv(name)
        for j, (cnts, split) in enumerate(hot_shapes(c)):
            kinds = PATTERNS[j % 4] if cnts[0] < 1000 else "random"
            out.append(HotCase(name, 0, cnts, split, kinds, 150 + j))
            out.append(HotCase(name, 1, cnts, split, kinds, 170 + j))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the bases: the ABI form, the two resident forms (msm_bases.h), k_prep_bases and k_table_next
# ---------------------------------------------------------------------------------------------------------------------------------------------
INF_BIT = 0x80000000
BASES_72, BASES_64, BASES_ABI = 0, 1, 2
FMT_NAMES = ("limb form", "64-byte form", "ABI array")


def from_ref_val(p, w):
    """what from_ref makes of the reference value w = x * 2^256 mod p: the Montgomery product w * (2^266 mod p) / 2^261 without a final
    subtraction -- congruent to x * 2^261, below 2p, not always below p (fp29.h)"""
    cst = (1 << 266) % p
    m = w * cst * (-pow(p, -1, R261)) % R261
    return (w * cst + m * p) >> 261


def abi_point(c, pt):
    """x | y of a pair of field elements (not necessarily on the curve): four 64-bit words per base-field element, value * 2^256 mod p"""
    return np.array([((v << 256) % c.p >> (64 * j)) & (2**64 - 1) for x in pt for v in c.comps(x) for j in range(4)], dtype=np.uint64)


def internal_vals(c, pt, canonical=False):
    """the 2 * NE internal values of x | y: canonical (value * 2^261 mod p), or as from_ref leaves them"""
    return [v * R261 % c.p if canonical else from_ref_val(c.p, (v << 256) % c.p) for x in pt for v in c.comps(x)]


def pack_resident(vals, inf, fmt):
    """limb form: nine limbs per value, INF_BIT in word 8; 64-byte form: the eight 32-bit words of each value, INF_BIT in word 7"""
    if fmt == BASES_64:
        w = [(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(8)]
        w[7] |= INF_BIT if inf else 0
    else:
        w = [x for v in vals for x in limbs(v)]
        w[8] |= INF_BIT if inf else 0
    return np.array(w, dtype=np.uint32)


def unpack_resident(c, w, fmt):
    """(internal values, flag) of one resident point"""
    w = [int(x) for x in w]
    if fmt == BASES_64:
        inf, w[7] = bool(w[7] & INF_BIT), w[7] & ~INF_BIT
        return [sum(w[8 * k + j] << (32 * j) for j in range(8)) for k in range(2 * c.NE)], inf
    inf, w[8] = bool(w[8] & INF_BIT), w[8] & ~INF_BIT
    return [val(w[9 * k:9 * k + 9]) for k in range(2 * c.NE)], inf


def resident_words(c, fmt):
    return 2 * c.NE * (8 if fmt == BASES_64 else 9) if fmt != BASES_ABI else 16


class WordsCase(Case):
    """a kernel whose output is compared word for word with the packer's"""

    def check(self, out):
        what = f"{self.entry} {self.name}"
        check_guards(out, what)
        SC.same(out["out"].own, self.want, f"{what}: resident words")

    def fresh(self):
        return {"out": OBuf(len(self.want))}

    def model(self):
        out = self.fresh()
        out["out"].own[:] = self.want
        return out


class PrepCase(WordsCase):
    """k_prep_bases: coordinates 0, 1, p - 1, the special points of acc_abi_cases, pool points; flagged points carry arbitrary coordinates"""
    entry = "dp_bases_prep"

    def __init__(self, name, n, fmt, with_inf):
        import acc_abi_cases
        self.c, self.n, self.fmt = cv(name), n, fmt
        c = self.c
        self.name = f"{name} n{n} {FMT_NAMES[fmt]}{' flags' if with_inf else ''}"
        e = lambda a, b=0: c.el([a, b])
        pts = [(e(0), e(1)), (e(1, c.p - 1), e(c.p - 1, 1)), (e(c.p - 1), e(0, c.p - 1)), (e(c.p - 1, c.p - 1), e(c.p - 1, c.p - 1))]
        if not c.ext:
            pts += [pt for _, pt in acc_abi_cases.special_points(name)]
        pool = [c.aff(m) for m in c.pool]
        self.pts = [(pts + pool)[i % (len(pts) + len(pool))] for i in range(n)]
        self.inf = None
        if with_inf:
            self.inf = np.zeros(n, dtype=np.uint8)
            self.inf[[0, n // 2, n - 1]] = [1, 7, 255]
        self.bases = np.concatenate([abi_point(c, pt) for pt in self.pts])
        self.want = np.concatenate([pack_resident(internal_vals(c, pt), with_inf and self.inf[i], fmt) for i, pt in enumerate(self.pts)])

    def call_args(self, out):
        return [self.bases, self.inf, out["out"]], [self.c.id, self.n, self.fmt]


def prep_cases():
    return [PrepCase(name, n, fmt, inf) for name in NAMES for fmt in (BASES_72, BASES_64) for n, inf in ((1, True), (255, False), (256, True), (257, True), (257, False))]


class TableCase(WordsCase):
    """k_table_next: the packer applied to 2^c * P in canonical internal values; a flagged point goes through as zeros with the flag"""
    entry = "dp_bases_table_next"

    def __init__(self, name, cw, n, fmt):
        self.c, self.cw, self.n, self.fmt = cv(name), cw, n, fmt
        c = self.c
        self.name = f"{name} c{cw} n{n} {FMT_NAMES[fmt]}"
        self.ms = [c.pool[(i * 7) % len(c.pool)] for i in range(n)]
        self.inf = [i % 9 == 4 or (n > 2 and i == n - 1) for i in range(n)]
        garbage = (c.el([3, 5]), c.el([c.p - 2, 1]))
        self.prev = np.concatenate([pack_resident(internal_vals(c, garbage if f else c.aff(m)), f, fmt) for m, f in zip(self.ms, self.inf)])
        zero = [0] * (2 * c.NE)
        self.want = np.concatenate([pack_resident(zero if f else internal_vals(c, c.aff(m << cw), True), f, fmt) for m, f in zip(self.ms, self.inf)])

    def call_args(self, out):
        return [self.prev, out["out"]], [self.c.id, self.n, self.cw, self.fmt]


def table_cases():
    return [TableCase(name, cw, n, fmt) for name in NAMES for cw in (1, 2, 13) for n in (1, 63, 64, 65) for fmt in (BASES_72, BASES_64)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# k_acc_tasks
# ---------------------------------------------------------------------------------------------------------------------------------------------
ACC_T = 32
CHAINS = ("P, P", "P, -P, P", "sign first", "sign last", "flag first", "flag middle", "flag last", "below every later set", "plain")


class AccCase(Case):
    """One launch of k_acc_tasks over the tables of a sort_cases.TaskCase.  Scalar i of set k has the base bm(k, i) * G:
    the period of bm is 8 (i and i + 8: the same point, i and i + 4: opposite points), sets differ by a shift, and in the resident forms the
    scalars i = 9 mod 16 are flagged identities with arbitrary coordinates.  Non-empty buckets get, in turn, the entry chains of CHAINS at the
    start of their first task; the other entries are random.  Set k takes the entries idx >= idx_off[k]; its bases are the points of scalars
    idx_off[k] ..; every set has its own partial buffer of ntasks + SLACK slots.  merged = number of table windows (0: a plain sort)."""
    entry = "dp_acc_tasks"
    SLACK = 3

    def __init__(self, name, tc, fmts, order, seed, merged=0):
        self.c, self.tc, self.fmts, self.order, self.merged = cv(name), tc, list(fmts), order, merged
        c, n = self.c, self.c.n
        nsets = self.nsets = len(fmts)
        self.name = f"{name} {tc.name} {' + '.join(FMT_NAMES[f] for f in fmts)}{' merged' if merged else ''} order {order}"
        rnd = random.Random(seed)
        W, B = tc.Wg, tc.B
        self.rowlen = N = int(tc.bsize.sum(axis=1).max()) + 23                  # scalars = row length of the sorted lists
        self.idx_off = [0, N // 3, N // 3 + N // 4][:nsets]
        self.mshift = (N - 1).bit_length() if merged else 0
        self.tab_n = N + 3 if merged else 0
        self.nbases = [merged * self.tab_n if merged else N - o for o in self.idx_off]
        pl = c.pool

        def bm(k, i, w=0):
            m = pl[(i + 3 * k + 5 * w) % 4]
            return m if (i + 3 * k + 5 * w) % 8 < 4 else n - m
        self.bm = bm
        self.flag = lambda k, i: self.fmts[k] != BASES_ABI and i % 16 == 9
        # the sorted lists
        self.sorted = np.full((W, N), FILL, dtype=np.uint32)
        self.chain_of, o = {}, 0
        last = self.idx_off[-1]
        hi0 = max(N - 17, last + 1)
        for w in range(W):
            for b in range(B):
                v = int(tc.bsize[w, b])
                if not v:
                    continue
                ent = [(rnd.randrange(N), rnd.randrange(2), rnd.randrange(max(merged, 1))) for _ in range(v)]
                tl = min(int(tc.Tb[w, b]), v)                                   # length of the bucket's first task
                a = last + 16 * rnd.randrange(max((hi0 - last) // 16, 1)) + 2   # a = 2 mod 16 above every idx_off: a + 7 = 9 mod 16 is flagged
                a -= last % 16
                a = a if last <= a and a + 8 < N else last
                f = a + 7 if (a + 7) % 16 == 9 and a + 7 < N else a
                kind = CHAINS[o % len(CHAINS)]
                plant = {"P, P": [(a, 0), (a + 8, 0)], "P, -P, P": [(a, 0), (a + 8, 1), (a, 0)], "sign first": [(a, 1)], "flag first": [(f, 0)]}.get(kind, [])
                if len(plant) <= tl and a + 8 < N:
                    for j, (i, s) in enumerate(plant):
                        ent[j] = (i, s, ent[j][2])
                    if kind == "sign last":
                        ent[tl - 1] = (a, 1, ent[tl - 1][2])
                    if kind == "flag last":
                        ent[tl - 1] = (f, 0, ent[tl - 1][2])
                    if kind == "flag middle" and tl >= 3:
                        ent[tl // 2] = (f, 0, ent[tl // 2][2])
                    if kind == "below every later set" and nsets > 1:
                        ent = [(rnd.randrange(self.idx_off[1]), s, t) for _, s, t in ent]
                    self.chain_of[(w, b)] = kind
                o += 1
                st = int(tc.bstart[w, b])
                self.sorted[w, st:st + v] = [i | (t << self.mshift) | (s << 31) for i, s, t in ent]
        # the task lists: any order in which the keys of the task lengths never rise is one the sort may leave
        nt = tc.ntasks
        flat_nt = tc.ntask.reshape(-1)
        bkt = np.repeat(np.arange(W * B), flat_nt)
        seg = np.arange(nt) - np.repeat(excl(flat_nt), flat_nt)
        ln = np.where(seg < np.repeat(flat_nt, flat_nt) - 1, np.repeat(tc.Tb.reshape(-1), flat_nt), np.repeat(tc.rem.reshape(-1), flat_nt))
        key = SC.len_key(ln)
        perm = np.argsort(-key, kind="stable") if order == 0 else np.lexsort((-np.arange(nt), -key))
        self.task_bkt, self.task_id = bkt[perm], np.arange(nt)[perm]
        self.cap = nt + self.SLACK
        # the reference: the group sum of every task's entries of every set, by affine additions
        cur = c.cur
        self.stats = {"doubling": 0, "identity mid-chain": 0, "skipped": [0] * nsets, "all skipped": [0] * nsets, "flagged": {"first": 0, "middle": 0, "last": 0}}
        self.want = []
        for k in range(nsets):
            sums = []
            for t in range(nt):
                w, b = divmod(int(bkt[t]), B)
                lo = int(seg[t]) * int(tc.Tb[w, b])
                es = self.sorted[w, int(tc.bstart[w, b]) + lo:int(tc.bstart[w, b]) + lo + int(ln[t])]
                m, pt, used = 0, None, 0
                for j, e in enumerate(int(x) for x in es):
                    idx, tw = (e & 0x7FFFFFFF) & ((1 << self.mshift) - 1 if merged else 0x7FFFFFFF), ((e & 0x7FFFFFFF) >> self.mshift if merged else 0)
                    if idx < self.idx_off[k]:
                        self.stats["skipped"][k] += 1
                        continue
                    used += 1
                    if self.flag(k, idx):
                        self.stats["flagged"]["first" if j == 0 else "last" if j == len(es) - 1 else "middle"] += 1
                        continue
                    d = bm(k, idx, tw) if not e >> 31 else n - bm(k, idx, tw)
                    if m and m == d:
                        self.stats["doubling"] += 1
                    m = (m + d) % n
                    pt = cur.add(pt, c.aff(d))
                    if m == 0 and j < len(es) - 1:
                        self.stats["identity mid-chain"] += 1
                self.stats["all skipped"][k] += used == 0
                sums.append(Pt(m, pt))
            self.want.append(sums + [KEEP] * self.SLACK)
        # the base arrays
        self.pb = []
        cache = {}
        for k in range(nsets):
            rows = []
            for r in range(self.nbases[k]):
                tw, i = (r // self.tab_n, r % self.tab_n) if merged else (0, r + self.idx_off[k])
                fl = self.flag(k, i)
                key2 = (bm(k, i, tw), fl, fmts[k])
                if key2 not in cache:
                    pt = (c.el([1, 2]), c.el([c.p - 3, 4])) if fl else c.aff(bm(k, i, tw))
                    cache[key2] = abi_point(c, pt).view(np.uint32) if fmts[k] == BASES_ABI else pack_resident(internal_vals(c, pt), fl, fmts[k])
                rows.append(cache[key2])
            self.pb.append(np.concatenate(rows))

    def fresh(self):
        return {f"partial{k}": OBuf(self.cap * self.c.NW) for k in range(self.nsets)}

    def call_args(self, out):
        tc = self.tc
        none = [None] * (3 - self.nsets)
        bufs = ([self.sorted, u32(tc.bstart), u32(tc.bsize), u32(tc.ntask), u32(tc.rel), u32(tc.base), u32(self.task_bkt), u32(self.task_id)] + self.pb + none +
                [out[f"partial{k}"] for k in range(self.nsets)] + none)
        p = [self.c.id, self.nsets, self.rowlen, tc.Wg, tc.B, tc.T0, self.mshift, tc.T_top, tc.top_w, self.cap]
        for k in range(self.nsets):
            p += [self.idx_off[k], self.tab_n, self.fmts[k], self.nbases[k]]
        return bufs, p

    def expected(self):
        return {f"partial{k}": (self.want[k], _rows_aos(self.c.NW), None, None) for k in range(self.nsets)}

    def write_model(self, buf, k, want):
        _put_aos(buf, self.c, want)


def _acc_sizes(B, W, small, cut, top_cut, seed):
    """`small` buckets of 1 .. 5 entries, one bucket of 2 T + 1 (two full tasks and a remainder of one entry), and in the last window one of
    2 T_top + 1 if top_cut"""
    rs = np.random.RandomState(seed)
    v = np.zeros(W * B, dtype=np.int64)
    slots = rs.permutation((W - 1) * B)[:small + 1]
    v[slots[:small]] = rs.randint(1, 6, small)
    if cut:
        v[slots[small]] = 2 * ACC_T + 1
    if top_cut:
        v[(W - 1) * B + 3] = 4 * ACC_T + 1
    return v.reshape(W, B)


@functools.lru_cache(maxsize=None)
def acc_task_tables():
    """{ntasks: TaskCase}: 1; 63, 64, 65 (a ragged last wave, a bucket in three tasks with a remainder of one entry, the top window at T_top);
    130 (a hot bucket of 32 T + 1 entries cut at T >> 2: 129 tasks)"""
    T = ACC_T
    out = {1: SC.TaskCase("1 task", 3, 4, T, 2, True, [[0, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 0]])}
    for nt in (63, 64, 65):
        out[nt] = SC.TaskCase(f"{nt} tasks", 3, 32, T, 2, True, _acc_sizes(32, 3, nt - 6, True, True, nt))
    out[130] = SC.TaskCase("130 tasks", 3, 4, T, 2, False, [[0, 5, 0, 0], [0, 0, 32 * T + 1, 0], [0, 0, 0, 0]])
    out["merged"] = SC.TaskCase("merged 3 windows", 1, 16, T, 0, False, np.random.RandomState(8).randint(0, 75, (1, 16)))
    for k, t in out.items():
        assert k == "merged" or t.ntasks == k, (k, t.ntasks)
    return out


def acc_cases():
    out = []
    tt = acc_task_tables()
    for name in NAMES:
        fm = [BASES_72, BASES_64] if cv(name).ext else [BASES_72, BASES_64, BASES_ABI]
        j = 0
        for order in (0, 1):
            for i, nt in enumerate((1, 63, 64, 65, 130)):
                out.append(AccCase(name, tt[nt], [fm[(i + order) % len(fm)]], order, 200 + j))
                j += 1
            out.append(AccCase(name, tt[65], [fm[-1], fm[0]], order, 220 + j))
            out.append(AccCase(name, tt[63], [fm[1], fm[0], fm[-1]], order, 230 + j))
            out.append(AccCase(name, tt[130], [fm[0], fm[-1], fm[1]], order, 240 + j))
            for fmt in (BASES_72, BASES_64):
                out.append(AccCase(name, tt["merged"], [fmt], order, 250 + j + fmt, merged=3))
    return out
