"""Inputs of tests/test_gpu_long_edges.py and their census (tests/test_long_edges_host.py): MSMs of N = 600 pairs whose bucket reductions meet the
exceptional exits of the point formulas on purpose, for every window width the long pipeline is forced to.

Bases come from a pool of a dozen subgroup points m_i * G and their negatives, made with pyoracle; every base therefore has a known multiplier,
and a bucket's sum is known as a multiplier modulo the group order (the groups have prime order: two sums are equal points exactly when their
multipliers are equal).  Nothing here needs a GPU."""
import random

import numpy as np

from helpers import CURVES, L, pt_to_np
from oracle import pyoracle as P

N = 600
POOL = 12
STAIR_WIDTHS = tuple(range(2, 14))
OTHER_WIDTHS = (2, 8, 9, 10, 11, 13, 0)               # 0: the automatic width; 9, 10, 11 cross B = 256 (one lane), 8, 9, 10 B = 128 (lane pair)
HOT_N = 1100                                          # pairs of the hot-bucket patterns: more than GATHER_SUM_MAX * 32 entries in one bucket
CLASSES = ("equal", "opposite", "one side empty", "both empty", "ordinary")

_pools, _patterns = {}, {}


def pool(cv):
    """[(multiplier, point)]: POOL points m * G, then their negatives"""
    if cv not in _pools:
        cur = CURVES[cv][1]
        rnd = random.Random(0x600 + CURVES[cv][0])
        ms = [rnd.randrange(2, cur.n) for _ in range(POOL)]
        pts = [cur.mul(cur.gen, m) for m in ms]
        _pools[cv] = [(m, pt) for m, pt in zip(ms, pts)] + [(cur.n - m, cur.neg(pt)) for m, pt in zip(ms, pts)]
    return _pools[cv]


class Pattern:
    """idx: pool index of every base; ks: canonical scalars; inf: identity flags or None; closed: the sum's multiplier in closed form, or None"""

    def __init__(self, cv, name, idx, ks, inf=None, closed=None):
        cur = CURVES[cv][1]
        pl = pool(cv)
        self.cv, self.name, self.idx, self.ks, self.closed = cv, name, list(idx), [k % cur.n for k in ks], closed
        assert len(self.idx) == len(self.ks)
        self.inf = None if inf is None else np.asarray(inf, dtype=np.uint8)
        rows = {i: pt_to_np(cur, pl[i][1]) for i in set(self.idx)}
        self.bases = np.stack([rows[i] for i in self.idx])
        mont = {k: L(P.to_mont(k, cur.n)) for k in set(self.ks)}
        self.scalars = np.stack([mont[k] for k in self.ks])

    def mults(self):
        """the multiplier of every base, 0 where the identity flag is set"""
        pl = pool(self.cv)
        return [0 if (self.inf is not None and self.inf[j]) else pl[i][0] for j, i in enumerate(self.idx)]

    def total(self):
        n = CURVES[self.cv][1].n
        return sum(m * k for m, k in zip(self.mults(), self.ks)) % n


def patterns(cv):
    if cv in _patterns:
        return _patterns[cv]
    cur = CURVES[cv][1]
    n, pl = cur.n, pool(cv)
    rnd = random.Random(0x6000 + CURVES[cv][0])
    m0 = pl[0][0]
    stair = list(range(1, N + 1))
    k1 = rnd.randrange(1 << 200, n)
    out = [
        Pattern(cv, "staircase", [0] * N, stair, closed=m0 * sum(stair) % n),
        Pattern(cv, "cancelling staircase, P on odd", [0 if k % 2 else POOL for k in stair], stair, closed=m0 * sum(k if k % 2 else -k for k in stair) % n),
        Pattern(cv, "cancelling staircase, P on even", [POOL if k % 2 else 0 for k in stair], stair, closed=m0 * sum(-k if k % 2 else k for k in stair) % n),
        Pattern(cv, "one bucket, random scalar", [0] * N, [k1] * N, closed=m0 * k1 * N % n),
        Pattern(cv, "one bucket, alternating +-P", [0 if j % 2 == 0 else POOL for j in range(N)], [k1] * N, closed=0),
        Pattern(cv, "one bucket, scalars 1", [0] * N, [1] * N, closed=m0 * N % n),
    ]
    ks = [0] * N
    for j in (5, 77, N - 1):
        ks[j] = rnd.randrange(1, n)
    inf = np.zeros(N, dtype=np.uint8)
    inf[[3, 77, 400]] = 1                                                  # one of the three non-zero scalars meets an identity base
    out.append(Pattern(cv, "sparse", [rnd.randrange(2 * POOL) for _ in range(N)], ks, inf=inf))
    # edge_mix of the parity tests over the pool: an identity base, a zero scalar, a duplicate point, P and -P under 1 and -1, a pair repeated
    idx = [rnd.randrange(2 * POOL) for _ in range(N)]
    ks = [rnd.randrange(n) for _ in range(N)]
    inf = np.zeros(N, dtype=np.uint8)
    inf[2] = 1; ks[1] = 0; idx[3] = idx[0]; idx[5] = idx[4]; ks[6] = ks[7]; idx[6] = idx[7]; ks[4] = 1; ks[5] = n - 1
    out.append(Pattern(cv, "edge_mix", idx, ks, inf=inf))
    assert all(len(p.ks) == N for p in out)
    _patterns[cv] = out
    return out


def hot_patterns(cv):
    """the one-bucket patterns at HOT_N pairs: one bucket per window holds more entries than GATHER_SUM_MAX tasks of the shortest task length"""
    cur = CURVES[cv][1]
    m0 = pool(cv)[0][0]
    k1 = patterns(cv)[3].ks[0]
    n = HOT_N
    return [Pattern(cv, "hot bucket, random scalar", [0] * n, [k1] * n, closed=m0 * k1 * n % cur.n),
            Pattern(cv, "hot bucket, alternating +-P", [0 if j % 2 == 0 else POOL for j in range(n)], [k1] * n, closed=0),
            Pattern(cv, "hot bucket, scalars 1", [0] * n, [1] * n, closed=m0 * n % cur.n)]


def widths(pat):
    return STAIR_WIDTHS if "staircase" in pat.name else OTHER_WIDTHS


def auto_width():
    return 8                                                                # pick_window (msm_sort.hip): 2^7 <= N < 2^10


def kwords(ks):
    return np.array([[(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for k in ks], dtype=np.uint32)


def bucket_multipliers(pat, c, digits):
    """{(window, bucket): (entries, multiplier of the sum)} from the signed digits (digits[i][w]; digit d lands in bucket |d| - 1 with its sign)"""
    n = CURVES[pat.cv][1].n
    W = (255 + c - 1) // c
    B = 1 << (c - 1)
    cnt, val = {}, {}
    for i, m in enumerate(pat.mults()):
        if pat.inf is not None and pat.inf[i]:
            continue
        for w in range(W):
            d = int(digits[i][w])
            if d:
                key = (w, abs(d) - 1)
                assert abs(d) <= B
                cnt[key] = cnt.get(key, 0) + 1
                val[key] = (val.get(key, 0) + (m if d > 0 else -m)) % n
    return cnt, val, W, B


def level1_census(pat, c, digits):
    """how many level-1 nodes (buckets 2i, 2i + 1 of a window) of each class the halving tree adds"""
    n = CURVES[pat.cv][1].n
    cnt, val, W, B = bucket_multipliers(pat, c, digits)
    cen = {k: 0 for k in CLASSES}
    for w in range(W):
        for i in range(B // 2):
            a, b = val.get((w, 2 * i), 0), val.get((w, 2 * i + 1), 0)
            if a == 0 and b == 0:
                cen["both empty"] += 1
            elif a == 0 or b == 0:
                cen["one side empty"] += 1
            elif a == b:
                cen["equal"] += 1
            elif (a + b) % n == 0:
                cen["opposite"] += 1
            else:
                cen["ordinary"] += 1
    cen["largest bucket"] = max(cnt.values()) if cnt else 0
    cen["recomposed"] = sum(m * sum(int(digits[i][w]) << (w * c) for w in range(W)) for i, m in enumerate(pat.mults())) % n
    return cen


def promised(pat, c):
    """the classes a (pattern, width) must show at level 1, by the construction of the pattern:
    staircase, window 0, B = 2^(c-1): bucket r - 1 (1 <= r < B) takes +P from every k = r (mod 2B) and -P from every k = -r (mod 2B) of 1 .. 600.
      With 600 = q 2B + s the first happens q + [r <= s] times and the second q + [r >= 2B - s] times, so the bucket holds P for r <= s (s < B) or
      for r < 2B - s (s >= B) and the identity beyond: neighbouring buckets 2i, 2i + 1 hold the same P as soon as that range reaches r = 2, which it
      does for every c >= 4 (600 mod 16, 32, ... = 8, 24, 24, 88, 88, 88, then 600 itself).  c = 2, 3 promise nothing of the kind.
      The high windows are empty: both-empty nodes (c >= 3: several nodes per window).
    cancelling staircase: 2B is even, so every k that meets bucket r - 1 has the parity of r: the same buckets hold +-P with alternating signs and the
      nodes of that range cancel (c >= 4).
    one bucket / sparse: at most three non-empty buckets per window: one-side-empty nodes and both-empty nodes; alternating +-P: identities only.
    edge_mix, c <= 5: 600 random digits over at most 16 buckets: ordinary nodes."""
    want = set()
    if pat.name == "staircase":
        want |= ({"equal"} if c >= 4 else set()) | ({"both empty"} if c >= 3 else set())
    elif pat.name.startswith("cancelling"):
        want |= ({"opposite"} if c >= 4 else set()) | ({"both empty"} if c >= 3 else set())
    elif "alternating" in pat.name:                                         # every bucket sums to the identity
        want |= {"both empty"}
    elif pat.name.startswith("one bucket") or pat.name == "sparse":
        want |= {"one side empty"} | ({"both empty"} if c >= 3 else set())
    elif pat.name == "edge_mix" and c <= 5:
        want |= {"ordinary"}
    return want
