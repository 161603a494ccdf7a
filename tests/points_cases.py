"""Inputs and expected statuses of the point-validation tests (tests/test_points_check_host.py on the CPU, tests/test_gpu_points_check.py on the
device).  The truth is computed here with Python integers alone: word values against p, the curve equation through pyoracle's field types,
and [r]P = O by a double-and-add of this module over Curve.add (Curve.mul reduces its scalar mod r and is useless outside the subgroup)."""
import functools
import importlib.util
import os

import numpy as np

from helpers import I, L, pt_to_np
from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KG_CHECK_CURVE, KG_CHECK_SUBGROUP = 1, 2
NON_CANONICAL, OFF_CURVE, NOT_IN_SUBGROUP = 1, 2, 4
Q, R = P.Q_MOD, P.R_MOD
H2 = 2 * Q - R                          # cofactor of the twist: #E'(Fq2) = r * h2, h2 = 10069 * 5864401 * (a 219-bit factor)
F1, F2 = 10069, 5864401


@functools.lru_cache(maxsize=None)
def psi_module():
    spec = importlib.util.spec_from_file_location("psi_consts", os.path.join(ROOT, "tools", "gen", "psi_consts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def mul_plain(cur, pt, k):
    """[k] pt by left-to-right double-and-add, k NOT reduced"""
    acc = None
    for bit in bin(k)[2:]:
        acc = cur.add(acc, acc)
        if bit == "1":
            acc = cur.add(acc, pt)
    return acc


_IN_SUBGROUP = {}


def in_subgroup(pt):
    """[r] pt == O for an on-curve point of the twist (memoised: the GPU tests reuse the points at several lengths)"""
    if pt is None:
        return True
    key = (pt[0].a, pt[0].b, pt[1].a, pt[1].b)
    if key not in _IN_SUBGROUP:
        _IN_SUBGROUP[key] = mul_plain(P.G2, pt, R) is None
    return _IN_SUBGROUP[key]


def point_from_words(cur, w):
    """ABI words (canonical) -> big-int affine point, on the curve or not"""
    p = cur.p
    v = [P.from_mont(I(w[4 * i:4 * i + 4]), p) for i in range(len(w) // 4)]
    return (P.Fq2(v[0], v[1]), P.Fq2(v[2], v[3])) if cur.ext else (v[0], v[1])


_CURVE_STATUS = {}


def _curve_status(cur, w):
    """(status of the canonicity and curve checks, the point when both pass), memoised by the words: the tests meet the same points at
    several lengths and masks"""
    key = (cur.name, w.tobytes())
    if key not in _CURVE_STATUS:
        if any(I(w[4 * i:4 * i + 4]) >= cur.p for i in range(len(w) // 4)):
            _CURVE_STATUS[key] = (NON_CANONICAL, None)
        else:
            pt = point_from_words(cur, w)
            _CURVE_STATUS[key] = (0, pt) if cur.on_curve(pt) else (OFF_CURVE, None)
    return _CURVE_STATUS[key]


def expected_status(cur, w, inf, checks):
    if inf:
        return 0
    st, pt = _curve_status(cur, np.ascontiguousarray(w, dtype=np.uint64))
    if st == 0 and (checks & KG_CHECK_SUBGROUP) and cur.ext and not in_subgroup(pt):
        return NOT_IN_SUBGROUP
    return st


def expected(cur, xy, inf, checks):
    """status bytes, bad count, first bad index of an (n, W) word array and its flags (None: no identities)"""
    st = np.array([expected_status(cur, xy[i], bool(inf[i]) if inf is not None else False, checks) for i in range(len(xy))], dtype=np.uint8)
    bad = np.flatnonzero(st)
    return st, len(bad), int(bad[0]) if len(bad) else len(xy)


def corrupt(cur, w, kind):
    """the replacements of the curve-check tests, applied to the words of a valid point"""
    w = w.copy()
    nw = len(w) // 2                     # words per coordinate
    p = cur.p
    if kind == "y+1":                    # y + 1 in the field (canonical, off the curve)
        y0 = P.from_mont(I(w[nw:nw + 4]), p)
        w[nw:nw + 4] = L(P.to_mont((y0 + 1) % p, p))
    elif kind == "swap":
        w = np.concatenate([w[nw:], w[:nw]])
    elif kind == "zero":                 # (0, 0) with flag 0: b != 0, off the curve
        w[:] = 0
    elif kind == "x+p":                  # the same residue, a word value >= p
        w[:4] = L(I(w[:4]) + p)
    elif kind == "y=p":
        w[nw:nw + 4] = L(p)
    elif kind == "ones":
        w[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    elif kind == "c1":                   # G2: a defect in the second component of y only
        y1 = P.from_mont(I(w[nw + 4:nw + 8]), p)
        w[nw + 4:nw + 8] = L(P.to_mont((y1 + 1) % p, p))
    else:
        raise ValueError(kind)
    return w


def curve_kinds(cur):
    return ["y+1", "swap", "zero", "x+p", "y=p", "ones"] + (["c1"] if cur.ext else [])


def curve_positions(n):
    """where the replacements go: index 0, n - 1, both sides of a wave boundary (63 | 64), and further workgroups of 64 at 257 and 1000"""
    pos = [0, n - 1, 63, 64, 1, n // 2, 130, 256, 700, 999]
    return sorted({q for q in pos if 0 <= q < n})


def curve_case(cur, valid, n, skip_first_group=False):
    """(xy, inf): `valid` (>= n, W) words of on-curve points; replacements dealt over curve_positions(n) (skip_first_group: none below index
    64, so that the lowest bad index lies outside the first workgroup); from 63 points on, two identity flags over garbage coordinates"""
    xy = valid[:n].copy()
    inf = np.zeros(n, dtype=np.uint8)
    kinds = curve_kinds(cur)
    pos = [q for q in curve_positions(n) if not (skip_first_group and q < 64)]
    for j, q in enumerate(pos):
        xy[q] = corrupt(cur, xy[q], kinds[j % len(kinds)])
    if n >= 63:                          # identities over garbage: all-ones words, and an off-curve point
        for q, kind in ((5, "ones"), (n - 3, "y+1")):
            if q not in pos:
                xy[q] = corrupt(cur, xy[q], kind)
                inf[q] = 1
    return xy, inf


@functools.lru_cache(maxsize=None)
def g2_special_points():
    """the case set of the subgroup check: [(name, point, in the subgroup?)] -- the third entry is what the construction promises; the tests
    take their truth from [r]P = O and assert that it agrees"""
    M, c, G = psi_module(), P.G2, P.G2.gen
    tw = [t for t in (M.twist_point(i) for i in range(1, 60)) if t is not None][:4]
    assert len(tw) == 4
    T, T2 = tw[0], tw[1]
    out = [("G", G, True)] + [(f"[{k}]G", c.mul(G, k), True) for k in (2, 3, 12345, R - 1)]
    out += [(f"T{i}", t, False) for i, t in enumerate(tw)]
    out += [(f"[h2]T{i}", mul_plain(c, t, H2), True) for i, t in enumerate(tw)]
    o1 = next(x for x in (mul_plain(c, t, R * H2 // F1) for t in tw) if x is not None)
    o2 = next(x for x in (mul_plain(c, t, R * H2 // F2) for t in tw) if x is not None)
    assert mul_plain(c, o1, F1) is None and mul_plain(c, o2, F2) is None
    out += [("order 10069", o1, False), ("order 5864401", o2, False), ("[r 10069 5864401]T", mul_plain(c, T, R * F1 * F2), False),
            ("G + T", c.add(G, T), False), ("G + T2", c.add(G, T2), False), ("order 10069 + G", c.add(o1, G), False)]
    out += [("-" + name, c.neg(pt), ok) for name, pt, ok in list(out)]
    for name, pt, ok in out:
        assert pt is not None and c.on_curve(pt), name
    return out


def g2_subgroup_case(valid, n):
    """(xy, names): the special points interleaved with `valid` (>= n, 16) words of subgroup points, cut to n points; n = 1 is an
    off-subgroup point alone"""
    sp = g2_special_points()
    if n == 1:
        return np.stack([pt_to_np(P.G2, sp[5][1])]), [sp[5][0]]
    xy, names, k = [], [], 0
    for i in range(n):
        if i % 3 == 1 and k < len(sp) or (i == n - 1 and k < len(sp)):
            xy.append(pt_to_np(P.G2, sp[k][1])); names.append(sp[k][0]); k += 1
        else:
            xy.append(valid[i]); names.append("valid")
    return np.stack(xy), names


def write_record(f, curve_id, checks, xy, inf):
    """one record of tests/host/points_check_host.cpp's case file"""
    n = len(xy)
    f.write(np.array([curve_id, checks], dtype=np.uint32).tobytes())
    f.write(np.array([n], dtype=np.uint64).tobytes())
    f.write(np.ascontiguousarray(xy, dtype=np.uint64).tobytes())
    f.write((np.zeros(n, dtype=np.uint8) if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)).tobytes())
