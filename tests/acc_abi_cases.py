"""Bases that reach every branch of the accumulation's ABI-form gather (csrc/msm_bases.h load_point_abi, curve.h add_mixed_signed with abi = true):
shared by tests/test_acc_abi_bases_host.py (the bound checker on the CPU) and tests/test_gpu_acc_abi_bases.py (the kernels against the oracle).
Points are affine big-int pairs on the curve; pt_to_np (helpers.py) gives their ABI words."""
import json
import os

from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# G1 has a point with y = p - 1 (x^3 = -2 has a cube root in Fq); Grumpkin has none (18 is not a cube in Fr).  Both generators have x = 1.
G1_Y_IS_MINUS_ONE = (0x2409ED9A7B7567337C6BFD3B97E9703C9DEFFB228C6C7324D8A447837238B15E, P.Q_MOD - 1)


def _golden_points(cur, key):
    """every affine point of tests/golden/points.json's record of the curve, as big-int pairs"""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "points.json")))[key]
    found = []

    def walk(v):
        if isinstance(v, list) and len(v) == 2 and all(isinstance(c, str) for c in v):
            raw = tuple(int(c, 16) for c in v)
            for pt in (raw, tuple(P.from_mont(c, cur.p) for c in raw)):
                if max(pt) < cur.p and cur.on_curve(pt):
                    found.append(pt)
                    break
        elif isinstance(v, (list, tuple)):
            for c in v:
                walk(c)
        elif isinstance(v, dict):
            for c in v.values():
                walk(c)

    walk(rec)
    return found


def special_points(name):
    """[(label, point)]: the generator (x = 1), a point with y = p - 1 where the curve has one, and otherwise the golden points with the largest
    x and the largest y"""
    cur = {"g1": P.G1, "gk": P.GRUMPKIN}[name]
    out = [("generator", cur.gen)]
    assert cur.gen[0] == 1 and cur.on_curve(cur.gen)
    if name == "g1":
        assert cur.on_curve(G1_Y_IS_MINUS_ONE)
        out.append(("y = p - 1", G1_Y_IS_MINUS_ONE))
    else:
        assert pow(1 - cur.b, (cur.p - 1) // 3, cur.p) != 1          # no x with x^3 + b = (p - 1)^2
        pts = _golden_points(cur, name)
        assert len(pts) >= 2
        out.append(("largest golden x", max(pts, key=lambda q: q[0])))
        out.append(("largest golden y", max(pts, key=lambda q: q[1])))
    return out
