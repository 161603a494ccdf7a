"""Census of the inputs of tests/test_gpu_long_edges.py, without a GPU: the signed digits come from the product's own host build
(ht_small_digits: the rule msm_digits.h says the long sort shares), every bucket's sum is known through the bases' multipliers, and for every
(pattern, width) the first level of the halving tree must hold the classes of nodes the pattern promises.  The closed forms of the expected
sums agree with the C oracle and with pyoracle's own MSM."""
import ctypes as C

import numpy as np
import pytest

import long_edge_cases as LE
from helpers import CURVES, np_to_pt, p32


def digits_of(hostlib, ks, c):
    kw = LE.kwords(ks)
    dig = np.zeros((len(ks), 128), dtype=np.int32)
    hostlib.ht_small_digits(p32(kw), C.c_size_t(len(ks)), c, dig.ctypes.data_as(C.POINTER(C.c_int32)))
    return dig


@pytest.mark.parametrize("cv", ["g1", "gk", "g2"])
def test_every_pattern_and_width_holds_the_promised_nodes(hostlib, cv):
    seen = {k: set() for k in LE.CLASSES}
    for pat in LE.patterns(cv):
        for c in LE.widths(pat):
            c = c or LE.auto_width()
            cen = LE.level1_census(pat, c, digits_of(hostlib, pat.ks, c))
            assert cen["recomposed"] == pat.total(), (pat.name, c, "the digits do not recompose the scalars")
            for cls in LE.promised(pat, c):
                assert cen[cls] >= 1, (cv, pat.name, c, cls, cen)
            for cls in LE.CLASSES:
                if cen[cls]:
                    seen[cls].add(c)
            if pat.name.startswith("one bucket"):
                assert cen["largest bucket"] == LE.N, (pat.name, c)          # one bucket per window takes every pair
    for c in (2, 8, 9, 10, 13):                                              # every width of the short list meets every class in some pattern
        missing = [cls for cls in LE.CLASSES if c not in seen[cls]]
        assert not missing or c == 2, (cv, c, missing)                       # (c = 2: one node per window)


@pytest.mark.parametrize("cv", ["g1", "gk", "g2"])
def test_closed_forms_agree_with_the_oracles(oracle, pyoracle, cv):
    cid, cur, _ = CURVES[cv]
    for pat in LE.patterns(cv):
        want = cur.mul(cur.gen, pat.total())
        if pat.closed is not None:
            assert pat.closed == pat.total(), pat.name
        xy, inf = oracle.to_affine(cv, oracle.msm(cv, pat.bases, pat.scalars, pat.inf, threads=8))
        assert np_to_pt(cur, xy, inf) == want, (cv, pat.name)
