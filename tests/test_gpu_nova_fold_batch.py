"""NovaProver.prove_batch on the device: many folding steps of one shape in two enqueued phases (fold_begin: cross terms and their
commitments; fold_end: the witness, error and instance folds).  Element b must equal NovaProver.prove on pair b in every word and flag, the
oracle's cross term and commitment, big-integer folds of witness and instance (pyoracle point arithmetic), and -- over Fr, where the pairs
satisfy the chain circuit -- the folded pairs must satisfy the relaxed relation.  Nothing here has a tolerance."""
import numpy as np
import pytest

from r1cs_cases import random_shape

pytestmark = pytest.mark.gpu
SEED = 0x4B6F676172617368 + 8000
M, COUNT = 300, 5


@pytest.fixture(scope="module")
def ctx():
    import kogarashi_amd as K
    c = K.Context(0)
    yield c
    c.close()


def same_point(a, b):
    return int(a[1]) == int(b[1]) and (np.asarray(a[0], dtype=np.uint64).reshape(-1) == np.asarray(b[0], dtype=np.uint64).reshape(-1)).all()


def assert_same_fold(got, want, what):
    """(instance, witness, commit_t) against (instance, witness, commit_t): every word and flag"""
    gi, gw, gt = got
    wi, ww, wt = want
    assert same_point(gt, wt), (what, "commit_t")
    for name in ("commit_w", "commit_e"):
        assert same_point(gi[name], wi[name]), (what, name, gi[name], wi[name])
    for name, g, w in (("u", gi["u"], wi["u"]), ("x", gi["x"], wi["x"]), ("w", gw["w"], ww["w"]), ("e", gw["e"], ww["e"])):
        g, w = np.asarray(g, dtype=np.uint64), np.asarray(w, dtype=np.uint64)
        assert g.shape == w.shape and (g == w).all(), (what, name)


class World:
    """one shape, key and prover over (fd, curve), seven fresh instance-witness pairs and the five pairs of the batch"""

    def __init__(self, ctx, O, fd, curve, m):
        import kogarashi_amd as K
        self.O, self.fd, self.m = O, fd, m
        self.one = O.f_consts(fd)["r"]
        if fd == 0:                                    # the oracle's chain circuit lives over Fr: satisfied pairs
            css = [O.chain_r1cs(m, O.gen_scalars(0, SEED + j, 0, 1)[0]) for j in range(7)]
            self.shape = (css[0].a, css[0].b, css[0].c)
            self.xs, self.ws = [cs.x[1:] for cs in css], [cs.w for cs in css]     # columns are (x | w) with x[0] = 1 = the one-wire u
        else:                                          # the Fq run folds unsatisfied random data
            lx, lw = 2, max(2 * m // 3, 2)
            self.shape = random_shape(O, fd, m, 1 + lx + lw, SEED + 20 + m)
            self.xs = [O.gen_scalars(fd, SEED + 30 + j, 0, lx) for j in range(7)]
            self.ws = [O.gen_scalars(fd, SEED + 40 + j, 0, lw) for j in range(7)]
        self.g = O.gen_bases(curve, SEED + 50, 0, m + 1)
        self.ck = K.PedersenCommitment(self.g, curve=curve, ctx=ctx)
        self.prover = K.NovaProver(self.shape, self.ck, ctx=ctx)
        self.rs = O.gen_scalars(fd, SEED + 60, 0, COUNT)
        self.rs[2] = 0                                 # one pair with r = 0
        folded1 = self.prover.prove(*self.relaxed(1), *self.fresh(2), O.gen_scalars(fd, SEED + 61, 0, 1)[0])
        folded2 = self.prover.prove(*folded1[:2], *self.fresh(3), O.gen_scalars(fd, SEED + 62, 0, 1)[0])
        self.pairs = [self.relaxed(0) + self.fresh(4),             # fresh relaxed: u = 1, E = 0, commit_e the identity
                      folded1[:2] + self.fresh(5),                 # already folded: u != 1, E != 0, commit_e not the identity
                      self.relaxed(6) + self.fresh(0),             # r = 0
                      folded2[:2] + self.fresh(6),                 # folded twice
                      self.relaxed(3) + self.fresh(3)]             # both sides the same witness

    def fresh(self, j):
        return {"commit_w": self.ck.commit(self.ws[j]), "x": self.xs[j]}, {"w": self.ws[j]}

    def relaxed(self, j):
        return ({"commit_w": self.ck.commit(self.ws[j]), "commit_e": (np.zeros(8, dtype=np.uint64), 1), "u": self.one, "x": self.xs[j]},
                {"w": self.ws[j], "e": np.zeros((self.m, 4), dtype=np.uint64)})


_WORLDS = {}


@pytest.fixture
def world(ctx, oracle, request):
    fd, curve = request.param
    if (fd, curve) not in _WORLDS:
        _WORLDS[(fd, curve)] = World(ctx, oracle, fd, curve, M)
    return _WORLDS[(fd, curve)]


BOTH = pytest.mark.parametrize("world", [(0, 0), (1, 1)], indirect=True, ids=["Fr G1", "Fq Grumpkin"])


@BOTH
def test_batch_equals_prove_per_pair_and_big_integer_folds(world, pyoracle):
    from helpers import CURVES, I, L, np_to_pt, pt_to_np
    W, O, P = world, world.O, pyoracle
    cv = "g1" if W.fd == 0 else "gk"
    cur = CURVES[cv][1]
    p = cur.n
    to_int = lambda a: [P.from_mont(I(row), p) for row in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)]
    to_np = lambda vals: np.array([L(P.to_mont(v % p, p)) for v in vals], dtype=np.uint64).reshape(-1, 4)
    pt = lambda c: np_to_pt(cur, c[0], c[1])
    folded = W.pairs[1]                                  # the already-folded pair is what it is meant to be
    assert not folded[0]["commit_e"][1] and (np.asarray(folded[0]["u"]) != W.one).any() and np.asarray(folded[1]["e"]).any()
    got = W.prover.prove_batch(W.pairs, W.rs)
    assert len(got) == COUNT
    for b, (i1, w1, i2, w2) in enumerate(W.pairs):
        inst, wit, commit_t = got[b]
        assert_same_fold(got[b], W.prover.prove(i1, w1, i2, w2, W.rs[b]), b)
        # the cross term and its commitment: the oracle's restatement
        z1 = np.concatenate([np.asarray(i1["u"]).reshape(1, 4), i1["x"], w1["w"]])
        z2 = np.concatenate([W.one.reshape(1, 4), i2["x"], w2["w"]])
        t = O.nova_cross_term(W.fd, W.shape[0], W.shape[1], W.shape[2], z1, z2, np.asarray(i1["u"]).reshape(4), W.one)
        nc = min(W.m, len(W.g))
        assert same_point(commit_t, O.commit_naive(cv, W.g[:nc], t[:nc]))
        # big-integer folds
        ri = to_int(W.rs[b])[0]
        assert (ri == 0) == (b == 2)
        assert (wit["w"] == to_np([x + ri * y for x, y in zip(to_int(w1["w"]), to_int(w2["w"]))])).all()
        assert (wit["e"] == to_np([x + ri * y for x, y in zip(to_int(w1["e"]), to_int(t))])).all()
        assert (inst["u"] == to_np([to_int(i1["u"])[0] + ri])[0]).all()
        assert (inst["x"] == to_np([x + ri * y for x, y in zip(to_int(i1["x"]), to_int(i2["x"]))])).all()
        for name, a, c in (("commit_w", i1["commit_w"], i2["commit_w"]), ("commit_e", i1["commit_e"], commit_t)):
            want = cur.add(pt(a), cur.mul(pt(c), ri))
            g = inst[name]
            assert (want is None) == bool(g[1]) and (want is None or (g[0] == pt_to_np(cur, want)).all()), (b, name)
        # the commitments of the folded witness are the folded commitments
        assert same_point(W.ck.commit(wit["w"]), inst["commit_w"]) and same_point(W.ck.commit(wit["e"]), inst["commit_e"]), b
    assert got[0][0]["commit_e"][1] == 0 and got[2][0]["commit_e"][1] == 1            # r = 0 keeps the identity commit_e, r != 0 leaves it
    if W.fd == 0:                                        # the folded pairs satisfy the relaxed relation
        sums = W.prover.check_batch([(i["u"], i["x"], w["w"], w["e"]) for i, w, _ in got])
        assert sums.tolist() == [[0, W.m]] * COUNT


@BOTH
def test_callable_challenges_and_a_second_batch_from_the_first(world):
    W = world
    seen = []

    def transcript(commit_ts):
        seen.append(commit_ts)
        return W.rs

    first = W.prover.prove_batch(W.pairs, transcript)
    plain = W.prover.prove_batch(W.pairs, W.rs)
    assert len(seen) == 1 and len(seen[0]) == COUNT
    for b in range(COUNT):
        assert_same_fold(first[b], plain[b], b)
        assert same_point(seen[0][b], plain[b][2])
    # the second batch starts from the first batch's outputs
    rs2 = W.O.gen_scalars(W.fd, SEED + 70, 0, 3)
    pairs2 = [(first[b][0], first[b][1]) + W.fresh(b + 1) for b in range(3)]
    second = W.prover.prove_batch(pairs2, rs2)
    for b in range(3):
        assert_same_fold(second[b], W.prover.prove(*pairs2[b], rs2[b]), ("second", b))
    if W.fd == 0:
        assert W.prover.check_batch([(i["u"], i["x"], w["w"], w["e"]) for i, w, _ in second]).tolist() == [[0, W.m]] * 3
    assert W.prover.prove_batch([], W.rs[:0]) == []


@pytest.mark.parametrize("fd,curve", [(0, 0), (1, 1)])
def test_one_constraint_one_pair(ctx, oracle, fd, curve):
    """m = 1, count = 1 (over Fq the random shape's single row is empty: T = 0 and commit_T is the identity)"""
    W = World(ctx, oracle, fd, curve, 1)
    got = W.prover.prove_batch(W.pairs[1:2], W.rs[1:2])
    assert len(got) == 1
    assert_same_fold(got[0], W.prover.prove(*W.pairs[1], W.rs[1]), "m = 1")
