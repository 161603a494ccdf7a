"""The NTT tile kernels no automatic plan below 2^22 reaches, each at the smallest size a public knob runs it: one table, shared by the
host emulation (tests/test_host_ntt.py) and the device test (tests/test_gpu_ntt_shapes.py).

ntt_tile.h compiles one tile body into 31 kernels: 11 column shapes and 20 row shapes (LOG_M, LOG_TC), once per shell (k_ntt_tile,
k_ntt_tile_batch).  The automatic plans of 2^1..2^21 -- what tests/test_gpu_parity.py, test_gpu_large.py and test_gpu_ntt_batch.py compare
with the oracle -- use 22 of them; the rows below reach the other nine, and two roles the automatic sizes up to 2^22 give only at 256 MiB or
not at all (step B with its direct table on an (8,3) tile, a batched three-step plan).

A row is (knob environment, log_n, the plan kg_ntt_plan must report as [(log_m, log_tile)], batch count).  The knobs are read once per
process, so the rows of one environment share one child process; ONE_STEP needs no knob."""
import numpy as np

SEED = 0x4B6F676172617368
SENTINEL = 0x0DEADBEEF0DEADBE            # every word of every gap element of a strided batch
VARIANTS = {"dft": (False, False), "idft": (True, False), "coset_dft": (False, True), "coset_idft": (True, True)}
ORACLE_MAX_LOG = 18                       # up to here every transform of every variant is compared with the oracle

ROWS = [
    # env                                          log_n  plan                           batch     reaches
    ({"KG_NTT_TILE": "11"},                          14, [(7, 11), (7, 11)],               3),   # (7,4) column, row
    ({"KG_NTT_TILE": "11"},                          16, [(8, 11), (8, 11)],               3),   # (8,3) column, row
    ({"KG_NTT_TILE": "11"},                          18, [(9, 11), (9, 11)],               3),   # (9,2) column, row
    ({"KG_NTT_TILE": "10"},                          20, [(10, 10), (10, 10)],             2),   # (10,0) column; (10,0) row in a two-step plan
    ({"KG_NTT_TILE": "10"},                          21, [(11, 11), (10, 10)],             2),   # (11,0) column
    ({"KG_NTT_STEPS": "2", "KG_NTT_TILE": "10"},     22, [(11, 11), (11, 11)],             2),   # (11,0) column + (11,0) row in two steps
    ({"KG_NTT_STEPS": "2"},                          22, [(11, 12), (11, 12)],             2),   # (11,1) row
    ({"KG_NTT_STEPS": "3", "KG_NTT_TILE": "11"},     21, [(7, 11), (8, 11), (6, 10)],      2),   # (8,3) as step B with its direct table
    ({"KG_NTT_STEPS": "3"},                          18, [(6, 10), (6, 10), (6, 10)],      3),   # a batched three-step plan at 8 MiB
]
ONE_STEP = list(range(1, 12))             # 2^1..2^11: extreme inputs for every one-step kernel, in the test's own process


def env_id(env):
    return "_".join(f"{k[7:].lower()}{v}" for k, v in sorted(env.items()))          # "steps3_tile11"


def environments():
    """the distinct knob environments, in table order"""
    out = []
    for env, *_ in ROWS:
        if env not in out:
            out.append(env)
    return out


def rows_of(env):
    return [r for r in ROWS if r[0] == env]


def knobs(env):
    """(steps, tile) as ntt_plan takes them"""
    return int(env.get("KG_NTT_STEPS", 0)), int(env.get("KG_NTT_TILE", 0))


def kernels_of(plan):
    """the (log_m, log_tc, row) kernels a plan [(log_m, log_tile)] launches: the last step is the row step"""
    return {(m, t - m, i == len(plan) - 1) for i, (m, t) in enumerate(plan)}


def seed_of(log_n):
    return SEED + 8000 + 16 * log_n       # transform b of a batch is gen_scalars(seed_of(log_n) + b)


def extreme_vectors(O, log_n):
    """the inputs that push the lazy sums hardest, as one (3, n, 4) array: every element p - 1, alternating p - 1 / 0, a single p - 1 at
    index n - 1 (Montgomery form, like every element the ABI takes)"""
    n = 1 << log_n
    pm1 = O.f_consts(0)["p"].copy()
    pm1[0] -= 1
    top = O.f_to_mont(0, pm1)
    v = np.zeros((3, n, 4), dtype=np.uint64)
    v[0] = top
    v[1, 0::2] = top
    v[2, n - 1] = top
    return v
