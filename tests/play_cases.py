"""The self-play cases the GPU tests compare with the checker (tests/play_ref.py),
each with its reference computed once and left read-only.  The host build
(tools/diag/play_host.cpp, tools/diag/play_host_check.py) runs the same cases."""
import functools

import numpy as np

import oracle
import play_ref
import search_ref
from subproc_amd import params

DEFAULT = np.asarray(params.DEFAULT_WEIGHTS, np.int8)
# test_gpu_search.py's "extreme" table: the second table pushed to the ends of int8
EXTREME = np.where(search_ref.WEIGHTS_B > 0, 127, -128).astype(np.int8)
EXTREME[search_ref.WEIGHTS_B == -127] = -127
TABLES = {"default": DEFAULT, "rng7": search_ref.WEIGHTS_B, "extreme": EXTREME}

# name -> the games' arguments: n, seed, game_id0, tables, depths, exact_empties,
# budgets, swap, and where the games start ("mid": the first n midgame samples)
CASES = {
    "mid64_d3v2": dict(n=64, seed=101, game_id0=0, tables=("default", "rng7"), depth=(3, 2), exact=0, n_rand=(0, 0),
                       swap=True, start="mid"),
    "mid64_d2v3": dict(n=64, seed=102, game_id0=7, tables=("default", "rng7"), depth=(2, 3), exact=0, n_rand=(0, 0),
                       swap=True, start="mid"),
    "open32_d3v3": dict(n=32, seed=103, game_id0=1000, tables=("default", "rng7"), depth=(3, 3), exact=0,
                        n_rand=(3, 12), swap=True, start=None),
    "mid32_d4v1": dict(n=32, seed=104, game_id0=0, tables=("default", "rng7"), depth=(4, 1), exact=0, n_rand=(0, 0),
                       swap=True, start="mid"),
    "mid8_d5v2": dict(n=8, seed=105, game_id0=3, tables=("rng7", "default"), depth=(5, 2), exact=0, n_rand=(0, 0),
                      swap=True, start="mid"),
    "mid64_extreme_d2": dict(n=64, seed=106, game_id0=0, tables=("extreme", "default"), depth=(2, 2), exact=0,
                             n_rand=(0, 0), swap=True, start="mid"),
    # the exact endgame: mid64_d2v3's games with the last eight empties searched to the end
    "mid64_d2v3_exact8": dict(n=64, seed=102, game_id0=7, tables=("default", "rng7"), depth=(2, 3), exact=8,
                              n_rand=(0, 0), swap=True, start="mid"),
}


@functools.lru_cache(maxsize=None)
def midgame(n=4097):
    g = oracle.sample_midgame(n, 0x5EED)
    for v in g.values():
        v.setflags(write=False)
    return g


def starts(case):
    """(boards, turn) of a case's games, or (None, None) from the opening."""
    c = CASES[case]
    if c["start"] is None:
        return None, None
    g = midgame()
    return g["boards"][:c["n"]], g["turn"][:c["n"]]


@functools.lru_cache(maxsize=None)
def reference(case):
    """play_ref.play's games of a case."""
    c = CASES[case]
    b, t = starts(case)
    wa, wb = TABLES[c["tables"][0]], TABLES[c["tables"][1]]
    r = play_ref.play(c["n"], c["seed"], play_ref.search_chooser(wa, wb, c["depth"][0], c["depth"][1], c["exact"]),
                      game_id0=c["game_id0"], n_rand_a=c["n_rand"][0], n_rand_b=c["n_rand"][1], swap=c["swap"],
                      start=b, start_turn=t)
    for v in r.values():
        v.setflags(write=False)
    return r
