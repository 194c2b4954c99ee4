"""Inputs of the Monte Carlo tree search's comparisons with the checker
(tests/mcts_ref.py), shared by tests/test_mcts_host.py and
tests/test_gpu_mcts.py: each set and each reference is computed once per
process and left unchanged.

    set      roots                                                          T    c          M
    small    the first 12 roots of oracle.sample_midgame(.., 0x5EED); all   40   0.5        default
             20 synthetic_cases.edges() roots (the empty board, full
             boards, a root pass, a game that is over); synthetic_cases.
             wide(4) (32 to 34 children); 6 solve_cases roots at 1 to 3
             empties; one overlapping board
    explore  6 midgame roots                                                40   0 and 4.0  default
    long     2 midgame roots                                                256  0.5        default and 24

`long` at M = 24 makes the tree run out of room: the no-expansion branch runs.
"""
import functools

import numpy as np

import mcts_ref
import oracle
import solve_cases
import synthetic_cases

SEED, GAME_ID0 = 0xC0FFEE, 1 << 40
OVERLAP = (np.array([[3, 1]], np.uint64), np.array([1], np.uint8))
# set -> (T, the (c, M) runs; M None = the default 1 + 16 T)
RUNS = {"small": (40, ((0.5, None),)), "explore": (40, ((0.0, None), (4.0, None))),
        "long": (256, ((0.5, None), (0.5, 24)))}
FIELDS = ("visits", "wins", "diffs", "root_wins", "root_diffs", "best_move", "status", "nodes")


def _freeze(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def midgame():
    g = oracle.sample_midgame(20, 0x5EED)
    return _freeze(g["boards"], g["turn"])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(boards, turn) of a set, read-only."""
    mb, mt = midgame()
    if name == "small":
        eb, et, _ = synthetic_cases.edges()
        cs = solve_cases.cases()
        parts = [(mb[:12], mt[:12]), (eb, et), synthetic_cases.wide(4)]
        parts += [(cs[e]["boards"][:2], cs[e]["turn"][:2]) for e in (1, 2, 3)]
        parts.append(OVERLAP)
    elif name == "explore":
        parts = [(mb[12:18], mt[12:18])]
    else:
        parts = [(mb[18:20], mt[18:20])]
    return _freeze(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def runs(name):
    """[(T, c, M)] of a set, M an int."""
    T, cms = RUNS[name]
    return [(T, c, mcts_ref.default_nodes(T) if m is None else m) for c, m in cms]


@functools.lru_cache(maxsize=None)
def reference(name, T, c, M):
    """The checker's answer on a set, as a dict of read-only int64 arrays."""
    b, t = inputs(name)
    r = mcts_ref.mcts(b, t, T, c=c, seed=SEED, game_id0=GAME_ID0, max_nodes=M)
    for a in r.values():
        a.setflags(write=False)
    return r


def same(got, want, what, fields=FIELDS):
    """Every field of ``got`` (anything indexable by the names) is the reference's."""
    for k in fields:
        w = want[k]
        g = np.asarray(got[k]).astype(np.int64).reshape(w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
