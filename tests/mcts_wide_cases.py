"""Inputs of the wide Monte Carlo tree search's comparisons with the checker
(tests/mcts_wide_ref.py), shared by tests/test_mcts_wide_host.py and
tests/test_gpu_mcts_wide.py: each reference is computed once per process and
left unchanged.  The roots are tests/mcts_cases.py's.

    set      roots                                          R x L              c          M
    small    mcts_cases.inputs("small"): 45 roots           10 x 4; 14 x 3 on  0.5        default
                                                            the first 12 roots
    wide     synthetic_cases.wide(4) (32 to 34 children)    3 x 16             0.5        default
             and the 20 synthetic_cases.edges() roots
    explore  mcts_cases.inputs("explore")                   10 x 4             0 and 4.0  default
    long     mcts_cases.inputs("long")                      16 x 16            0.5        default and 24

In `wide`, round 0 puts all 16 walkers on fresh children of one node; on the
finished game and the full boards all 16 end at a terminal root.  `long` at
M = 24 has 16 walkers a round on a tree with no room left.  The playouts are
the existing sets' number: 40, 48 (42), 40 and 256 leaf visits a root.
"""
import functools

import numpy as np

import mcts_cases
import mcts_ref
import mcts_wide_ref
import synthetic_cases

SEED, GAME_ID0 = mcts_cases.SEED, mcts_cases.GAME_ID0
FIELDS = mcts_cases.FIELDS
same = mcts_cases.same
# set -> [(rows or None: all, R, L, c, M or None: the default 1 + 16 R L)]
RUNS = {"small": ((None, 10, 4, 0.5, None), (12, 14, 3, 0.5, None)),
        "wide": ((None, 3, 16, 0.5, None),),
        "explore": ((None, 10, 4, 0.0, None), (None, 10, 4, 4.0, None)),
        "long": ((None, 16, 16, 0.5, None), (None, 16, 16, 0.5, 24))}
SETS = tuple(RUNS)


@functools.lru_cache(maxsize=None)
def _roots(name):
    if name != "wide":
        return mcts_cases.inputs(name)
    wb, wt = synthetic_cases.wide(4)
    eb, et, _ = synthetic_cases.edges()
    out = (np.ascontiguousarray(np.concatenate([wb, eb])), np.ascontiguousarray(np.concatenate([wt, et])))
    for a in out:
        a.setflags(write=False)
    return out


def inputs(name, rows=None):
    """(boards, turn) of a set, read-only; rows: only the first so many."""
    b, t = _roots(name)
    return (b, t) if rows is None else (b[:rows], t[:rows])


def runs(name):
    """[(rows, R, L, c, M)] of a set, M an int."""
    return [(rows, R, L, c, mcts_ref.default_nodes(R * L) if m is None else m) for rows, R, L, c, m in RUNS[name]]


@functools.lru_cache(maxsize=None)
def reference(name, rows, R, L, c, M):
    """The checker's answer on a run of a set, as a dict of read-only int64 arrays."""
    b, t = inputs(name, rows)
    r = mcts_wide_ref.mcts_wide(b, t, R, L, c=c, seed=SEED, game_id0=GAME_ID0, max_nodes=M)
    for a in r.values():
        a.setflags(write=False)
    return r
