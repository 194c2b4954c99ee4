"""Inputs of the split search's comparisons with the exhaustive checker
(tests/search_ref.py), shared by tests/test_gpu_tree.py and the host build's
driver tools/diag/tree_host_check.py: the references are computed once per
process and left unchanged.

    mid3 / mid4 / mid5   the first 64 / 32 / 8 midgame roots of test_gpu_search.py's recipe, both tables
    deep9a               depth 9 at 10 empties (8 roots): eval and terminal leaves mixed
    deep9b               depth 9 at 11 empties (4 roots)
    deep10               depth 10 at 11 empties (2 roots)
    special3 / special9  every forced-pass and game-over root of solve_cases.cases() at 3..9 empties,
                         depth 3 (a pass at the root) and depth 9 with split 4 (passes and game-overs
                         inside the split plies)
"""
import functools

import numpy as np

import oracle
import search_ref
import solve_cases
from solve_ref import _bits
from subproc_amd import params

TABLES = {"default": np.asarray(params.DEFAULT_WEIGHTS, np.int8), "rng7": search_ref.WEIGHTS_B}
BOTH = ("default", "rng7")

# name -> (depth, splits, tables)
CASES = {
    "mid3": (3, (1, 2), BOTH),
    "mid4": (4, (1, 2, 3), BOTH),
    "mid5": (5, (1, 2, 3, 4), BOTH),
    "deep9a": (9, (1, 2, 3, 4), ("default",)),
    "deep9b": (9, (1, 2, 3, 4), ("default",)),
    "deep10": (10, (2, 3, 4), ("default",)),
    "special3": (3, (1, 2), BOTH),
    "special9": (9, (4,), ("default",)),
}
MID_ROOTS = {"mid3": 64, "mid4": 32, "mid5": 8}
LADDERS = {"deep9a": (10, 8), "deep9b": (11, 4), "deep10": (11, 2)}


@functools.lru_cache(maxsize=None)
def midgame():
    g = oracle.sample_midgame(4096, 0x5EED)
    for v in g.values():
        v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(boards, turn) of a case, read-only."""
    if name in MID_ROOTS:
        g, k = midgame(), MID_ROOTS[name]
        b, t = g["boards"][:k], g["turn"][:k]
    elif name in LADDERS:
        b, t = solve_cases.ladder(*LADDERS[name])
    else:
        cs = solve_cases.cases()
        es = [e for e in sorted(cs) if 3 <= e <= 9]
        sel = {e: cs[e]["forced_pass"] | cs[e]["over"] for e in es}
        b = np.concatenate([cs[e]["boards"][sel[e]] for e in es])
        t = np.concatenate([cs[e]["turn"][sel[e]] for e in es])
    b, t = np.ascontiguousarray(b), np.ascontiguousarray(t)
    b.setflags(write=False)
    t.setflags(write=False)
    return b, t


@functools.lru_cache(maxsize=None)
def reference(name, table):
    """The checker's (value, best_move, nodes_expanded) of a case."""
    b, t = inputs(name)
    v, m, expanded = search_ref.search(b, t, CASES[name][0], TABLES[table])
    v.setflags(write=False)
    m.setflags(write=False)
    return v, m, expanded


def expected_noroom(boards, turn, depth, split, slab):
    """Which roots must end as OTHT_NOROOM, by include/othello_tree.h's rule
    stated over the oracle alone: the tree grows a whole level at a time (the
    children of every node of the last level that is not final and has more
    than depth - split plies left; a node that must pass has one child, with the
    same plies left), a level that does not fit `slab` nodes is not made, and
    the root has no room when a node left unexpanded, not final, has more than
    8 plies to go."""
    out = np.zeros(len(turn), bool)
    for i in range(len(turn)):
        b = np.asarray(boards[i:i + 1], np.uint64)
        t = np.asarray(turn[i:i + 1], np.uint8)
        rem = np.array([depth])
        used = 1
        pending = np.zeros(0, np.int64)  # plies left of the nodes that stay tasks
        while True:
            own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
            final = (own == 0) & (opp == 0)
            grow = ~final & (rem > depth - split)
            pending = np.concatenate([pending, rem[~final & ~grow]])
            passes = grow & (own == 0)
            idx, sq = _bits(np.where(grow, own, np.uint64(0)))
            total = len(idx) + int(passes.sum())
            if total == 0 or used + total > slab:
                pending = np.concatenate([pending, rem[grow]])
                break
            kids = oracle.step(b[idx], t[idx], sq)["boards"]
            pi = np.nonzero(passes)[0]
            b, t, rem = (np.concatenate([kids, b[pi]]), np.concatenate([3 - t[idx], 3 - t[pi]]).astype(np.uint8),
                         np.concatenate([rem[idx] - 1, rem[pi]]))
            used += total
        out[i] = (pending > 8).any()
    return out


def symmetries(board):
    """The eight images of one 64-bit board under the square's symmetries."""
    sq = np.arange(64)
    x, y = sq & 7, sq >> 3
    out = []
    for fx, fy, tr in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        xx, yy = (7 - x if fx else x), (7 - y if fy else y)
        if tr:
            xx, yy = yy, xx
        dst = xx + 8 * yy
        v = 0
        for s in range(64):
            if int(board) >> s & 1:
                v |= 1 << int(dst[s])
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def opening_ties():
    """The opening's eight images, each also with the colours swapped (White to
    move): 16 roots (with repeats: the opening has symmetries of its own) whose
    maximisers tie four ways."""
    b, t, _ = oracle.reset(1)
    blacks, whites = symmetries(b[0, 0]), symmetries(b[0, 1])
    rows = [[bl, wh] for bl, wh in zip(blacks, whites)] + [[wh, bl] for bl, wh in zip(blacks, whites)]
    boards = np.array(rows, np.uint64)
    turn = np.array([int(t[0])] * 8 + [3 - int(t[0])] * 8, np.uint8)
    boards.setflags(write=False)
    turn.setflags(write=False)
    return boards, turn
