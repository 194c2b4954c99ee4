"""Expected answers of the principal-variation calls (include/othello_line.h,
DESIGN.md §24), with no knowledge of the code under test: the header's walk
over the oracle alone.

A walk holds (position, side to move t, plies left rem, root mover r) and
repeats: neither side can move -> stop; rem == 0 (search) -> stop; t must pass
-> append 64, hand the move over; otherwise append the LOWEST square among t's
moves that maximise minus the child's value, play it, rem -= 1.  The child's
value is solve_ref.solve's (exact) or moves_ref.search_rooted's with the root
mover passed in (search), over moves_ref.children.  All walks of a batch advance
together, one ply per round.  Results are cached per process and read-only.

The assertion at the bottom pins it: the first move and the value are
solve_ref's / search_ref.search's on a few roots.
"""
import functools

import numpy as np

import moves_ref
import oracle
import search_ref
import solve_cases
import solve_ref
import tree_cases
from solve_ref import mover

T = search_ref.T
PASS, NO_MOVE = 64, 255
STRIDE = 32
UNBOUNDED = 99  # the exact walk's rem


def _walk(boards, turn, rem, child_value):
    """dict(line (n, 32) uint8, length, best_move, end_boards, end_turn); child_value(boards, turn, root, rem) is
    the value of each child from ITS mover's side."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2).copy()
    t = mover(turn).copy()
    r = t.copy()
    rem = np.asarray(rem, np.int64).copy()
    n = len(b)
    line = np.full((n, STRIDE), NO_MOVE, np.uint8)
    length = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    while live.any():
        idx = np.nonzero(live)[0]
        own = oracle.legal(b[idx], t[idx])
        opp = oracle.legal(b[idx], (3 - t[idx]).astype(np.uint8))
        over = (own == 0) & (opp == 0)
        stop = over | (rem[idx] == 0)
        live[idx[stop]] = False
        pi = idx[~stop & (own == 0)]
        line[pi, length[pi]] = PASS
        length[pi] += 1
        t[pi] = 3 - t[pi]
        mi = idx[~stop & (own != 0)]
        if len(mi) == 0:
            continue
        ci, csq, cb, ct, _, _ = moves_ref.children(b[mi], t[mi])
        cv = -np.asarray(child_value(cb, ct, r[mi][ci], rem[mi][ci] - 1), np.int64)
        best = np.full(len(mi), -(1 << 40), np.int64)
        np.maximum.at(best, ci, cv)
        hit = cv == best[ci]
        mv = np.full(len(mi), NO_MOVE, np.int64)
        np.minimum.at(mv, ci[hit], csq[hit])
        sel = csq == mv[ci]
        assert (ci[sel] == np.arange(len(mi))).all()
        b[mi] = cb[sel]
        t[mi] = 3 - t[mi]
        rem[mi] -= 1
        line[mi, length[mi]] = mv
        length[mi] += 1
    best_move = np.where(length > 0, line[:, 0], NO_MOVE).astype(np.int64)
    return dict(line=line, length=length, best_move=best_move, end_boards=b, end_turn=t.astype(np.int64))


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def exact(boards, turn):
    """The exact line of every position (at most 9 empties or so: the checker expands whole trees)."""
    out = _walk(boards, turn, np.full(len(turn), UNBOUNDED), lambda cb, ct, root, rem: solve_ref.solve(cb, ct)[0])
    out["value"] = solve_ref.solve(boards, turn)[0].astype(np.int64)
    return _frozen(out)


def search(boards, turn, depth, weights):
    """The search line at `depth` (an int or an array of n, each >= 1)."""
    t = mover(turn)
    d = np.broadcast_to(np.asarray(depth, np.int64), (len(t),)).copy()
    out = _walk(boards, turn, d, lambda cb, ct, root, rem: moves_ref.search_rooted(cb, ct, root, rem, weights))
    out["value"] = moves_ref.search_rooted(boards, t, t, d, weights).astype(np.int64)
    return _frozen(out)


def end_score(end_boards, root, weights=None):
    """The static score of end positions from the side `root`: the disc difference (weights None), else
    othello_search.h's rule 1 or 2."""
    b = np.ascontiguousarray(end_boards, np.uint64).reshape(-1, 2)
    root = mover(root)
    diff = oracle.result(b)["diff"].astype(np.int64) * np.where(root == 1, 1, -1)
    if weights is None:
        return diff
    over = (oracle.legal(b, root) == 0) & (oracle.legal(b, (3 - root).astype(np.uint8)) == 0)
    return np.where(over, T * diff, oracle.evaluate(b, root, weights).astype(np.int64))


@functools.lru_cache(maxsize=None)
def exact_inputs(lo, hi):
    """(boards, turn) of every position of solve_cases.cases() at lo..hi empties, read-only."""
    cs = solve_cases.cases()
    b = np.concatenate([cs[e]["boards"] for e in range(lo, hi + 1)])
    t = np.concatenate([cs[e]["turn"] for e in range(lo, hi + 1)])
    b.setflags(write=False)
    t.setflags(write=False)
    return b, t


@functools.lru_cache(maxsize=None)
def exact_cases(lo, hi):
    """exact() of exact_inputs(lo, hi)."""
    return exact(*exact_inputs(lo, hi))


@functools.lru_cache(maxsize=None)
def search_case(name, depth, table):
    """search() of tree_cases.inputs(name) at `depth` with a table of tree_cases.TABLES."""
    b, t = tree_cases.inputs(name)
    return search(b, t, depth, tree_cases.TABLES[table])


def _pin():
    """The first move and the value against solve_ref.solve and search_ref.search."""
    cs = solve_cases.cases()
    for e in (2, 5):
        b, t = cs[e]["boards"][:24], cs[e]["turn"][:24]
        r = exact(b, t)
        assert (r["value"] == cs[e]["value"][:24]).all() and (r["best_move"] == cs[e]["best_move"][:24]).all(), e
    for name, k in (("mid3", 6), ("special3", 16)):
        b, t = tree_cases.inputs(name)
        b, t = b[:k], t[:k]
        for depth, w in ((1, tree_cases.TABLES["default"]), (2, tree_cases.TABLES["rng7"])):
            r = search(b, t, depth, w)
            v, m, _ = search_ref.search(b, t, depth, w)
            assert (r["value"] == v).all() and (r["best_move"] == m).all(), (name, depth)


_pin()
