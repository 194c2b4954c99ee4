"""Expected answers of the per-move calls (include/othello_moves.h, DESIGN.md
§21), with no knowledge of the code under test.

Exact rows: window_ref.roots' exhaustive value of every root move (ci, csq,
cval), scattered into (n, 64) rows.

Search rows: search_ref.search's level-by-level minimax of othello_search.h's
four rules with the ROOT MOVER PASSED IN instead of taken from `turn`
(:func:`search_rooted`), applied to the oracle's children with root = the
parent's mover and d = depth - 1, or to the same board with the opponent to move
at d = depth for a forced pass.  The assertion at the bottom pins it to
search_ref.search: the max and the lowest argmax of its rows are that
checker's value and move on the same roots.
"""
import functools

import numpy as np

import oracle
import search_ref
import solve_cases
import tree_cases
import window_ref
from solve_ref import _bits, mover

T = search_ref.T
PASS, NO_MOVE = 64, 255
NOT_A_MOVE, UNKNOWN = -128, -127
NOT_A_MOVE32, UNKNOWN32 = -2**31, -2**31 + 1


def rows_of(n, ci, csq, cval, fill):
    rows = np.full((n, 64), fill, np.int64)
    rows[ci, csq] = cval
    return rows


def exact(r):
    """(rows (n, 64), value, move) of window_ref.Roots r."""
    value, move = window_ref.expect(r, window_ref.LO, window_ref.HI)
    return rows_of(r.n, r.ci, r.csq, r.cval, NOT_A_MOVE), value, move


@functools.lru_cache(maxsize=None)
def exact_cases(lo, hi):
    """Every position of solve_cases.cases() at lo..hi empties as one batch:
    (boards, turn, rows, value, move, forced_pass, over), read-only."""
    cs = solve_cases.cases()
    parts = [(cs[e]["boards"], cs[e]["turn"]) + exact(window_ref.case_roots(e)) +
             (cs[e]["forced_pass"], cs[e]["over"]) for e in range(lo, hi + 1)]
    out = tuple(np.concatenate([p[k] for p in parts]) for k in range(7))
    for v in out:
        v.setflags(write=False)
    return out


def search_rooted(boards, turn, root, d, weights):
    """S(pos, turn, d) with root mover `root` (arrays of n; d >= 0), from the
    side to move: search_ref.search's expansion, the root passed in."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = mover(turn)
    root = np.asarray(root, np.uint8).copy()
    d = np.asarray(d, np.int64).copy()
    parent = np.arange(len(b))
    levels = []
    while len(b):
        own = oracle.legal(b, t)
        opp = oracle.legal(b, (3 - t).astype(np.uint8))
        diff = oracle.result(b)["diff"].astype(np.int64) * np.where(t == 1, 1, -1)
        ev = oracle.evaluate(b, root, weights).astype(np.int64) * np.where(t == root, 1, -1)
        over = (own == 0) & (opp == 0)                 # rule 1
        leaf = ~over & (d == 0)                        # rule 2
        passes = ~over & ~leaf & (own == 0)            # rule 3
        inner = ~over & ~leaf & (own != 0)             # rule 4
        levels.append(dict(parent=parent, final=over | leaf, static=np.where(over, T * diff, np.where(leaf, ev, 0)),
                           n=len(b)))
        ci, csq = _bits(np.where(inner, own, np.uint64(0)))
        st = oracle.step(b[ci], t[ci], csq)
        assert (st["ret"] >= 1).all()
        pi = np.nonzero(passes)[0]
        b, t, root, d, parent = (np.concatenate([st["boards"], b[pi]]),
                                 np.concatenate([3 - t[ci], 3 - t[pi]]).astype(np.uint8),
                                 np.concatenate([root[ci], root[pi]]), np.concatenate([d[ci] - 1, d[pi]]),
                                 np.concatenate([ci, pi]))
    lo = -(1 << 40)
    child_val = child_parent = None
    val = np.zeros(0, np.int64)
    for lv in reversed(levels):
        val = np.where(lv["final"], lv["static"], lo).astype(np.int64)
        if child_val is not None and len(child_val):
            np.maximum.at(val, child_parent, -child_val)
        assert (val > lo).all()
        child_val, child_parent = val, lv["parent"]
    return val


def children(boards, turn):
    """The oracle's children of every root: (ci, csq, child boards, child turn,
    forced_pass, over)."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = mover(turn)
    own = oracle.legal(b, t)
    opp = oracle.legal(b, (3 - t).astype(np.uint8))
    ci, csq = _bits(own)
    st = oracle.step(b[ci], t[ci], csq)
    assert (st["ret"] >= 1).all()
    return ci, csq.astype(np.int64), st["boards"], (3 - t[ci]).astype(np.uint8), (own == 0) & (opp != 0), \
        (own == 0) & (opp == 0)


def search(boards, turn, depth, weights):
    """(rows (n, 64), value, move) of otha_search_moves at `depth`."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = mover(turn)
    n = len(b)
    ci, csq, cb, ct, forced, over = children(b, t)
    cval = -search_rooted(cb, ct, t[ci], np.full(len(ci), depth - 1), weights)
    rows = rows_of(n, ci, csq, cval, NOT_A_MOVE32)
    value = np.zeros(n, np.int64)
    move = np.full(n, NO_MOVE, np.int64)
    has = ~forced & ~over
    value[has] = rows[has].max(axis=1)
    move[has] = (rows[has] == value[has, None]).argmax(axis=1)
    pi = np.nonzero(forced)[0]
    value[pi] = -search_rooted(b[pi], (3 - t[pi]).astype(np.uint8), t[pi], np.full(len(pi), depth), weights)
    move[pi] = PASS
    oi = np.nonzero(over)[0]
    value[oi] = T * oracle.result(b[oi])["diff"].astype(np.int64) * np.where(t[oi] == 1, 1, -1)
    return rows, value, move


@functools.lru_cache(maxsize=None)
def search_case(name, depth, table):
    """search() of tree_cases.inputs(name) at `depth` with a table of tree_cases.TABLES, read-only."""
    b, t = tree_cases.inputs(name)
    out = search(b, t, depth, tree_cases.TABLES[table])
    for v in out:
        v.setflags(write=False)
    return out


def hint_lines(row, fill):
    """The engine's `hint` order of one row: (square, value) best first, lowest square first among equals."""
    sq = np.nonzero(np.asarray(row) != fill)[0]
    return sorted(((int(s), int(row[s])) for s in sq), key=lambda x: (-x[1], x[0]))


def _pin():
    """search() against search_ref.search: midgame roots and the pass / finished roots, both tables."""
    for name, k in (("mid3", 8), ("special3", 24)):
        b, t = tree_cases.inputs(name)
        b, t = b[:k], t[:k]
        for depth, w in ((1, tree_cases.TABLES["default"]), (2, tree_cases.TABLES["rng7"])):
            rows, value, move = search(b, t, depth, w)
            v, m, _ = search_ref.search(b, t, depth, w)
            assert (value == v).all() and (move == m).all(), (name, depth)


_pin()
