"""The depth-limited search's checker: an exhaustive, unpruned minimax of
include/othello_search.h's four rules over the C oracle's legal / step /
result / evaluate, expanded level by level in numpy, with no knowledge of the
code under test.

For side to move s with d plies left and root mover r, the first that applies:
    1. neither side can move:  T * (discs(s) - discs(opponent)),  T = 2**17
    2. d == 0:                 +evaluate(pos, r, W) if s == r else -evaluate(pos, r, W)
    3. s must pass:            -S(pos, opponent, d)        (no depth spent)
    4. otherwise:              max over s's moves of -S(child, opponent, d - 1)

best move = the lowest square among the maximisers, 64 for a forced pass at the
root, 255 when the game is over at the root.  Cost: the whole tree to depth d.
"""
import numpy as np

import oracle
from solve_ref import _bits, mover

T = 1 << 17
PASS, NO_MOVE = 64, 255
WEIGHTS_B = np.random.default_rng(7).integers(-128, 128, (4, 9)).astype(np.int8)
WEIGHTS_B.setflags(write=False)


def search(boards, turn, depth, weights):
    """(value int32[n], best_move uint8[n], nodes_expanded)."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    n = len(b)
    t = mover(turn)
    root = t.copy()  # each node's root mover
    d = np.full(n, depth, np.int64)
    parent = np.arange(n)
    move = np.full(n, NO_MOVE, np.uint8)
    levels = []
    expanded = 0
    while len(b):
        own = oracle.legal(b, t)
        opp = oracle.legal(b, (3 - t).astype(np.uint8))
        diff = oracle.result(b)["diff"].astype(np.int64) * np.where(t == 1, 1, -1)
        ev = oracle.evaluate(b, root, weights).astype(np.int64) * np.where(t == root, 1, -1)
        over = (own == 0) & (opp == 0)                 # rule 1
        leaf = ~over & (d == 0)                        # rule 2
        passes = ~over & ~leaf & (own == 0)            # rule 3
        inner = ~over & ~leaf & (own != 0)             # rule 4
        static = np.where(over, T * diff, np.where(leaf, ev, 0))
        levels.append(dict(parent=parent, move=move, final=over | leaf, static=static, n=len(b)))
        expanded += len(b)
        ci, csq = _bits(np.where(inner, own, np.uint64(0)))
        st = oracle.step(b[ci], t[ci], csq)
        assert (st["ret"] >= 1).all()
        pi = np.nonzero(passes)[0]
        nb = np.concatenate([st["boards"], b[pi]])
        nt = np.concatenate([3 - t[ci], 3 - t[pi]]).astype(np.uint8)
        nroot = np.concatenate([root[ci], root[pi]])
        nd = np.concatenate([d[ci] - 1, d[pi]])
        parent = np.concatenate([ci, pi])
        move = np.concatenate([csq, np.full(len(pi), PASS, np.uint8)])
        b, t, root, d = nb, nt, nroot, nd
    lo = -(1 << 40)
    child_val = child_parent = child_move = None
    value, best_move = np.zeros(0, np.int64), np.zeros(0, np.int64)
    for lv in reversed(levels):
        val = np.where(lv["final"], lv["static"], lo).astype(np.int64)
        best = np.full(lv["n"], NO_MOVE, np.int64)
        if child_val is not None and len(child_val):
            score = -child_val
            np.maximum.at(val, child_parent, score)
            hit = score == val[child_parent]
            np.minimum.at(best, child_parent[hit], child_move[hit].astype(np.int64))
        assert (val > lo).all()
        child_val, child_parent, child_move = val, lv["parent"], lv["move"]
        value, best_move = val, best
    assert (np.abs(value) <= 64 * T).all()
    return value.astype(np.int32), best_move.astype(np.uint8), expanded
