"""The endgame solver's checker: an exhaustive minimax over the C oracle's
legal / step / result, expanded level by level in numpy, with no pruning and
no knowledge of the code under test.

    V(pos, mover) = max over the mover's legal moves of -V(child, opponent)
                  = -V(pos, opponent)          the mover must pass, the opponent can move
                  = discs(mover) - discs(opponent)   neither can move

best move = the lowest square among the maximisers, 64 for a forced pass, 255
when the game is over.  Cost: the whole tree, so at most 9 empties or so.
"""
import numpy as np

import oracle

PASS, NO_MOVE = 64, 255


def mover(turn):
    """The solver's rule for `turn`: White if 2, else Black."""
    return np.where(np.asarray(turn, np.uint8) == 2, 2, 1).astype(np.uint8)


def empties(boards):
    b = np.ascontiguousarray(boards, np.uint64)
    occ = b[:, 0] | b[:, 1]
    return np.array([64 - bin(int(v)).count("1") for v in occ], np.int64)


def _bits(mask):
    """(index into mask, square) of every set bit, ordered by index then square."""
    idx, sq = [], []
    for s in range(64):
        hit = np.nonzero((mask >> np.uint64(s)) & np.uint64(1))[0]
        idx.append(hit)
        sq.append(np.full(len(hit), s, np.uint8))
    idx, sq = np.concatenate(idx), np.concatenate(sq)
    order = np.lexsort((sq, idx))
    return idx[order], sq[order]


def solve(boards, turn):
    """(value int8[n], best_move uint8[n], inner_passes): inner_passes counts the
    pass nodes below the roots."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = mover(turn)
    levels = []  # per level: dict(parent, move, kind, value)
    parent = np.arange(len(b))
    move = np.full(len(b), NO_MOVE, np.uint8)
    inner_passes = 0
    while len(b):
        own = oracle.legal(b, t)
        opp = oracle.legal(b, (3 - t).astype(np.uint8))
        r = oracle.result(b)
        diff = r["diff"].astype(np.int64) * np.where(t == 1, 1, -1)
        can = own != 0
        passes = ~can & (opp != 0)
        over = ~can & (opp == 0)
        lv = dict(parent=parent, move=move, over=over, passes=passes, diff=diff, n=len(b))
        levels.append(lv)
        if len(levels) > 1:
            inner_passes += int(passes.sum())
        # children: one per legal move, one (the same board, the other side) per pass
        ci, csq = _bits(np.where(can, own, np.uint64(0)))
        st = oracle.step(b[ci], t[ci], csq)
        assert (st["ret"] >= 1).all()
        pi = np.nonzero(passes)[0]
        nb = np.concatenate([st["boards"], b[pi]])
        nt = np.concatenate([3 - t[ci], 3 - t[pi]]).astype(np.uint8)
        parent = np.concatenate([ci, pi])
        move = np.concatenate([csq, np.full(len(pi), PASS, np.uint8)])
        b, t = nb, nt
    # back up
    child_val = child_parent = child_move = None
    for lv in reversed(levels):
        val = np.where(lv["over"], lv["diff"], -99).astype(np.int64)
        best = np.full(lv["n"], NO_MOVE, np.int64)
        if child_val is not None and len(child_val):
            score = -child_val
            np.maximum.at(val, child_parent, score)
            hit = score == val[child_parent]
            np.minimum.at(best, child_parent[hit], child_move[hit].astype(np.int64))
        assert (val >= -64).all() and (val <= 64).all()
        child_val, child_parent, child_move = val, lv["parent"], lv["move"]
        value, best_move = val, best
    if not levels:
        return np.zeros(0, np.int8), np.zeros(0, np.uint8), 0
    return value.astype(np.int8), best_move.astype(np.uint8), inner_passes
