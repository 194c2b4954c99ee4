"""Perft's checker: include/othello_perft.h's three rules over the C oracle's
legal / step, expanded level by level in numpy, with no knowledge of the code
under test.

    N(pos, s, 0) = 1
    N(pos, s, d) = sum over s's legal moves of N(child, opponent, d - 1)   s has a move
                 = N(pos, opponent, d - 1)                                 s must pass: a pass IS a ply
                 = 1                                                       neither side can move

Every node of the level carries its root and the root move it lies under; a
node that is final (d == 0 or the game over) adds 1 to its root's count and to
that move's column.  Cost: the whole tree, a node per path.

OPENING holds the published values from the opening, Black to move, depths
1..12; they are not this project's.  Depth 9 is the first where "a pass costs
no ply" would differ (3,005,320), depth 10 the first where counting a finished
game as 0 would (24,571,056).
"""
import numpy as np

import oracle
from solve_ref import _bits, mover

OPENING = (4, 12, 56, 244, 1396, 8200, 55092, 390216, 3005288, 24571284, 212258800, 1939886636)
COUNTED, INVALID, LIMIT, BADDEPTH = 1, 2, 3, 7
MAX_DEPTH = 14
NO_COLUMN = 255


def perft(boards, turn, depth):
    """(leaves int64[n], divide int64[n, 64], status uint8[n]); ``depth`` an int or one per position."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    n = len(b)
    t = mover(turn)
    d = np.broadcast_to(np.asarray(depth, np.int64), (n,)).copy()
    leaves, divide = np.zeros(n, np.int64), np.zeros((n, 64), np.int64)
    status = np.where((b[:, 0] & b[:, 1]) != 0, INVALID, np.where(d > MAX_DEPTH, BADDEPTH, COUNTED)).astype(np.uint8)
    keep = np.nonzero(status == COUNTED)[0]
    b, t, d, root = b[keep], t[keep], d[keep], keep
    col = np.full(len(keep), NO_COLUMN, np.int64)  # the root move the node lies under
    first = True
    while len(b):
        own = oracle.legal(b, t)
        opp = oracle.legal(b, (3 - t).astype(np.uint8))
        final = (d == 0) | ((own == 0) & (opp == 0))
        np.add.at(leaves, root[final], 1)
        under = final & (col < 64)
        np.add.at(divide, (root[under], col[under]), 1)
        passes = ~final & (own == 0)
        ci, csq = _bits(np.where(final, np.uint64(0), own))
        st = oracle.step(b[ci], t[ci], csq)
        assert (st["ret"] >= 1).all()
        pi = np.nonzero(passes)[0]
        ccol = np.concatenate([csq.astype(np.int64) if first else col[ci], col[pi]])  # (a root pass has no column)
        b = np.concatenate([st["boards"], b[pi]])
        t = np.concatenate([3 - t[ci], 3 - t[pi]]).astype(np.uint8)
        d = np.concatenate([d[ci] - 1, d[pi] - 1])
        root = np.concatenate([root[ci], root[pi]])
        col = ccol
        first = False
    return leaves, divide, status


def opening():
    b, t, _ = oracle.reset(1)
    return b, t
