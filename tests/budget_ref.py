"""The budget search's checker: include/othello_budget.h's rule as a plain loop
over a callable ``search_at(d) -> (value, best_move, status, nodes)`` that runs
the FIXED-DEPTH search of the whole batch at depth d and knows nothing of the
code under test.

    K = min(cap, max(1, empties));  rem = B
    for d = 1..K:  iteration d completes iff its search needs n_d <= rem nodes;
                   then (value, move, d) are recorded and rem -= n_d; the loop
                   ends at the first that does not complete, or when rem == 0.

The callable may run its searches under any node limit L >= the largest budget:
a completed search's n_d does not depend on the limit, and a search that ends as
LIMIT there needed more than L >= rem nodes.  So completion is decided HERE by
n_d <= rem, and every reference search stays bounded by L nodes a position.

A budget of 0 is outside the rule (B >= 1): the calls end such a position as
LIMIT with nothing searched.  Overlapping boards are INVALID whatever the budget.
"""
import numpy as np

SEARCHED, INVALID, LIMIT = 1, 2, 3
NO_MOVE = 255


def empties(boards):
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    occ = b[:, 0] | b[:, 1]
    return 64 - np.unpackbits(occ.view(np.uint8).reshape(len(occ), 8), axis=1).sum(1).astype(np.int64)


def deepen(search_at, boards, budgets, cap):
    """dict(value int32, best_move uint8, status uint8, depth uint8, nodes
    int64, counts) of the rule; ``budgets`` an int or n of them.  ``counts[d]``
    is search_at(d)'s node column for every depth asked (a diagnostic)."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    n = len(b)
    rem = np.broadcast_to(np.asarray(budgets, np.int64), (n,)).copy()
    last = np.minimum(cap, np.maximum(1, empties(b)))
    invalid = (b[:, 0] & b[:, 1]) != 0
    value = np.zeros(n, np.int32)
    move = np.full(n, NO_MOVE, np.uint8)
    depth = np.zeros(n, np.uint8)
    nodes = np.zeros(n, np.int64)
    alive = ~invalid & (rem > 0)
    counts = {}
    for d in range(1, cap + 1):
        run = alive & (d <= last)
        if not run.any():
            break
        v, m, st, nd = (np.asarray(x) for x in search_at(d))
        nd = nd.astype(np.int64) & 0xFFFFFFFF
        counts[d] = nd
        assert ((st == INVALID) == invalid).all()
        done = run & (st == SEARCHED) & (nd <= rem)
        value[done], move[done], depth[done] = v[done], m[done], d
        nodes[done] += nd[done]
        rem[done] -= nd[done]
        alive = done & (rem > 0)
    status = np.where(invalid, INVALID, np.where(depth > 0, SEARCHED, LIMIT)).astype(np.uint8)
    return dict(value=value, best_move=move, status=status, depth=depth, nodes=nodes, counts=counts)
