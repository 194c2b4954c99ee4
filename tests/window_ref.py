"""Expected answers of the exact solvers under a root window,
from the exhaustive checker alone: a root's V and the exhaustive value of every
root move (solve_ref.solve over oracle.step's children), then

    value = clamp(V, alpha, beta)
    move  = 64 for a forced pass, 255 for a finished game, else
            alpha < V < beta: the lowest square among the maximisers
            V >= beta:        the lowest square among the moves whose value is >= beta
            V <= alpha:       255 (no move is proved)

No knowledge of the code under test.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle
import solve_cases
import solve_ref

PASS, NO_MOVE = 64, 255
LO, HI = -65, 65
FAMILIES = ("full", "wld", "around", "on_alpha", "on_beta", "below", "above", "top", "bottom")
# the two with V on a bound: a wrong < or <= shows there
ON_BOUND = ("on_alpha", "on_beta")

# per root: value, has (the mover has a move), forced_pass; per root move (flat, by root then square):
# ci (root index), csq (square), cval (the move's exhaustive value from the root mover's side)
Roots = namedtuple("Roots", "n value has forced_pass ci csq cval")


def roots(boards, turn):
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = solve_ref.mover(turn)
    value, _, _ = solve_ref.solve(b, t)
    own = oracle.legal(b, t)
    opp = oracle.legal(b, (3 - t).astype(np.uint8))
    ci, csq = solve_ref._bits(own)
    if len(ci):
        st = oracle.step(b[ci], t[ci], csq)
        assert (st["ret"] >= 1).all()
        child, _, _ = solve_ref.solve(st["boards"], (3 - t[ci]).astype(np.uint8))
        cval = -child.astype(np.int64)
    else:
        cval = np.zeros(0, np.int64)
    r = Roots(len(b), value.astype(np.int64), own != 0, (own == 0) & (opp != 0), ci, csq.astype(np.int64), cval)
    for v in r[1:]:
        v.setflags(write=False)
    return r


def family(name, v):
    """The window family `name` for the truths v: (alpha, beta, keep); keep is
    False where the clipped window is empty."""
    v = np.asarray(v, np.int64)
    lo, hi = np.full_like(v, LO), np.full_like(v, HI)
    a, b = {"full": (lo, hi), "wld": (lo * 0 - 1, lo * 0 + 1), "around": (v - 1, v + 1), "on_alpha": (v, v + 1),
            "on_beta": (v - 1, v), "below": (lo, v), "above": (v, hi), "top": (lo * 0 + 63, hi),
            "bottom": (lo, lo * 0 - 63)}[name]
    a, b = np.clip(a, LO, HI), np.clip(b, LO, HI)
    return a, b, a < b


def expect(r, alpha, beta):
    """(value, move) of the roots r under the windows (alpha, beta), arrays of r.n."""
    alpha, beta = np.broadcast_to(np.asarray(alpha, np.int64), (r.n,)), np.broadcast_to(np.asarray(beta, np.int64), (r.n,))
    assert ((LO <= alpha) & (alpha < beta) & (beta <= HI)).all()
    value = np.clip(r.value, alpha, beta)
    need = np.where(r.value >= beta, beta, r.value)  # what a move must reach to be the answer
    ok = (r.cval >= need[r.ci]) & (r.value > alpha)[r.ci]
    move = np.full(r.n, NO_MOVE, np.int64)
    np.minimum.at(move, r.ci[ok], r.csq[ok])
    move[r.forced_pass] = PASS
    return value, move


@functools.lru_cache(maxsize=None)
def case_roots(e):
    """roots() of solve_cases.cases()[e], computed once per process."""
    c = solve_cases.cases()[e]
    r = roots(c["boards"], c["turn"])
    # the helper's own full-window answer is the checker's
    v, m = expect(r, LO, HI)
    assert (v == c["value"]).all() and (m == c["best_move"]).all()
    return r


def case_batch(lo, hi, names=FAMILIES):
    """Every position of cases() at lo..hi empties under every family of
    `names`, as one batch: (boards, turn, alpha, beta, value, move, family index)."""
    out = [[] for _ in range(7)]
    for e in range(lo, hi + 1):
        c, r = solve_cases.cases()[e], case_roots(e)
        for k, name in enumerate(FAMILIES):
            if name not in names:
                continue
            a, b, keep = family(name, r.value)
            a, b = np.where(keep, a, LO), np.where(keep, b, HI)
            v, m = expect(r, a, b)
            for dst, src in zip(out, (c["boards"], c["turn"], a, b, v, m, np.full(r.n, k))):
                dst.append(src[keep])
    return tuple(np.concatenate(x) for x in out)
