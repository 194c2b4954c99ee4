"""Inputs of perft's comparisons with the checker (tests/perft_ref.py), shared by
tests/test_perft_host.py and tests/test_gpu_perft.py: each set and each
reference is computed once per process and left unchanged.

    small     tree_cases' 64 midgame roots and every forced-pass and game-over root at 3..9 empties, with one
              overlapping board at the end; depths 0..4
    endgames  32 roots of solve_cases at each of 1..6 empties (the specials first); depth 8: every game ends
              inside the depth and the passes cost plies
    offtree   16 roots each of synthetic_cases' uniform(20/40/52), lopsided(8), islands(6) and the 8 of wide(8);
              depth 3
    mixed     `small` with depths 0..4 cycling over the positions, in one call
"""
import functools

import numpy as np

import perft_ref
import solve_cases
import synthetic_cases
import tree_cases

DEPTHS = {"small": (0, 1, 2, 3, 4), "endgames": (8,), "offtree": (3,)}
OVERLAP = (np.array([[3, 1]], np.uint64), np.array([1], np.uint8))


def _freeze(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(boards, turn) of a set, read-only."""
    if name == "small":
        parts = [tree_cases.inputs("mid3"), tree_cases.inputs("special3"), OVERLAP]
    elif name == "endgames":
        cs = solve_cases.cases()
        parts = [(cs[e]["boards"][:32], cs[e]["turn"][:32]) for e in range(1, 7)]
    else:
        parts = [(b[:16], t[:16]) for b, t in (synthetic_cases.uniform(20), synthetic_cases.uniform(40),
                                               synthetic_cases.uniform(52), synthetic_cases.lopsided(8),
                                               synthetic_cases.islands(6), synthetic_cases.wide(8))]
    return _freeze(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


@functools.lru_cache(maxsize=None)
def reference(name, depth):
    """The checker's (leaves, divide, status) of a set at a depth."""
    b, t = inputs(name)
    return _freeze(*perft_ref.perft(b, t, depth))


@functools.lru_cache(maxsize=None)
def mixed():
    """(boards, turn, depths uint8, (leaves, divide, status)): `small`, position i at depth i % 5."""
    b, t = inputs("small")
    d = (np.arange(len(t)) % 5).astype(np.uint8)
    refs = [reference("small", k) for k in range(5)]
    pick = lambda j: np.stack([refs[k][j] for k in range(5)])[d, np.arange(len(t))]  # noqa: E731
    return _freeze(b, t, d) + (_freeze(pick(0), pick(1), pick(2)),)


def same(got, want, what):
    """leaves, divide and status of ``got`` (anything indexable by those names) are the reference's."""
    for k, w in zip(("leaves", "divide", "status"), want):
        g = np.asarray(got[k], np.int64).reshape(np.shape(w))
        bad = np.argwhere(g != np.asarray(w, np.int64))
        assert len(bad) == 0, (what, k, bad[:6].tolist(), g[tuple(bad[0])], np.asarray(w)[tuple(bad[0])])
