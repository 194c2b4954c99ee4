"""Positions for the solver tests, cut from one seeded random rollout and
classified with the C oracle (computed once per process, never changed).

pool():  every recorded position of rollout(2048, seed=0x501E), grouped by its
         number of empty squares.
cases(): for each E in 0..9 all forced-pass and game-over roots of that E plus
         the first 256 others (E <= 6), 64 (E = 7, 8) or 32 (E = 9), with the
         exhaustive checker's value and best move.
"""
import functools

import numpy as np

import oracle
import solve_ref

POOL_GAMES, POOL_SEED = 2048, 0x501E
OTHERS = {0: 256, 1: 256, 2: 256, 3: 256, 4: 256, 5: 256, 6: 256, 7: 64, 8: 64, 9: 32}


@functools.lru_cache(maxsize=None)
def pool():
    """dict E -> dict(boards (k,2) u64, turn (k,) u8, forced_pass (k,) bool, over (k,) bool), in game / ply order."""
    g = oracle.rollout(POOL_GAMES, POOL_SEED, record_moves=True)
    rp = oracle.replay(g["moves"], g["plies"])
    keep = np.arange(rp["boards"].shape[1])[None, :] <= g["plies"].astype(np.int64)[:, None]
    boards = np.ascontiguousarray(rp["boards"][keep])
    turn = np.ascontiguousarray(rp["turn"][keep])
    emp = solve_ref.empties(boards)
    own = oracle.legal(boards, turn)
    opp = oracle.legal(boards, (3 - turn).astype(np.uint8))
    out = {}
    for e in range(0, 61):
        sel = emp == e
        if sel.any():
            d = dict(boards=boards[sel], turn=turn[sel], forced_pass=(own[sel] == 0) & (opp[sel] != 0),
                     over=(own[sel] == 0) & (opp[sel] == 0))
            for v in d.values():
                v.setflags(write=False)
            out[e] = d
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """dict E (0..9) -> dict(boards, turn, forced_pass, over, value, best_move, inner_passes)."""
    out = {}
    for e, others in OTHERS.items():
        p = pool()[e]
        special = p["forced_pass"] | p["over"]
        idx = np.concatenate([np.nonzero(special)[0], np.nonzero(~special)[0][:others]])
        d = {k: np.ascontiguousarray(v[idx]) for k, v in p.items()}
        d["value"], d["best_move"], d["inner_passes"] = solve_ref.solve(d["boards"], d["turn"])
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[e] = d
    return out


def ladder(e, k):
    """The first k positions of the pool at e empties where the mover has a move."""
    p = pool()[e]
    idx = np.nonzero(~(p["forced_pass"] | p["over"]))[0][:k]
    return np.ascontiguousarray(p["boards"][idx]), np.ascontiguousarray(p["turn"][idx])
