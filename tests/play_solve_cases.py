"""What the tests of the search self-play with the exact solver's endgame
(include/othello_play_solve.h) share: the checker's chooser, the starts, and the
host build's files (tools/diag/play_solve_host.cpp)."""
import numpy as np

import host_programs as hp
import play_ref
import search_ref
import solve_cases
import solve_ref

KEYS = ("a_black", "final_boards", "diff", "plies", "moves", "status")


def chooser(weights_a, weights_b, depth_a, depth_b, solve_empties, solver=None):
    """The rule's policy move: search_ref.search's at the mover's depth above
    ``solve_empties`` empty squares, the solver's at or below it.  ``solver``
    (boards, turn) -> best moves; default: solve_ref's exhaustive minimax."""
    above = play_ref.search_chooser(weights_a, weights_b, depth_a, depth_b)
    solver = solver or (lambda b, t: solve_ref.solve(b, t)[1])

    def choose(boards, turn, player):
        late = solve_ref.empties(boards) <= solve_empties
        out = np.full(len(turn), 255, np.uint8)
        if (~late).any():
            out[~late] = above(boards[~late], turn[~late], player[~late])
        if late.any():
            out[late] = solver(boards[late], turn[late])
        return out
    return choose


def flagged(flag, e_max):
    """The first position of solve_cases.pool() with ``flag`` ("over", "forced_pass") set, from e_max empty
    squares downwards."""
    for e in range(e_max, -1, -1):
        p = solve_cases.pool().get(e)
        if p is not None and p[flag].any():
            i = int(np.nonzero(p[flag])[0][0])
            return p["boards"][i], p["turn"][i]
    raise AssertionError("no %s position at <= %d empties" % (flag, e_max))


def starts(solve_empties, above=11, inside=10):
    """(boards, turn): `above` starts two empties above the zone, `inside` starts on its edge, then a start
    already over, a forced pass at (or inside) the zone's edge, and an overlapping board."""
    parts = [solve_cases.ladder(solve_empties + 2, above), solve_cases.ladder(solve_empties, inside)]
    for flag in ("over", "forced_pass"):
        b, t = flagged(flag, solve_empties)
        parts.append((b[None, :], np.array([t], np.uint8)))
    parts.append((np.array([[3, 1]], np.uint64), np.array([1], np.uint8)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def compiled(tmp_path_factory, flags=hp.PLAIN):
    return hp.compiled(tmp_path_factory, "play_solve_host", flags)


def run_host(exe, tmp, order, n, seed, depths, budgets, solve_empties, n_rand, swap, limit, start, start_turn, wa, wb,
             raw=False):
    """The host build's games as a dict of arrays (with raw: the output file's bytes as well)."""
    args, out = str(tmp / "xargs"), str(tmp / "xout")
    hp.write_game_args(args, n, seed, depths, solve_empties, n_rand, swap, limit, wa, wb, start, start_turn, budgets)
    r = hp.run([exe, args, out, order, 8])
    got = dict(hp.read_games(out), parked=int(r.stderr.split()[1]))
    if raw:
        got["raw"] = open(out, "rb").read()
    return got


def assert_same(got, want, what, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
        assert len(bad) == 0, (what, k, bad[:8], a[bad[:4]], b[bad[:4]])
