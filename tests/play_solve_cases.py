"""What the tests of the search self-play with the exact solver's endgame
(include/othello_play_solve.h) share: the checker's chooser, the starts, and the
host build's files (tools/diag/play_solve_host.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import play_ref
import search_ref
import solve_cases
import solve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "diag", "play_solve_host.cpp")
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


def compiled(tmp_path_factory, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, SOURCE])
    return exe


def run_host(exe, tmp, order, n, seed, depths, budgets, solve_empties, n_rand, swap, limit, start, start_turn, wa, wb,
             raw=False):
    """The host build's games as a dict of arrays (with raw: the output file's bytes as well)."""
    args, out = str(tmp / "xargs"), str(tmp / "xout")
    with open(args, "w") as f:
        f.write("%d %d 0 %d %d %d %d %d %d %d %d %d %d\n" % (n, seed, depths[0], depths[1], budgets[0], budgets[1],
                                                             solve_empties, n_rand[0], n_rand[1], int(swap), limit,
                                                             int(start is not None)))
        for w in (wa, wb):
            f.write(" ".join(str(int(x)) for x in np.asarray(w).reshape(-1)) + "\n")
        if start is not None:
            for (bl, wh), t in zip(np.asarray(start, np.uint64).tolist(), np.asarray(start_turn).tolist()):
                f.write("%x %x %d\n" % (bl, wh, t))
    r = subprocess.run([exe, args, out, str(order), "8"], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    rows = [ln.split() for ln in open(out)]
    got = dict(a_black=np.array([int(r[0]) for r in rows]),
               final_boards=np.array([[int(r[1], 16), int(r[2], 16)] for r in rows], np.uint64).reshape(-1, 2),
               diff=np.array([int(r[3]) for r in rows]), plies=np.array([int(r[4]) for r in rows]),
               status=np.array([int(r[5]) for r in rows]), nodes=np.array([int(r[6]) for r in rows]),
               moves=np.array([list(bytes.fromhex(r[7])) for r in rows], np.uint8).reshape(-1, 128),
               parked=int(r.stderr.split()[1]))
    if raw:
        got["raw"] = open(out, "rb").read()
    return got


def assert_same(got, want, what, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
        assert len(bad) == 0, (what, k, bad[:8], a[bad[:4]], b[bad[:4]])
