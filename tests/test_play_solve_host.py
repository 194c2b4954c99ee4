"""Search self-play with the exact solver's endgame on the host
(tools/diag/play_solve_host.cpp: both phases of play_solve.hip in plain C++
over play_core.hpp, budget_core.hpp, solve_core.hpp and play_solve_core.hpp)
against tests/play_ref.py's game loop with a chooser that is search_ref's
exhaustive search above the zone and solve_ref's exhaustive minimax inside it.
DESIGN.md §25.

Per E in {1, 5, 8, 9}: 24 games at depths (2, 1), random budgets (1, 2), the
colour swap on, from starts two empties above the zone and on its edge, one
start already over, one forced pass where the zone begins and one overlapping
board.  Both orders and a run by budget give the same games; so does the build
under -fsanitize=address,undefined, byte for byte, as a process of its own.
CPU only."""
import functools

import numpy as np
import pytest

import host_programs as hp
import play_ref
import play_solve_cases as cases
import tree_cases

WA, WB = tree_cases.TABLES["default"], tree_cases.TABLES["rng7"]
ZONES = (1, 5, 8, 9)
DEPTHS, N_RAND, SEED = (2, 1), (1, 2), 4242


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return cases.compiled(tmp_path_factory)


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return cases.compiled(tmp_path_factory, hp.SANITIZED)


def arguments(e):
    b, t = cases.starts(e)
    return dict(n=len(t), seed=SEED + e, depths=DEPTHS, budgets=(0, 0), solve_empties=e, n_rand=N_RAND, swap=True,
                limit=0, start=b, start_turn=t, wa=WA, wb=WB)


@functools.lru_cache(maxsize=None)
def reference(e):
    b, t = cases.starts(e)
    r = play_ref.play(len(t), SEED + e, cases.chooser(WA, WB, DEPTHS[0], DEPTHS[1], e), n_rand_a=N_RAND[0],
                      n_rand_b=N_RAND[1], swap=True, start=b, start_turn=t)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("e", ZONES)
def test_host_games_are_the_checkers(binary, tmp_path, e):
    kw = arguments(e)
    assert 16 <= kw["n"] <= 32
    want = reference(e)
    got = cases.run_host(binary, tmp_path, 0, **kw)
    cases.assert_same(got, want, ("fixed", e))
    # the list held the games that reached the zone alive: all but the overlapping board, at least
    assert got["parked"] >= 10 and got["parked"] <= kw["n"] - 1
    assert (got["status"][:-1] == play_ref.SEARCHED).all() and got["status"][-1] == play_ref.INVALID
    assert got["plies"][-3] == 0 and (got["moves"][-3] == 255).all()  # the start already over
    assert got["moves"][-2][0] == play_ref.PASS  # the forced pass
    # the other order and a run by budget whose budgets reach the caps: the same games
    cases.assert_same(cases.run_host(binary, tmp_path, 1, **kw), want, ("ordered", e))
    kw["budgets"] = (1 << 20, 1 << 20)
    for order in (0, 1):
        cases.assert_same(cases.run_host(binary, tmp_path, order, **kw), want, ("by budget", order, e))


def test_a_small_budget_plays_the_budget_games_above_the_zone(binary, tmp_path):
    """By budget the moves above the zone are the deepening's, not the caps': with budgets of a few nodes and
    caps of 6 some game differs from the fixed-depth one, and every game still ends SEARCHED with the zone's
    plies the solver's (the final difference is the solver's value where the game came in: checked on the GPU
    against ops.solve, tests/test_gpu_play_solve.py)."""
    kw = arguments(8)
    kw["depths"] = (6, 6)
    deep = cases.run_host(binary, tmp_path, 0, **kw)
    kw["budgets"] = (8, 30)
    small = cases.run_host(binary, tmp_path, 0, **kw)
    assert (small["status"][:-1] == play_ref.SEARCHED).all()
    assert (small["moves"] != deep["moves"]).any()


def test_node_limit_stops_a_game_where_its_solve_would_pass_it(binary, tmp_path):
    kw = arguments(9)
    kw["limit"] = 1
    got = cases.run_host(binary, tmp_path, 0, **kw)
    full = reference(9)
    lim = got["status"] == play_ref.LIMIT
    assert lim.any() and (got["status"][~lim] != play_ref.LIMIT).all()
    for g in np.nonzero(lim)[0]:
        p = int(got["plies"][g])
        assert (got["moves"][g][:p] == full["moves"][g][:p]).all() and (got["moves"][g][p:] == 255).all()


@pytest.mark.parametrize("e", (5, 9))
def test_the_same_bytes_under_the_address_and_undefined_behaviour_sanitizers(binary, binary_asan, tmp_path, e):
    kw = arguments(e)
    for order, budgets in ((0, (0, 0)), (1, (0, 0)), (0, (40, 300))):
        kw["budgets"] = budgets
        plain = cases.run_host(binary, tmp_path, order, raw=True, **kw)
        san = cases.run_host(binary_asan, tmp_path, order, raw=True, **kw)
        assert plain["raw"] == san["raw"] and len(plain["raw"]) > 0, (order, budgets)
