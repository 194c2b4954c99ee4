"""The budget searches on the host (tools/diag/budget_host.cpp: budget_core.hpp's
deepening layer in plain C++ around search_core.hpp's, order_core.hpp's and
play_core.hpp's machines) against tests/budget_ref.py's loop over the existing
fixed-depth host build (tools/diag/search_host.cpp) and, at the depth reached,
against tests/search_ref.py's exhaustive minimax.  DESIGN.md §22.

Inputs: the search tests' small sets (midgame roots, every forced-pass and
game-over root at 3..9 empties) and the off-tree boards of
tests/synthetic_cases.py, with an overlapping board; both orders, budgets 1, 8,
64, 512, 4096 and caps 1, 4, 8.  The same under
-fsanitize=address,undefined, as a process of its own.  CPU only."""
import functools

import numpy as np
import pytest

import budget_ref
import host_programs as hp
import play_ref
import search_ref
import synthetic_cases
import tree_cases

BUDGETS = (1, 8, 64, 512, 4096)
CAPS = (1, 4, 8)
BMAX = max(BUDGETS)


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "budget_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "budget_host", hp.SANITIZED)


@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "search_host")


@functools.lru_cache(maxsize=None)
def inputs():
    """(boards, turn), read-only: 64 midgame roots, the forced-pass and game-over roots, off-tree boards of
    20..52 empties, the widest roots, the fixed edge list, 6 and 8 empties off the tree, one overlapping board."""
    parts = [tree_cases.inputs("mid3"), tree_cases.inputs("special3")]
    parts += [(b[:16], t[:16]) for b, t in (synthetic_cases.uniform(20), synthetic_cases.uniform(40),
                                            synthetic_cases.uniform(52), synthetic_cases.lopsided(8),
                                            synthetic_cases.islands(6), synthetic_cases.centre(6))]
    parts += [synthetic_cases.wide(8), synthetic_cases.edges()[:2]]
    parts += [(np.array([[3, 1]], np.uint64), np.array([1], np.uint8))]
    b = np.concatenate([p[0] for p in parts])
    t = np.concatenate([p[1] for p in parts])
    b.setflags(write=False)
    t.setflags(write=False)
    return b, t


def run_budget(exe, tmp, boards, turn, budgets, cap, weights, order):
    inp, out, wf = str(tmp / "bin"), str(tmp / "bout"), str(tmp / "bw")
    budgets = np.broadcast_to(np.asarray(budgets, np.int64), (len(turn),))
    hp.write_positions(inp, boards, turn, budgets)
    hp.write_weights(wf, weights)
    hp.run([exe, "search", inp, out, wf, cap, order, 8])
    a = hp.read_rows(out, (len(turn), 5))
    return dict(value=a[:, 0], best_move=a[:, 1], status=a[:, 2], depth=a[:, 3], nodes=a[:, 4])


def fixed_depth(exe, tmp, boards, turn, weights, order, limit):
    """search_at(d) of the existing host build, each depth run once."""
    inp, wf = str(tmp / "fin"), str(tmp / "fw")
    hp.write_positions(inp, boards, turn)
    hp.write_weights(wf, weights)

    @functools.lru_cache(maxsize=None)
    def search_at(d):
        out = str(tmp / ("fout%d" % d))
        hp.run([exe, inp, out, wf, d, limit, 8, order])
        a = hp.read_rows(out, (len(turn), 4))
        return a[:, 0], a[:, 1], a[:, 2], a[:, 3]

    return search_at


def same(got, want, what):
    for k in ("status", "depth", "nodes", "value", "best_move"):
        bad = np.nonzero(np.asarray(got[k], np.int64) != np.asarray(want[k], np.int64))[0]
        assert len(bad) == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:8]], np.asarray(want[k])[bad[:8]])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("table", tree_cases.BOTH)
def test_budget_host_equals_the_loop_over_the_fixed_depth_host_build(binary, fixed, tmp_path, order, table):
    b, t = inputs()
    w = tree_cases.TABLES[table]
    search_at = fixed_depth(fixed, tmp_path, b, t, w, order, BMAX)
    reached = set()
    for cap in CAPS:
        for budget in BUDGETS:
            want = budget_ref.deepen(search_at, b, budget, cap)
            got = run_budget(binary, tmp_path, b, t, budget, cap, w, order)
            same(got, want, (order, table, cap, budget))
            assert (got["nodes"] <= budget).all() and (got["depth"] <= cap).all()
            reached |= set(got["depth"].tolist())
    assert reached == set(range(9)), reached  # every depth, and the position that completes none
    # per-position budgets, zeros among them, in one run
    budgets = np.array([(0, 1, 8, 64, 512, 4096, 37, 1000)[i % 8] for i in range(len(t))], np.int64)
    want = budget_ref.deepen(search_at, b, budgets, 8)
    got = run_budget(binary, tmp_path, b, t, budgets, 8, w, order)
    same(got, want, "per-position budgets")
    zero = (budgets == 0) & (want["status"] != budget_ref.INVALID)
    assert zero.any() and (got["status"][zero] == budget_ref.LIMIT).all() and (got["best_move"][zero] == 255).all()
    assert (got["status"][-1] == budget_ref.INVALID) and got["nodes"][-1] == 0 and got["depth"][-1] == 0


def test_value_and_move_are_the_exhaustive_checkers_at_the_depth_reached(binary, tmp_path):
    b, t = inputs()
    b, t = b[:-1], t[:-1]  # (the checker takes no overlapping board)
    for order, table, budget in ((0, "default", 512), (1, "rng7", 4096)):
        w = tree_cases.TABLES[table]
        got = run_budget(binary, tmp_path, b, t, budget, 8, w, order)
        assert (got["status"] == budget_ref.SEARCHED).all()
        checked = 0
        for d in sorted(set(got["depth"].tolist())):
            sel = np.nonzero(got["depth"] == d)[0]
            # the checker expands the unpruned tree: every root up to depth 3, a few above, all of those whose
            # whole tree the depth covers
            small = budget_ref.empties(b[sel]) <= 8
            sel = sel if d <= 3 else np.concatenate([sel[small], sel[~small][:4 if d <= 4 else 0]])
            if len(sel) == 0:
                continue
            v, m, _ = search_ref.search(b[sel], t[sel], int(d), w)
            assert (got["value"][sel] == v).all() and (got["best_move"][sel] == m).all(), (order, table, d)
            checked += len(sel)
        assert checked >= len(t) // 2


def run_games(exe, tmp, order, **kw):
    args, out = str(tmp / "gargs"), str(tmp / "gout")
    hp.write_game_args(args, **kw)
    hp.run([exe, "play", args, out, order, 8])
    return hp.read_games(out)


def budget_chooser(fixed, tmp, tables, caps, budgets, exact, order):
    """tests/play_ref.py's chooser for the budget games: the loop over the existing fixed-depth host build on
    the round's positions, one run per depth; without a budget at empties <= exact."""
    def choose(boards, turn, player):
        out = np.full(len(turn), 255, np.uint8)
        emp = budget_ref.empties(boards)
        for p in (0, 1):
            for late in (False, True):
                sel = np.nonzero((player == p) & ((emp <= exact) == late))[0]
                if len(sel) == 0:
                    continue
                search_at = fixed_depth(fixed, tmp, boards[sel], turn[sel], tables[p], order, 1 << 28)
                if late:
                    for d in np.unique(np.maximum(caps[p], emp[sel])):
                        k = np.maximum(caps[p], emp[sel]) == d
                        out[sel[k]] = search_at(int(d))[1][k]
                else:
                    r = budget_ref.deepen(search_at, boards[sel], budgets[p], caps[p])
                    assert (r["status"] == budget_ref.SEARCHED).all()
                    out[sel] = r["best_move"]
        return out
    return choose


@pytest.mark.parametrize("order,exact", [(0, 0), (1, 6)])
def test_budget_games_on_the_host_are_the_game_loops(binary, fixed, tmp_path, order, exact):
    wa, wb = tree_cases.TABLES["default"], tree_cases.TABLES["rng7"]
    caps, budgets = (6, 6), (512, 2048)
    mid = tree_cases.midgame()
    for what, kw in (("opening", dict(start=None, start_turn=None, n_rand=(3, 3))),
                     ("midgame", dict(start=mid["boards"][:8], start_turn=mid["turn"][:8], n_rand=(0, 0)))):
        got = run_games(binary, tmp_path, order, n=8, seed=77, depths=caps, budgets=budgets, exact=exact, swap=True,
                        limit=0, wa=wa, wb=wb, **kw)
        want = play_ref.play(8, 77, budget_chooser(fixed, tmp_path, (wa, wb), caps, budgets, exact, order),
                             n_rand_a=kw["n_rand"][0], n_rand_b=kw["n_rand"][1], swap=True, start=kw["start"],
                             start_turn=kw["start_turn"])
        for k in ("a_black", "final_boards", "diff", "plies", "status", "moves"):
            assert (np.asarray(got[k]) == np.asarray(want[k])).all(), (what, k)
        assert (got["nodes"] > 0).all()


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary, binary_asan, fixed, tmp_path):
    b, t = inputs()
    w = tree_cases.TABLES["rng7"]
    for order in (0, 1):
        search_at = fixed_depth(fixed, tmp_path, b, t, w, order, BMAX)
        for cap, budget in ((8, 4096), (4, 64), (1, 1)):
            same(run_budget(binary_asan, tmp_path, b, t, budget, cap, w, order),
                 budget_ref.deepen(search_at, b, budget, cap), ("asan", order, cap, budget))
    budgets = np.array([(0, 1, 8, 64, 512, 4096, 37, 1000)[i % 8] for i in range(len(t))], np.int64)
    same(run_budget(binary_asan, tmp_path, b, t, budgets, 8, w, 1), budget_ref.deepen(search_at, b, budgets, 8), "asan")
    mid = tree_cases.midgame()
    kw = dict(n=4, seed=5, depths=(6, 3), budgets=(300, 2000), exact=6, n_rand=(2, 2), swap=True, limit=0,
              start=mid["boards"][:4], start_turn=mid["turn"][:4], wa=w, wb=tree_cases.TABLES["default"])
    plain, san = run_games(binary, tmp_path, 1, **kw), run_games(binary_asan, tmp_path, 1, **kw)
    for k in plain:
        assert (plain[k] == san[k]).all(), k
