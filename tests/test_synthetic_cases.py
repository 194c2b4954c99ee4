"""tests/synthetic_cases.py's claims about its own positions, checked with the C
oracle and the exhaustive checkers alone, and the eight host drivers of the
searches' cores (tools/diag/{solve,search,tree,solve_tree,play,solve_window,
moves,line}_host.cpp: plain C++ rules, plain loads and stores) against the
checkers on every family: a rules bug in a *_core.hpp shows here, before any GPU
run.  The two tree drivers run every position's tasks in four orders (forward,
reverse, shuffled, nothing shared); every driver runs with order 0 and 1.  The
last three drivers (root windows, the value of every root move, the principal
variation) run on batches X and S, with the helpers of their own host files.
CPU only."""
import numpy as np
import pytest

import host_programs as hp
import oracle
import play_ref
import search_ref
import line_ref
import moves_ref
import solve_cases
import solve_ref
import synthetic_cases as sc
import test_line_host as line_host
import test_moves_host as moves_host
import test_solve_window_host as window_host
import tree_cases
import window_ref

DRIVERS = ("solve", "search", "tree", "solve_tree", "play")
SOLVED = SEARCHED = 1
SKIPPED, NOROOM = 0, 4
NODE_LIMIT = 1 << 22
THREADS = 8
SOLVE_TREE_DEFAULT_NODES, TREE_DEFAULT_NODES = 65536, 32768
T = sc.T
GAME_KEYS = ("a_black", "final_boards", "diff", "plies", "status", "moves")


# ---------------------------------------------------------------- the generator's claims
@pytest.mark.parametrize("family,e", [(f, e) for f in sorted(sc.FAMILIES) for e in (4, 6, 8, 12, 20, 40, 52)
                                      if f != "islands" or e <= 8])
def test_families_are_disjoint_with_the_empties_asked_and_both_movers(family, e):
    b, t = sc.FAMILIES[family](e)
    assert len(t) == (sc.ISLANDS_DEEP_ROOTS if family == "islands" and e > 6 else sc.ROOTS)
    assert ((b[:, 0] & b[:, 1]) == 0).all() and (solve_ref.empties(b) == e).all()
    assert set(t.tolist()) == {1, 2} and not b.flags.writeable and not t.flags.writeable
    assert len(np.unique(b, axis=0)) == len(b)
    if family == "centre":
        assert ((b[:, 0] | b[:, 1]) & np.uint64(sc._mask(sc.CENTRE)) == 0).all()
    if family == "islands":
        assert (sc.cut_off(b) >= (2 if e >= 6 else 1)).all()
    if family == "lopsided":
        share = sc.popcount(b[:, 0]) / (64.0 - e)
        for k, want in enumerate(sc.SHARES):
            assert abs(share[k::4].mean() - want) < 0.03
            assert set(t[k::4].tolist()) == {1, 2}


def test_the_rollout_pool_has_no_such_boards():
    """The centre squares are never empty in a game, and two empty squares
    without an occupied neighbour are rare near its end (none of the pool's
    2,078 positions at 4 empties, 0.3 % at 6, 0.9 % at 8)."""
    centre = np.uint64(sc._mask(sc.CENTRE))
    for p in solve_cases.pool().values():
        assert (((p["boards"][:, 0] | p["boards"][:, 1]) & centre) == centre).all()
    for e in (4, 6, 8):
        assert (sc.cut_off(solve_cases.pool()[e]["boards"]) >= 2).mean() < 0.01


@pytest.mark.parametrize("e", [6, 8])
def test_lopsided_roots_pass_and_end(e):
    fp, over = sc.root_kinds(*sc.lopsided(e))
    assert fp.sum() >= 8 and over.sum() >= 8
    # (measured: 13 and 13 at 6 empties, 11 and 16 at 8; the 8-empties rollout case has 8 of both kinds together)
    c = solve_cases.cases()[8]
    assert int(c["forced_pass"].sum() + c["over"].sum()) <= 8


def test_lopsided_values_go_further_than_uniform_ones():
    lv = sc.solver_reference("lopsided8")[0]
    uv = sc.solver_reference("uniform8")[0]
    assert np.abs(lv).max() >= 58 and np.abs(uv).max() <= 48  # (61 and 44)


def test_lopsided_trees_hold_more_passes_than_the_rollouts():
    """Per node of the whole trees: 69,586 inner passes in 435,741 nodes (0.160)
    against 0.103 in the trees of the last 16 roots of solve_cases.cases()[8].
    Per root it is the other way round, 544 against 1,352: the lopsided trees
    are a quarter of the size, most of their lines end early."""
    b, t = sc.solver_inputs("lopsided8")
    passes, _, _, nodes = sc.census(b, t, 16)
    assert passes.sum() == sc.solver_reference("lopsided8")[2]  # the checker's count
    c = solve_cases.cases()[8]
    rp, _, _, rn = sc.census(c["boards"][-16:], c["turn"][-16:], 16)
    assert passes.sum() / nodes.sum() > rp.sum() / rn.sum()
    assert passes.sum() / len(t) < c["inner_passes"] / len(c["turn"])


def test_wide_roots_have_28_moves_or_more():
    b, t = sc.wide()
    moves = sc.popcount(oracle.legal(b, t))
    assert len(t) == 16 and (moves >= sc.WIDE_MIN).all() and set(t.tolist()) == {1, 2}
    assert ((b[:, 0] & b[:, 1]) == 0).all()
    assert sc.wide_max() == 35 and moves.max() == 34  # the midgame roots of the other tests have at most 21
    assert sc.popcount(oracle.legal(tree_cases.midgame()["boards"], tree_cases.midgame()["turn"])).max() == 21
    assert len(sc.wide(32)[1]) == 32 and (sc.wide(32)[0][:16] == b).all()


def test_every_islands_root_can_end_with_empties_left():
    for e in (4, 6, 8):
        b, t = sc.islands(e)
        assert sc.census(b, t, 2 * e)[2].all()


@pytest.mark.parametrize("name", ["lopsided6_d9", "lopsided8_d9", "islands6_d9", "islands8_d9"])
def test_split_cases_pass_and_end_inside_the_split_plies(name):
    """Split 4: a node that must pass at levels 1..3, a game-over node at
    levels 1..4.  Measured, roots with a pass / with a final: lopsided 81 / 20
    at 6 empties and 68 / 19 at 8, islands 42 / 9 at 6 and 19 / 0 at 8: no
    islands(8) game ends within four plies (it would leave four empties or
    more), so that case has passes only and islands(6) stands in for the finals."""
    b, t = sc.search_inputs(name)
    passes, finals, _, _ = sc.census(b, t, 4)
    assert (passes > 0).sum() >= 8
    assert (finals > 0).sum() >= (0 if name == "islands8_d9" else 8)
    fp, over = sc.root_kinds(b, t)
    assert fp.sum() + over.sum() >= (8 if name.startswith("lopsided") else 1)


def test_islands_end_inside_the_solvers_split_plies():
    """The split solver expands down to task_empties = 1: every level of an
    islands(6) tree, game-overs with empties included."""
    b, t = sc.islands(6)
    _, finals, with_empties, _ = sc.census(b, t, 5)
    assert (finals > 0).sum() >= 8 and with_empties.sum() >= 8


def test_the_edges_are_what_their_names_say():
    b, t, names = sc.edges()
    assert len(t) == 2 * len(sc.EDGES) == 20 and ((b[:, 0] & b[:, 1]) == 0).all()
    own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
    emp = solve_ref.empties(b)
    for name, e in (("empty", 64), ("one disc", 63), ("two adjacent discs", 62), ("full black", 0), ("full white", 0),
                    ("full 63:1", 0), ("full 32:32", 0), ("four unplayable empties", 4)):
        for turn in (1, 2):
            i = sc.edge(name, turn)
            assert names[i] == name and t[i] == turn and emp[i] == e and own[i] == 0 and opp[i] == 0, (name, turn)
    i = sc.edge("wipe-out", 1)
    assert own[i] == 1 and emp[i] == 2  # a1, and it leaves White without a disc
    after = oracle.step(b[i:i + 1], t[i:i + 1], np.array([0], np.uint8))["boards"]
    assert after[0, 1] == 0 and sc.popcount(after[:, 0])[0] == 63
    i = sc.edge("pass then the last move", 1)
    assert own[i] == 0 and opp[i] == 1 and emp[i] == 1
    v, m, _ = solve_ref.solve(b, t)
    want = {("full black", 1): 64, ("full black", 2): -64, ("full white", 1): -64, ("full 63:1", 1): 62,
            ("full 63:1", 2): -62, ("full 32:32", 1): 0, ("empty", 1): 0, ("wipe-out", 1): 63,
            ("four unplayable empties", 1): 3 - 57}
    for (name, turn), value in want.items():
        assert v[sc.edge(name, turn)] == value, (name, turn)
    assert m[sc.edge("wipe-out", 1)] == 0 and m[sc.edge("pass then the last move", 1)] == 64
    assert (m[:16] == 255).all()


def test_images_are_the_16_images():
    b, t = sc.uniform(30)
    ib, it, perm = sc.images(b[:4], t[:4])
    assert ib.shape == (64, 2) and it.shape == (64,) and perm.shape == (64, 64)
    assert (np.sort(perm, axis=1) == np.arange(64)).all()
    assert (ib[0] == b[0]).all() and it[0] == t[0] and (perm[0] == np.arange(64)).all()  # the identity comes first
    assert (ib[8] == b[0, ::-1]).all() and it[8] == 3 - t[0]
    for j in range(64):
        src = b[j // 16, ::-1] if j % 16 >= 8 else b[j // 16]
        for c in (0, 1):
            assert int(ib[j, c]) == sc._mask(perm[j][s] for s in range(64) if int(src[c]) >> s & 1)
    assert len(np.unique(ib[:16], axis=0)) == 16
    # legal moves move with the squares
    own = oracle.legal(ib, it)
    root = oracle.legal(b[:4], t[:4])
    for j in range(64):
        assert int(own[j]) == sc._mask(perm[j][s] for s in range(64) if int(root[j // 16]) >> s & 1)


def test_the_eval_is_the_same_on_all_16_images():
    """The region masks are symmetric and the eval is from the given side: what
    the GPU file's metamorphic tests rely on.  (It is not antisymmetric in the
    side: an image's value is equal, not opposite, because the mover swaps too.)"""
    for e in (10, 30, 52):
        b, t = sc.uniform(e)
        ib, it, _ = sc.images(b[:16], t[:16])
        for w in sc.TABLES.values():
            ev = oracle.evaluate(ib, it, w).reshape(16, 16)
            assert (ev == ev[:, :1]).all()
            assert len(np.unique(ev[:, 0])) > 8


def test_the_tied_roots():
    for kind, roots in (("solve", 8), ("search", 5)):  # 13 tied roots: at least 8 are asked for
        b, t, v, m = sc.tie_roots(kind)
        assert len(t) == 16 * roots
        v, m = v.reshape(-1, 16), m.reshape(-1, 16)
        assert (v == v[:, :1]).all()
        assert all(len(set(row.tolist())) > 1 for row in m)


# ---------------------------------------------------------------- the host drivers
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return {name: hp.compiled(tmp_path_factory, name + "_host") for name in DRIVERS}


def run_driver(exe, tmp_path, boards, turn, args, weights=None, orders=1):
    """(value, move, status) of a driver: [n], or [4 task orders][n] for the two tree drivers."""
    inp, out, wf = (str(tmp_path / x) for x in ("in", "out", "w"))
    hp.write_positions(inp, boards, turn)
    head = [exe, inp, out]
    if weights is not None:
        hp.write_weights(wf, weights, end="\n")
        head.append(wf)
    hp.run(head + list(args))
    if orders == 1:
        rows = hp.read_rows(out)
        return rows[:, 0], rows[:, 1], rows[:, 2]
    return hp.read_rows(out, orders=orders)[:3]


def solve_host(host, tmp_path, boards, turn, max_empties=12):
    return run_driver(host["solve"], tmp_path, boards, turn, [max_empties, NODE_LIMIT, THREADS])


def solve_tree_host(host, tmp_path, boards, turn, task_empties, npp, order, max_empties=16):
    return run_driver(host["solve_tree"], tmp_path, boards, turn,
                      [max_empties, task_empties, npp, NODE_LIMIT, 7, order, THREADS], orders=4)


def search_host(host, tmp_path, boards, turn, depth, table, order):
    return run_driver(host["search"], tmp_path, boards, turn, [depth, NODE_LIMIT, THREADS, order], sc.TABLES[table])


def tree_host(host, tmp_path, boards, turn, depth, split, table, order, npp=TREE_DEFAULT_NODES):
    return run_driver(host["tree"], tmp_path, boards, turn, [depth, split, npp, NODE_LIMIT, 1, order],
                      sc.TABLES[table], orders=4)


def play_host(host, tmp_path, name, order, boards=None, turn=None, depth=None, exact=None, seed=None):
    c = sc.PLAY[name] if name else dict(depth=depth, exact=exact, seed=seed)
    if boards is None:
        boards, turn = sc.play_starts(name)
    args, out = str(tmp_path / "args"), str(tmp_path / "out")
    hp.write_game_args(args, len(turn), c["seed"], c["depth"], c["exact"], (0, 0), True, NODE_LIMIT,
                       sc.TABLES["default"], sc.TABLES["rng7"], boards, turn)
    hp.run([host["play"], args, out, THREADS, order])
    return hp.read_games(out)


def same(got, want, what, status=SOLVED):
    v, m, s = got
    assert (s == status).all(), (what, np.nonzero(s != status)[0][:8])
    bad = np.nonzero((v != want[0]) | (m != want[1]))[0]
    assert len(bad) == 0, (what, bad[:8], v[bad[:8]], want[0][bad[:8]], m[bad[:8]], want[1][bad[:8]])


def same_in_all_orders(got, want, what, status=SOLVED):
    for o in range(4):
        same(tuple(x[o] for x in got), want, (what, o), status)


@pytest.mark.parametrize("name", sorted(sc.SOLVER))
def test_solve_host_matches_the_checker(host, tmp_path, name):
    b, t = sc.solver_inputs(name)
    same(solve_host(host, tmp_path, b, t), sc.solver_reference(name), name)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.SOLVER))
def test_solve_tree_host_matches_the_checker(host, tmp_path, name, order):
    b, t = sc.solver_inputs(name)
    for task_empties in (1, 3):
        for npp in (64, SOLVE_TREE_DEFAULT_NODES):
            got = solve_tree_host(host, tmp_path, b, t, task_empties, npp, order)
            same_in_all_orders(got, sc.solver_reference(name), (name, task_empties, npp))


def test_the_solvers_host_builds_on_the_edges(host, tmp_path):
    b, t, names = sc.edges()
    rv, rm, _ = solve_ref.solve(b, t)
    small = solve_ref.empties(b) <= 12
    want = (np.where(small, rv, 0), np.where(small, rm, 255))
    status = np.where(small, SOLVED, SKIPPED)
    v, m, s = solve_host(host, tmp_path, b, t)
    assert (s == status).all() and (v == want[0]).all() and (m == want[1]).all()
    for order in (0, 1):
        for task_empties in (1, 3):
            v, m, s = solve_tree_host(host, tmp_path, b, t, task_empties, 64, order)
            for o in range(4):
                assert (s[o] == status).all() and (v[o] == want[0]).all() and (m[o] == want[1]).all()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.SEARCH))
def test_search_host_matches_the_checker(host, tmp_path, name, order):
    _, depth, _, tables, _ = sc.SEARCH[name]
    b, t = sc.search_inputs(name)
    for table in tables:
        same(search_host(host, tmp_path, b, t, depth, table, order), sc.search_reference(name, table), (name, table))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.SEARCH) + sorted(sc.TREE))
def test_tree_host_matches_the_checker(host, tmp_path, name, order):
    _, depth, _, tables, splits = sc.search_case(name)
    b, t = sc.search_inputs(name)
    for table in tables if name in sc.TREE or depth < 8 else ("default",):  # (full depth: no eval is taken)
        for split in splits:
            for npp in (TREE_DEFAULT_NODES,) if name == "wide5" else (TREE_DEFAULT_NODES, 64):
                # (64 nodes: the tasks start higher; depth - 1 <= 8 plies are left below the root's level)
                got = tree_host(host, tmp_path, b, t, depth, split, table, order, npp)
                same_in_all_orders(got, sc.search_reference(name, table), (name, table, split, npp))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("split", sc.NOROOM_SPLITS)
def test_tree_host_has_no_room_exactly_where_the_rule_says(host, tmp_path, split, order):
    b, t, rv, rm = sc.noroom_case()
    want = tree_cases.expected_noroom(b, t, sc.NOROOM_DEPTH, split, sc.NOROOM_SLAB)
    assert want.sum() == 16 and len(t) == 48 and (want == (sc.popcount(oracle.legal(b, t)) >= sc.WIDE_MIN)).all()
    v, m, s = tree_host(host, tmp_path, b, t, sc.NOROOM_DEPTH, split, "default", order, sc.NOROOM_SLAB)
    for o in range(4):
        assert (s[o] == np.where(want, NOROOM, SEARCHED)).all()
        assert (v[o] == rv).all() and (m[o] == rm).all()


def test_the_searches_host_builds_on_the_edges(host, tmp_path):
    b, t, names = sc.edges()
    for table in ("default", "extreme"):
        rv, rm, _ = search_ref.search(b, t, 3, sc.TABLES[table])
        assert rv[sc.edge("full black", 1)] == 64 * T and rv[sc.edge("full white", 1)] == -64 * T
        for order in (0, 1):
            same(search_host(host, tmp_path, b, t, 3, table, order), (rv, rm), "edges")
            same_in_all_orders(tree_host(host, tmp_path, b, t, 3, 2, table, order), (rv, rm), "edges")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.PLAY))
def test_play_host_matches_the_checker(host, tmp_path, name, order):
    got, ref = play_host(host, tmp_path, name, order), sc.play_reference(name)
    for k in GAME_KEYS:
        assert (got[k] == ref[k]).all(), (name, k)
    if name.startswith("lopsided"):
        assert (ref["plies"] == 0).any() and (ref["moves"] == 64).any()  # starts that are over; passes


@pytest.mark.parametrize("order", [0, 1])
def test_ties_in_the_host_builds(host, tmp_path, order):
    """Every image against the checker run on that image, through all five."""
    b, t, rv, rm = sc.tie_roots("solve")
    same(solve_host(host, tmp_path, b, t), (rv, rm), "solve")
    for task_empties in (1, 3):
        same_in_all_orders(solve_tree_host(host, tmp_path, b, t, task_empties, 64, order), (rv, rm), "solve tree")
    same(search_host(host, tmp_path, b, t, 6, "default", order), (T * rv, rm), "search, full depth")
    for split in (1, 2, 3):
        same_in_all_orders(tree_host(host, tmp_path, b, t, 6, split, "default", order), (T * rv, rm), "tree")
    ref = play_ref.play(len(t), 300, play_ref.search_chooser(sc.TABLES["default"], sc.TABLES["rng7"], 2, 2, 6),
                        swap=True, start=b, start_turn=t)
    got = play_host(host, tmp_path, None, order, b, t, depth=(2, 2), exact=6, seed=300)
    for k in GAME_KEYS:
        assert (got[k] == ref[k]).all(), k
    own = sc.popcount(oracle.legal(b, t))
    assert (ref["moves"][own > 1, 0] == rm[own > 1]).all()  # the first move is the solver's, the tie rule's
    b, t, rv, rm = sc.tie_roots("search")
    same(search_host(host, tmp_path, b, t, sc.TIE_DEPTH, sc.TIE_TABLE, order), (rv, rm), "search")
    same_in_all_orders(tree_host(host, tmp_path, b, t, sc.TIE_DEPTH, 1, sc.TIE_TABLE, order), (rv, rm), "tree")


# ---------------------------------------------------------------- windows, per-move values and lines: batches X and S
def test_what_batches_x_and_s_hold():
    """From the oracle and the checkers alone: a drift in the generators shows here."""
    b, t = sc.batch_x()
    emp = solve_ref.empties(b)
    own = sc.popcount(oracle.legal(b, t))
    forced, over = sc.root_kinds(b, t)
    assert len(t) == 398 and emp.max() == 8 and not b.flags.writeable
    assert (forced.sum(), over.sum()) == (21, 23)
    ln = sc.x_line()
    assert ((ln["line"] == 64).any(1).sum(), (ln["line"][:, 1:] == 64).any(1).sum()) == (139, 128)
    assert (solve_ref.empties(ln["end_boards"]) > 0).sum() == 51 and ln["length"].max() == 13
    assert ((own == emp) & (emp > 0)).sum() == 86 and own.max() == 8  # the last of max(max_empties, 1) task slots
    r, w = sc.x_roots(), sc.x_windows()
    assert len(w["turn"]) == 3582 == 9 * len(t) and set(w["family"].tolist()) == set(range(9))
    wld = sc.x_family("wld")
    assert ((w["value"][wld] == 1).sum(), (w["value"][wld] == -1).sum()) == (203, 177)
    assert ((r.value >= 1).sum(), (r.value <= -1).sum()) == (203, 177)
    assert (w["move"][sc.x_family("on_beta")] < 64).sum() == 354
    assert np.abs(r.value).max() == 64 and (np.abs(r.value) >= 61).sum() >= 8  # the ends of the windows' range
    rows, value, move = sc.x_moves()
    assert (value == r.value).all() and (value == ln["value"]).all() and (move == ln["best_move"]).all()
    b, t = sc.batch_s()
    forced, over = sc.root_kinds(b, t)
    assert len(t) == 124 and (forced.sum(), over.sum()) == (6, 22)
    assert sc.popcount(oracle.legal(b, t)).max() == 34
    ln = sc.s_line(4, "default")
    assert ((ln["line"] == 64).any(1).sum(), (ln["length"] < 4).sum()) == (17, 32)
    for depth, table in sc.S_RUNS:  # the two checkers agree with each other
        rows, value, move = sc.s_moves(depth, table)
        assert (value == sc.s_line(depth, table)["value"]).all(), (depth, table)
        assert (move == sc.s_line(depth, table)["best_move"]).all(), (depth, table)
    for name in sc.FULL_DEPTH_CASES:
        fb, ft, _, _ = sc.full_depth_case(name)
        assert len(ft) == 32 and (fb == sc.solver_inputs(name)[0][:32]).all()


def test_the_checkers_rows_move_with_the_squares():
    """What the GPU file's image tests of the rows rely on: an image's row, taken back through its permutation,
    is its root's; exact rows at 6 empties, search rows at depth 2 on the three tables."""
    for family in ("uniform", "lopsided"):
        b, t = sc.FAMILIES[family](6)
        ib, it, perm = sc.images(b[:8], t[:8])
        rows = np.take_along_axis(moves_ref.exact(window_ref.roots(ib, it))[0], perm, 1).reshape(8, 16, 64)
        assert (rows == rows[:, :1]).all() and (rows != moves_ref.NOT_A_MOVE).any()
    b, t = sc.uniform(30)
    ib, it, perm = sc.images(b[:4], t[:4])
    for table in sc.ALL_TABLES:
        rows = np.take_along_axis(moves_ref.search(ib, it, 2, sc.TABLES[table])[0], perm, 1).reshape(4, 16, 64)
        assert (rows == rows[:, :1]).all()


@pytest.fixture(scope="module")
def window_exe(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_window_host")


@pytest.fixture(scope="module")
def moves_exe(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "moves_host")


@pytest.fixture(scope="module")
def line_exe(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "line_host")


def run_windows(exe, tmp_path, rows, task_empties, npp, threads, what):
    w = sc.x_windows()
    got = window_host.run(exe, tmp_path, ("a", 16, task_empties, npp, threads), w["boards"][rows], w["turn"][rows],
                          w["alpha"][rows], w["beta"][rows])
    window_host.check_mode_a(got, w["value"][rows], w["move"][rows], what)
    return got


@pytest.mark.parametrize("npp", [64, 4096])
@pytest.mark.parametrize("task_empties", [1, 3])
def test_window_host_on_batch_x_in_every_family(window_exe, tmp_path, task_empties, npp):
    w = sc.x_windows()
    got = run_windows(window_exe, tmp_path, slice(None), task_empties, npp, THREADS, (task_empties, npp))
    full = w["family"] == 0
    assert (got[:, 3] <= got[:, 4]).all() and (got[full, 3] == got[full, 4]).all()  # a subtree of the full window's
    over = sc.root_kinds(w["boards"], w["turn"])[1]
    assert (got[over, 1] == 255).all() and (got[over, 3] == 0).all()


def check_exact_rows(got, want, b, t, what):
    moves_host.check(got, want, SOLVED, what)
    forced, over = sc.root_kinds(b, t)
    assert (got[3][over] == 0).all() and (got[1][over] == 255).all() and (got[1][forced] == 64).all(), what
    assert (got[4][forced | over] == moves_ref.NOT_A_MOVE).all(), what


@pytest.mark.parametrize("level", [8, 12])
def test_moves_host_exact_rows_on_batch_x(moves_exe, tmp_path, level):
    """Level 8: the roots of 8 empties with 8 moves fill the last of their task slots."""
    b, t = sc.batch_x()
    check_exact_rows(moves_host.run(moves_exe, tmp_path, "solve", b, t, level), sc.x_moves(), b, t, level)


def check_search_rows(exe, tmp_path, runs):
    b, t = sc.batch_s()
    _, over = sc.root_kinds(b, t)
    for depth, table in runs:
        got = moves_host.run(exe, tmp_path, "search", b, t, depth, sc.TABLES[table])
        moves_host.check(got, sc.s_moves(depth, table), SEARCHED, (depth, table))
        assert (got[3][over] == 0).all() and (got[4][over] == moves_ref.NOT_A_MOVE32).all(), (depth, table)


@pytest.mark.parametrize("depth,table", sc.S_RUNS)
def test_moves_host_search_rows_on_batch_s(moves_exe, tmp_path, depth, table):
    check_search_rows(moves_exe, tmp_path, [(depth, table)])


def check_exact_lines(exe, tmp_path):
    b, t = sc.batch_x()
    got = line_host.run_solve(exe, tmp_path, b, t)
    assert (got["status"] == SOLVED).all()
    line_host.same_line(got, sc.x_line(), "batch X")
    assert (line_ref.end_score(got["end_boards"], t) == got["value"]).all()
    forced, over = sc.root_kinds(b, t)
    assert (got["line"][forced, 0] == 64).all() and (got["length"][over] == 0).all()
    assert (got["best_move"][over] == 255).all() and (got["nodes"][over] == 0).all()


def check_search_lines(exe, tmp_path, runs):
    b, t = sc.batch_s()
    for depth, table in runs:
        for order in (0, 1):
            got = line_host.run_search(exe, tmp_path, b, t, depth, sc.TABLES[table], order)
            assert (got["status"] == SEARCHED).all()
            line_host.same_line(got, sc.s_line(depth, table), (depth, table, order))
            assert (line_ref.end_score(got["end_boards"], t, sc.TABLES[table]) == got["value"]).all()


def test_line_host_exact_lines_on_batch_x(line_exe, tmp_path):
    check_exact_lines(line_exe, tmp_path)


@pytest.mark.parametrize("depth,table", sc.S_RUNS)
def test_line_host_search_lines_on_batch_s(line_exe, tmp_path, depth, table):
    check_search_lines(line_exe, tmp_path, [(depth, table)])


@pytest.mark.parametrize("name", sc.FULL_DEPTH_CASES)
def test_the_three_drivers_at_full_depth(window_exe, moves_exe, line_exe, tmp_path, name):
    """Depth 8 at 8 empties: the search rows and the search line are the exact ones times T on every table; the
    window driver on the same roots with tasks of six empties, which no other run here has."""
    b, t, line, exact = sc.full_depth_case(name)
    sel = sc.x_rows_of(name)
    pairs = np.nonzero((sc.x_windows()["root"] >= sel.start) & (sc.x_windows()["root"] < sel.stop))[0]
    assert len(pairs) == 9 * 32
    run_windows(window_exe, tmp_path, pairs, 6, 64, THREADS, name)
    for table in sc.ALL_TABLES:
        w = sc.TABLES[table]
        got = moves_host.run(moves_exe, tmp_path, "search", b, t, sc.FULL_DEPTH, w)
        moves_host.check(got, sc.exact_rows_times_t(*exact), SEARCHED, (name, table))
        for order in (0, 1):
            got = line_host.run_search(line_exe, tmp_path, b, t, sc.FULL_DEPTH, w, order)
            assert (got["status"] == SEARCHED).all()
            line_host.same_line(got, line, (name, table, order), scale=T)
            assert (line_ref.end_score(got["end_boards"], t, w) == got["value"]).all()


def test_line_host_depths_per_position_on_batch_s(line_exe, tmp_path):
    """0 is not searched, 9 is out of range, 8 only where it ends the game (at most 8 empties; depth 3 on the
    other rows of that index): test_line_host.deep_and_mixed_checks' statuses."""
    b, t = sc.batch_s()
    depths = per_position_depths(b)
    w = sc.TABLES["default"]
    got = line_host.run_search(line_exe, tmp_path, b, t, depths, w, 1)
    check_per_position(got, b, t, depths, w)


def per_position_depths(boards):
    d = np.array([(0, 1, 2, 3, 8, 9)[i % 6] for i in range(len(boards))])
    return np.where((d == 8) & (solve_ref.empties(boards) > 8), 3, d)


def check_per_position(got, b, t, depths, weights):
    """A per-position result of batch S on the "default" table against the references of each depth."""
    assert (got["status"] == np.where(depths == 0, line_host.LIMIT,
                                      np.where(depths == 9, line_host.BADDEPTH, SEARCHED))).all()
    off = (depths == 0) | (depths == 9)
    assert (got["length"][off] == 0).all() and (got["value"][off] == 0).all() and (got["nodes"][off] == 0).all()
    assert (got["best_move"][off] == 255).all() and (got["line"][off] == 255).all()
    assert (got["end_boards"][off] == b[off]).all()
    for depth in (1, 2, 3, 8):
        sel = depths == depth
        assert sel.sum() >= 4  # (7 rows of batch S at depth 8, 20 or more at the others)
        ref = line_ref.search(b[sel], t[sel], 8, weights) if depth == 8 else \
            {k: v[sel] for k, v in sc.s_line(depth, "default").items()}
        line_host.same_line({k: v[sel] for k, v in got.items()}, ref, ("per position", depth))
    assert (line_ref.end_score(got["end_boards"][~off], t[~off], weights) == got["value"][~off]).all()


S_DEFAULT_RUNS = [(d, "default") for d in (1, 2, 3)]


def test_window_host_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "solve_window_host", hp.SANITIZED)
    run_windows(exe, tmp_path, slice(None), 3, 4096, 1, "asan")
    run_windows(exe, tmp_path, slice(None), 1, 64, 1, "asan, 64 nodes")


def test_moves_host_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "moves_host", hp.SANITIZED)
    b, t = sc.batch_x()
    for level in (8, 12):
        check_exact_rows(moves_host.run(exe, tmp_path, "solve", b, t, level), sc.x_moves(), b, t, ("asan", level))
    check_search_rows(exe, tmp_path, S_DEFAULT_RUNS)


def test_line_host_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "line_host", hp.SANITIZED)
    check_exact_lines(exe, tmp_path)
    check_search_lines(exe, tmp_path, S_DEFAULT_RUNS)
