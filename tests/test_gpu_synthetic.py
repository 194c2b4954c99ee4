"""The five search entry points on the GPU (ops.solve, ops.solve(task_empties=),
ops.search, ops.search(split=), ops.play) on the positions of
tests/synthetic_cases.py, which no game from the opening reaches: every value,
best move and status against the exhaustive checkers (tests/solve_ref.py,
search_ref.py, play_ref.py), node counts never; then what no checker reaches,
by symmetry: a root's 16 images have one value, and an image's best move leads
to a position worth minus that.

The same for the calls built on them, on batches X and S of synthetic_cases.py:
root windows and win/draw/loss (ops.solve(window=, wld=), one lane and split)
against tests/window_ref.py, the value of every root move (ops.solve_moves in
its three forms, ops.search_moves) against tests/moves_ref.py, the principal
variation (ops.solve_line, ops.search_line) against tests/line_ref.py; beyond
the checkers, a root's 16 images have one row up to the images' permutations, and
rows, lines and windowed answers are those of the calls they replace.

NODE_LIMIT is 2**22 throughout: a defect ends as LIMIT, which every comparison
refuses, not as a long kernel.  runner.do_matches(policy="search") takes no start
positions, so it is not run here."""
import functools

import numpy as np
import pytest
import torch

import line_ref
import moves_ref
import oracle
import play_ref
import search_ref
import solve_ref
import synthetic_cases as sc
import test_gpu_line as gpu_line
import test_gpu_moves as gpu_moves
import test_gpu_solve_window as gpu_window
import tree_cases
import window_ref
from test_line_host import same_line
from test_synthetic_cases import check_per_position, per_position_depths

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402

SKIPPED, SOLVED, LIMIT = _lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_LIMIT
SEARCHED, NOROOM = _lib.SEARCH_SEARCHED, _lib.TREE_NOROOM
NODE_LIMIT = 1 << 22
T = sc.T
GAME_KEYS = ("a_black", "final_boards", "diff", "plies", "moves", "status")


def dev(boards, turn):
    return (ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda"),
            torch.from_numpy(np.array(turn, np.uint8)).cuda())


def gpu_solve(boards, turn, max_empties=12, **kw):
    """ops.solve's (value int64, best_move, status); with task_empties= the split solver."""
    b, t = dev(boards, turn)
    r = ops.solve(b, t, max_empties=max_empties, node_limit=NODE_LIMIT, **kw)
    torch.cuda.synchronize()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()


def gpu_search(boards, turn, depth, table, **kw):
    """ops.search's (value int64, best_move, status); with split= the split search."""
    b, t = dev(boards, turn)
    r = ops.search(b, t, depth, weights=sc.TABLES[table], node_limit=NODE_LIMIT, **kw)
    torch.cuda.synchronize()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()


def gpu_play(boards, turn, seed, depth, exact, order):
    b, t = dev(boards, turn)
    r = ops.play(len(turn), seed, weights_a=sc.TABLES["default"], weights_b=sc.TABLES["rng7"], depth_a=depth[0],
                 depth_b=depth[1], exact_empties=exact, swap_colours=True, start=b, start_turn=t, record_moves=True,
                 node_limit=NODE_LIMIT, order=order)
    torch.cuda.synchronize()
    out = {k: getattr(r, k).cpu().numpy() for k in ("a_black", "diff", "plies", "moves", "status")}
    out["final_boards"] = ops.to_numpy_u64(r.final_boards).reshape(-1, 2)
    return out


def same(got, want, what, status=SOLVED):
    v, m, s = got
    assert (s == status).all(), (what, np.nonzero(s != status)[0][:8], s[s != status][:8])
    bad = np.nonzero((v != want[0]) | (m != want[1]))[0]
    assert len(bad) == 0, (what, bad[:8], v[bad[:8]], want[0][bad[:8]], m[bad[:8]], want[1][bad[:8]])


def same_games(got, ref, what):
    for k in GAME_KEYS:
        bad = np.nonzero(np.asarray(got[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[0]
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:4]], ref[k][bad[:4]])


# ---------------------------------------------------------------- the solvers
@pytest.mark.parametrize("name", sorted(sc.SOLVER))
def test_solve_matches_the_checker(name):
    b, t = sc.solver_inputs(name)
    same(gpu_solve(b, t), sc.solver_reference(name), name)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3])
@pytest.mark.parametrize("name", sorted(sc.SOLVER))
def test_split_solve_matches_the_checker(name, task_empties, order):
    """With the default slab the whole top of every tree is expanded (game-overs
    with empties left and passes inside it); with 64 nodes the levels stop
    fitting and the tasks start higher."""
    b, t = sc.solver_inputs(name)
    for slab in (_lib.SOLVE_TREE_DEFAULT_NODES, _lib.SOLVE_TREE_MIN_NODES):
        got = gpu_solve(b, t, 16, task_empties=task_empties, order=order, nodes_per_position=slab)
        same(got, sc.solver_reference(name), (name, task_empties, order, slab))
    assert ops.work_word("cuda").item() == 0


def test_the_solvers_on_the_edges():
    b, t, names = sc.edges()
    rv, rm, _ = solve_ref.solve(b, t)
    small = solve_ref.empties(b) <= 12
    assert (~small).sum() == 6  # the empty board, one disc, two discs
    want = (np.where(small, rv, 0), np.where(small, rm, 255))
    status = np.where(small, SOLVED, SKIPPED)
    runs = [gpu_solve(b, t)] + [gpu_solve(b, t, 16, task_empties=te, order=o, nodes_per_position=slab)
                                for te in (1, 3) for o in (0, 1) for slab in (65536, 64)]
    for v, m, s in runs:
        assert (s == status).all() and (v == want[0]).all() and (m == want[1]).all(), (v, m, s)
        for (name, turn), value in {("full black", 1): 64, ("full black", 2): -64, ("full white", 1): -64,
                                    ("full white", 2): 64, ("full 63:1", 1): 62, ("full 63:1", 2): -62,
                                    ("full 32:32", 1): 0, ("full 32:32", 2): 0}.items():
            i = sc.edge(name, turn)
            assert (v[i], m[i], s[i]) == (value, 255, SOLVED), (name, turn)
        i = sc.edge("empty", 1)
        assert (v[i], m[i], s[i]) == (0, 255, SKIPPED)
        i = sc.edge("wipe-out", 1)
        assert (v[i], m[i]) == (63, 0)  # the discs on the board, the empty square earns nothing
        i = sc.edge("pass then the last move", 1)
        assert (v[i], m[i]) == (int(rv[i]), 64)


# ---------------------------------------------------------------- the searches
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.SEARCH))
def test_search_matches_the_checker(name, order):
    _, depth, _, tables, _ = sc.SEARCH[name]
    b, t = sc.search_inputs(name)
    for table in tables:
        same(gpu_search(b, t, depth, table, order=order), sc.search_reference(name, table), (name, table), SEARCHED)
    assert ops.work_word("cuda").item() == 0


def test_full_depth_search_is_t_times_the_solver():
    for name in ("lopsided8", "islands8"):
        b, t = sc.search_inputs(name)
        v, m, s = gpu_solve(b, t)
        assert (s == SOLVED).all()
        for table in sc.ALL_TABLES:
            same(gpu_search(b, t, 8, table), (T * v, m), (name, table), SEARCHED)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.SEARCH) + sorted(sc.TREE))
def test_split_search_matches_the_checker(name, order):
    """split 1..3 below the depth; depth 9 with split 4 at 6 and 8 empties, where
    roots without a single task are answered by the expansion alone; depth 5 with
    split 4 on the wide roots.  In 64 nodes the level after a wide root's does
    not fit: the tasks start higher and search deeper."""
    _, depth, _, tables, splits = sc.search_case(name)
    b, t = sc.search_inputs(name)
    for table in tables:
        for split in splits:
            for slab in (_lib.TREE_DEFAULT_NODES,) if name == "wide5" else (_lib.TREE_DEFAULT_NODES, 64):
                got = gpu_search(b, t, depth, table, split=split, order=order, nodes_per_position=slab)
                same(got, sc.search_reference(name, table), (name, table, split, slab), SEARCHED)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("split", sc.NOROOM_SPLITS)
def test_no_room_exactly_on_the_wide_roots(split, order):
    """Depth 10 in 64 nodes: a wide root's own level fits and leaves 9 plies,
    the next does not fit; the roots of four empties beside them fit whole."""
    b, t, rv, rm = sc.noroom_case()
    want = tree_cases.expected_noroom(b, t, sc.NOROOM_DEPTH, split, sc.NOROOM_SLAB)
    assert want.sum() == 16 and len(t) == 48
    v, m, s = gpu_search(b, t, sc.NOROOM_DEPTH, "default", split=split, order=order, nodes_per_position=sc.NOROOM_SLAB)
    assert (s == np.where(want, NOROOM, SEARCHED)).all(), (s, want)
    assert (v == rv).all() and (m == rm).all()
    assert ops.work_word("cuda").item() == 0


def test_the_searches_on_the_edges():
    b, t, names = sc.edges()
    for table in sc.ALL_TABLES:
        rv, rm, _ = search_ref.search(b, t, 3, sc.TABLES[table])
        runs = [gpu_search(b, t, 3, table, order=o, want_nodes=False) for o in (0, 1)]
        runs += [gpu_search(b, t, 3, table, split=sp, order=o) for sp in (1, 2) for o in (0, 1)]
        for v, m, s in runs:
            same((v, m, s), (rv.astype(np.int64), rm), table, SEARCHED)
            for name, turn, value in (("full black", 1, 64), ("full black", 2, -64), ("full white", 1, -64),
                                      ("full white", 2, 64), ("full 63:1", 1, 62), ("empty", 1, 0), ("empty", 2, 0)):
                i = sc.edge(name, turn)
                assert (v[i], m[i]) == (value * T, 255), (name, turn)
    # the documented bound 64 * T = 2**23, and no node is counted on a board where the game is over
    eb, et = dev(b, t)
    r = ops.search(eb, et, 3, weights=sc.TABLES["extreme"], node_limit=NODE_LIMIT, want_nodes=True)
    nodes = r.nodes.cpu().numpy().view(np.uint32)
    assert int(r.value.cpu().numpy()[sc.edge("full black", 1)]) == 1 << 23
    assert nodes[sc.edge("empty", 1)] == 0 and nodes[sc.edge("empty", 2)] == 0


# ---------------------------------------------------------------- play
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.PLAY))
def test_games_match_the_checker(name, order):
    c = sc.PLAY[name]
    b, t = sc.play_starts(name)
    got = gpu_play(b, t, c["seed"], c["depth"], c["exact"], order)
    assert (got["status"] == SEARCHED).all()
    same_games(got, sc.play_reference(name), name)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("order", [0, 1])
def test_ties_keep_each_images_own_lowest_square(order):
    """13 tied roots (8 under the solver, 5 under the depth-2 search), 16 images
    each, every image against the checker run on that image: the image's
    permutation does not keep the lowest square the lowest."""
    b, t, rv, rm = sc.tie_roots("solve")
    assert len(t) == 16 * 8 and len(sc.tie_roots("search")[1]) == 16 * 5
    if order == 0:
        same(gpu_solve(b, t), (rv, rm), "solve")
    for task_empties in (1, 3):
        same(gpu_solve(b, t, 16, task_empties=task_empties, order=order), (rv, rm), ("split solve", task_empties))
    same(gpu_search(b, t, 6, "default", order=order), (T * rv, rm), "search, full depth", SEARCHED)
    for split in (1, 2, 3):
        same(gpu_search(b, t, 6, "default", split=split, order=order), (T * rv, rm), ("split search", split), SEARCHED)
    ref = play_ref.play(len(t), 300, play_ref.search_chooser(sc.TABLES["default"], sc.TABLES["rng7"], 2, 2, 6),
                        swap=True, start=b, start_turn=t)
    same_games(gpu_play(b, t, 300, (2, 2), 6, order), ref, "play")
    b, t, rv, rm = sc.tie_roots("search")
    same(gpu_search(b, t, sc.TIE_DEPTH, sc.TIE_TABLE, order=order), (rv, rm), "search", SEARCHED)
    same(gpu_search(b, t, sc.TIE_DEPTH, sc.TIE_TABLE, split=1, order=order), (rv, rm), "split search", SEARCHED)


# ---------------------------------------------------------------- beyond the checkers: the 16 images
def after_the_move(boards, turn, move):
    """The positions after each root's move (a pass included), on the device."""
    b, t = dev(boards, turn)
    st = ops.step(b, t, torch.from_numpy(np.array(move, np.uint8)).cuda())
    assert bool((st.ret >= 0).all())
    return ops.to_numpy_u64(st.boards).reshape(-1, 2), st.turn.cpu().numpy()


def assert_images_agree(v, m, s, boards, turn, again, what, status):
    """One value per root over its 16 images; each image's move, played, leaves
    a position that `again` values at minus that."""
    assert (s == status).all(), (what, s)
    v16 = v.reshape(-1, 16)
    assert (v16 == v16[:, :1]).all(), (what, v16)
    go = m != 255
    assert go.any()
    cb, ct = after_the_move(boards[go], turn[go], m[go])
    cv, _, cs = again(cb, ct)
    assert (cs == status).all() and (cv == -v[go]).all(), (what, np.nonzero(cv != -v[go])[0][:8])


@functools.lru_cache(maxsize=None)
def image_roots(family, e, k):
    b, t = sc.FAMILIES[family](e)
    return sc.images(b[:k], t[:k])[:2]


def test_the_eval_is_the_same_on_all_16_images():
    """What the value comparisons below rely on (tests/test_synthetic_cases.py
    has it for more boards): symmetric region masks, and an eval taken from the
    root mover's side, who changes colour with the board."""
    ib, it = image_roots("uniform", 30, 8)
    for w in sc.TABLES.values():
        ev = oracle.evaluate(ib, it, w).reshape(8, 16)
        assert (ev == ev[:, :1]).all()


@pytest.mark.parametrize("e", [10, 11])
@pytest.mark.parametrize("family", ["uniform", "lopsided", "centre"])
def test_solve_is_the_same_on_all_16_images(family, e):
    """8 roots at 10 empties, 4 at 11: one lane solves one image and the launch
    lasts as long as its hardest; 8 centre roots at 11 took 5 s."""
    b, t = image_roots(family, e, 8 if e == 10 else 4)
    v, m, s = gpu_solve(b, t)
    assert_images_agree(v, m, s, b, t, gpu_solve, (family, e), SOLVED)


def test_split_solve_is_the_same_on_all_16_images():
    b, t = image_roots("uniform", 13, 4)
    split = functools.partial(gpu_solve, max_empties=16, task_empties=8, order=1)
    v, m, s = split(b, t)
    assert_images_agree(v, m, s, b, t, split, "13 empties", SOLVED)


def test_search_and_split_search_are_the_same_on_all_16_images():
    b, t = image_roots("uniform", 30, 8)
    lane = gpu_search(b, t, 6, "default")
    assert (lane[2] == SEARCHED).all()
    assert (lane[0].reshape(-1, 16) == lane[0].reshape(-1, 16)[:, :1]).all()
    # the split search where both are defined: depth 6, the same answers move for move
    same(gpu_search(b, t, 6, "default", split=2), lane[:2], "depth 6, split 2", SEARCHED)
    deep = gpu_search(b, t, 8, "default", split=2, order=1)
    assert (deep[2] == SEARCHED).all()
    assert (deep[0].reshape(-1, 16) == deep[0].reshape(-1, 16)[:, :1]).all()


# ---------------------------------------------------------------- root windows and win/draw/loss on batch X
NAM, NAM32 = moves_ref.NOT_A_MOVE, moves_ref.NOT_A_MOVE32


def window_solve(rows=slice(None), **kw):
    """gpu_window.solve's (value, move, status, nodes) of x_windows()'s rows under their own windows."""
    w = sc.x_windows()
    return gpu_window.solve(w["boards"][rows], w["turn"][rows], w["alpha"][rows], w["beta"][rows],
                            node_limit=NODE_LIMIT, **kw)


def check_windows(**kw):
    """Every pair in one launch; wld=True against the wld family; the full family is the call without a window."""
    w = sc.x_windows()
    b, t = sc.batch_x()
    assert len(w["turn"]) == 3582
    got = window_solve(**kw)
    gpu_window.assert_same(got, (w["value"], w["move"]), ("windows", kw))
    wld, full = sc.x_family("wld"), sc.x_family("full")
    assert (w["root"][wld] == np.arange(len(t))).all() and (w["root"][full] == np.arange(len(t))).all()
    gpu_window.assert_same(gpu_window.solve(b, t, node_limit=NODE_LIMIT, wld=True, **kw),
                           (w["value"][wld], w["move"][wld]), ("wld", kw))
    plain = gpu_window.solve(b, t, node_limit=NODE_LIMIT, **kw)
    for k, (x, y) in enumerate(zip(got, plain)):
        if k < 3 or "task_empties" not in kw:  # (the split solver's node counts depend on the tasks' timing)
            assert (x[full] == y).all(), ("full", kw, k)
    return got, plain


def test_windows_on_batch_x_in_one_launch():
    got, plain = check_windows()
    # a narrower window searches a subtree of the full window's
    assert (got[3] <= plain[3][sc.x_windows()["root"]]).all()
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3])
def test_split_windows_on_batch_x(task_empties, order):
    for slab in (_lib.SOLVE_TREE_DEFAULT_NODES, _lib.SOLVE_TREE_MIN_NODES):
        check_windows(task_empties=task_empties, order=order, nodes_per_position=slab)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- the value of every root move
def check_exact_rows(got, what):
    b, t = sc.batch_x()
    want = sc.x_moves()
    gpu_moves.assert_rows(got, want, SOLVED, what)
    rows, value, move, st, nodes = got
    forced, over = sc.root_kinds(b, t)
    assert (nodes >= np.maximum((want[0] != NAM).sum(axis=1), want[2] == 64)).all(), what  # a task a move, one for a pass
    assert (nodes[over] == 0).all() and (rows[forced | over] == NAM).all(), what


@pytest.mark.parametrize("max_empties", [8, 12])
def test_exact_rows_on_batch_x(max_empties):
    """max_empties = 8: 8 task slots a position, and the roots of 8 empties with 8 moves fill the last."""
    b, t = sc.batch_x()
    check_exact_rows(gpu_moves.gpu_solve_moves(b, t, max_empties=max_empties, node_limit=NODE_LIMIT), max_empties)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("npp", [64, 4096])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3])
def test_split_exact_rows_on_batch_x(task_empties, order, npp):
    b, t = sc.batch_x()
    got = gpu_moves.gpu_solve_moves(b, t, max_empties=8, node_limit=NODE_LIMIT, task_empties=task_empties, order=order,
                                    nodes_per_position=npp)
    check_exact_rows(got, (task_empties, order, npp))
    assert ops.work_word("cuda").item() == 0


def test_split_exact_rows_with_a_16_entry_table_on_batch_x():
    b, t = sc.batch_x()
    table = ops.SolveTable(4)
    got = gpu_moves.gpu_solve_moves(b, t, max_empties=8, node_limit=NODE_LIMIT, task_empties=3, order=1,
                                    nodes_per_position=64, table=table, hash_min_empties=1)
    check_exact_rows(got, "table")
    assert int((table.data != 0).sum()) > 0  # the table was used
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("depth,table", sc.S_RUNS)
def test_search_rows_on_batch_s(depth, table):
    b, t = sc.batch_s()
    w = sc.TABLES[table]
    got = gpu_moves.gpu_search_moves(b, t, depth, w, node_limit=NODE_LIMIT)
    gpu_moves.assert_rows(got, sc.s_moves(depth, table), SEARCHED, (depth, table))
    _, over = sc.root_kinds(b, t)
    assert (got[4][over] == 0).all() and (got[0][over] == NAM32).all()
    gpu_moves.assert_is_ops_search(b, t, depth, w, got)
    assert ops.work_word("cuda").item() == 0


def test_search_rows_of_batch_s_tiled_nine_times_in_a_permuted_order():
    """1,116 positions, up to 34 tasks each: several blocks of the expand kernel pack their tasks through the one
    counter, and row i must be the row of the position it is a copy of."""
    b, t = sc.batch_s()
    idx = np.random.default_rng([sc.SEED, 7]).permutation(9 * len(t)) % len(t)
    assert len(idx) == 1116 and (np.bincount(idx) == 9).all()
    got = gpu_moves.gpu_search_moves(b[idx], t[idx], 3, sc.TABLES["default"], node_limit=NODE_LIMIT)
    gpu_moves.assert_rows(got, tuple(x[idx] for x in sc.s_moves(3, "default")), SEARCHED, "tiled")
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- the principal variation
def check_line(got, want, b, t, what, weights=None, scale=1, status=SOLVED):
    assert (got["status"] == status).all(), what
    same_line(got, want, what, scale=scale)
    gpu_line.assert_padded(got)
    gpu_line.assert_replays(b, t, got, weights)


def test_exact_lines_on_batch_x():
    """A third of these lines hold a pass, 51 end with an empty square left."""
    b, t = sc.batch_x()
    got = gpu_line.gpu_solve_line(b, t, node_limit=NODE_LIMIT)
    check_line(got, sc.x_line(), b, t, "batch X")
    forced, over = sc.root_kinds(b, t)
    assert (got["line"][forced, 0] == 64).all() and (got["length"][over] == 0).all()
    assert (got["best_move"][over] == 255).all() and (got["nodes"][over] == 0).all()
    v, m, s = gpu_solve(b, t)
    assert (got["value"] == v).all() and (got["best_move"] == m).all() and (got["status"] == s).all()
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("depth,table", sc.S_RUNS)
def test_search_lines_on_batch_s(depth, table, order):
    b, t = sc.batch_s()
    w = sc.TABLES[table]
    got = gpu_line.gpu_search_line(b, t, depth, w, order=order, node_limit=NODE_LIMIT)
    check_line(got, sc.s_line(depth, table), b, t, (depth, table, order), w, status=SEARCHED)
    v, m, s = gpu_search(b, t, depth, table, order=order)
    assert (got["value"] == v).all() and (got["best_move"] == m).all() and (got["status"] == s).all()
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
def test_search_lines_with_a_depth_per_position_on_batch_s(order):
    b, t = sc.batch_s()
    depths = per_position_depths(b)
    w = sc.TABLES["default"]
    got = gpu_line.gpu_search_line(b, t, torch.from_numpy(depths.astype(np.uint8)).cuda(), w, order=order,
                                   node_limit=NODE_LIMIT)
    check_per_position(got, b, t, depths, w)
    gpu_line.assert_padded(got)
    gpu_line.assert_replays(b, t, got, w, rows=got["status"] == SEARCHED)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("name", sc.FULL_DEPTH_CASES)
def test_full_depth_rows_and_lines_are_the_exact_ones_times_t(name):
    b, t, line, exact = sc.full_depth_case(name)
    for table in sc.ALL_TABLES:
        w = sc.TABLES[table]
        got = gpu_moves.gpu_search_moves(b, t, sc.FULL_DEPTH, w, node_limit=NODE_LIMIT)
        gpu_moves.assert_rows(got, sc.exact_rows_times_t(*exact), SEARCHED, (name, table))
        for order in (0, 1):
            got = gpu_line.gpu_search_line(b, t, sc.FULL_DEPTH, w, order=order, node_limit=NODE_LIMIT)
            check_line(got, line, b, t, (name, table, order), w, scale=T, status=SEARCHED)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- the edges, by name
def test_rows_and_lines_on_the_edges():
    b, t, names = sc.edges()
    rows, value, move, st, nodes = gpu_moves.gpu_solve_moves(b, t, node_limit=NODE_LIMIT)
    ln = gpu_line.gpu_solve_line(b, t, node_limit=NODE_LIMIT)
    w = sc.TABLES["extreme"]
    srows, svalue, smove, sst, snodes = gpu_moves.gpu_search_moves(b, t, 3, w, node_limit=NODE_LIMIT)
    sln = gpu_line.gpu_search_line(b, t, 3, w, node_limit=NODE_LIMIT)
    gpu_line.assert_padded(ln), gpu_line.assert_padded(sln)
    assert (sst == SEARCHED).all() and (sln["status"] == SEARCHED).all()
    assert (ln["value"] == value).all() and (ln["best_move"] == move).all() and (ln["status"] == st).all()
    assert (sln["value"] == svalue).all() and (sln["best_move"] == smove).all()
    for (name, turn), v in {("full black", 1): 64, ("full black", 2): -64, ("full white", 1): -64, ("full white", 2): 64,
                            ("full 63:1", 1): 62, ("full 63:1", 2): -62, ("full 32:32", 1): 0,
                            ("full 32:32", 2): 0}.items():
        i = sc.edge(name, turn)
        assert (value[i], move[i], st[i], nodes[i]) == (v, 255, SOLVED, 0) and (rows[i] == NAM).all(), (name, turn)
        assert (ln["length"][i], ln["value"][i]) == (0, v) and (ln["end_boards"][i] == b[i]).all(), (name, turn)
        assert (svalue[i], smove[i], snodes[i]) == (v * T, 255, 0) and (srows[i] == NAM32).all(), (name, turn)
        assert (sln["length"][i], sln["value"][i]) == (0, v * T), (name, turn)
    i = sc.edge("wipe-out", 1)  # a1 takes White's only disc; h1 stays empty for ever
    assert (rows[i] != NAM).sum() == 1 and rows[i, 0] == 63 and (value[i], move[i], st[i]) == (63, 0, SOLVED)
    assert ln["length"][i] == 1 and ln["line"][i, 0] == 0 and ln["value"][i] == 63
    assert int(ln["end_boards"][i, 0] | ln["end_boards"][i, 1]) == sc.FULL ^ (1 << 7)
    assert (srows[i] != NAM32).sum() == 1 and srows[i, 0] == 63 * T and sln["line"][i, :2].tolist() == [0, 255]
    i = sc.edge("pass then the last move", 1)
    assert (rows[i] == NAM).all() and move[i] == 64 and st[i] == SOLVED and nodes[i] >= 1
    assert ln["length"][i] == 2 and ln["line"][i, :3].tolist() == [64, 0, 255]
    assert (srows[i] == NAM32).all() and smove[i] == 64 and sln["line"][i, :3].tolist() == [64, 0, 255]
    assert svalue[i] == T * int(value[i])
    for turn in (1, 2):
        i = sc.edge("four unplayable empties", turn)
        v = (3 - 57) * (1 if turn == 1 else -1)
        assert (value[i], move[i], st[i], nodes[i]) == (v, 255, SOLVED, 0) and (rows[i] == NAM).all()
        assert ln["length"][i] == 0 and (ln["end_boards"][i] == b[i]).all()
        assert (svalue[i], smove[i], snodes[i], sln["length"][i]) == (v * T, 255, 0, 0)
        for name in ("empty", "one disc"):
            i = sc.edge(name, turn)
            assert (value[i], move[i], st[i], nodes[i]) == (0, 255, SKIPPED, 0) and (rows[i] == NAM).all(), name
            assert (ln["length"][i], ln["status"][i], ln["nodes"][i]) == (0, SKIPPED, 0) and (ln["line"][i] == 255).all()
            d = (0 if name == "empty" else 1) * (1 if turn == 1 else -1)
            assert (svalue[i], smove[i], snodes[i]) == (d * T, 255, 0) and (srows[i] == NAM32).all(), name
            assert (sln["length"][i], sln["value"][i], sln["nodes"][i]) == (0, d * T, 0), name
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- beyond the checkers: rows, lines and windows
@functools.lru_cache(maxsize=None)
def image_roots_with_perm(family, e, k):
    b, t = sc.FAMILIES[family](e)
    return sc.images(b[:k], t[:k])


def assert_rows_permute(rows, perm, what):
    """An image's row taken back through its permutation is the same for all 16 images of a root."""
    home = np.take_along_axis(rows, perm, 1).reshape(-1, 16, 64)
    assert (home == home[:, :1]).all(), (what, np.nonzero((home != home[:, :1]).any(axis=(1, 2)))[0])


def assert_rows_are_solves(got, b, t, solve, what):
    """Every legal entry is minus `solve` of the child ops.step makes, the row's maximum `solve`'s value of the
    root and its lowest maximiser `solve`'s move."""
    rows, value, move, st, _ = got
    assert (st == SOLVED).all(), what
    legal = rows != NAM
    assert (legal.sum(axis=1) == sc.popcount(oracle.legal(b, t))).all(), what
    ci, csq = np.nonzero(legal)
    cb, ct = after_the_move(b[ci], t[ci], csq)
    cv, _, cs = solve(cb, ct)
    assert (cs == SOLVED).all() and (rows[ci, csq] == -cv).all(), what
    rv, rm, rs = solve(b, t)
    assert (rs == SOLVED).all() and (value == rv).all() and (move == rm).all(), what
    has = legal.any(axis=1)
    assert has.sum() >= len(t) // 2, what
    assert (rows[has].max(axis=1) == rv[has]).all() and (rows[has].argmax(axis=1) == rm[has]).all(), what


@pytest.mark.parametrize("family,e,k", [("uniform", 10, 8), ("centre", 11, 4)])
def test_exact_rows_permute_with_the_images_and_are_the_solves_they_replace(family, e, k):
    b, t, perm = image_roots_with_perm(family, e, k)
    got = gpu_moves.gpu_solve_moves(b, t, node_limit=NODE_LIMIT)
    assert_rows_permute(got[0], perm, (family, e))
    assert_rows_are_solves(got, b, t, gpu_solve, (family, e))


def test_split_exact_rows_permute_with_the_images_and_are_the_solves_they_replace():
    b, t, perm = image_roots_with_perm("uniform", 13, 4)
    kw = dict(max_empties=16, task_empties=8, order=1)
    got = gpu_moves.gpu_solve_moves(b, t, node_limit=NODE_LIMIT, **kw)
    assert_rows_permute(got[0], perm, "13 empties")
    assert_rows_are_solves(got, b, t, functools.partial(gpu_solve, **kw), "13 empties")


def test_search_rows_permute_with_the_images_and_their_maximum_is_the_search():
    """(The entries are not minus ops.search of the children: that call scores the leaves from the child's
    mover's side, and the eval is not antisymmetric.)"""
    b, t, perm = image_roots_with_perm("uniform", 30, 8)
    rows, value, move, st, _ = gpu_moves.gpu_search_moves(b, t, 5, sc.TABLES["default"], node_limit=NODE_LIMIT)
    assert (st == SEARCHED).all()
    assert_rows_permute(rows, perm, "depth 5")
    assert ((rows != NAM32).sum(axis=1) == sc.popcount(oracle.legal(b, t))).all()
    v, m, s = gpu_search(b, t, 5, "default")
    assert (s == SEARCHED).all() and (value == v).all() and (move == m).all()
    assert (rows.max(axis=1) == v).all() and (rows.argmax(axis=1) == m).all()  # (every root here has a move)


@pytest.mark.parametrize("family,e,k", [("uniform", 10, 8), ("centre", 11, 2)])
def test_exact_lines_on_the_images_hold_ops_solves_move_at_every_ply(family, e, k):
    """(2 centre roots at 11 empties: a launch lasts as long as its hardest lane, the first root's 2.1 M nodes,
    and this test has two such launches, the walk and ops.solve of every prefix position; with the 4 roots of
    the other image tests and a third launch, ops.solve of the roots, it took 7.9 s.)"""
    b, t, _ = image_roots_with_perm(family, e, k)
    got = gpu_line.gpu_solve_line(b, t, node_limit=NODE_LIMIT)
    assert (got["status"] == SOLVED).all() and (got["length"] > 0).all()
    gpu_line.assert_padded(got)
    gpu_line.assert_replays(b, t, got)
    # ops.solve of every prefix position, the root (the one in front of entry 0) included: plus or minus the
    # value, and the lowest best move holds at every ply
    (pi, pk, pb, pt), _, _ = gpu_line.replay(b, t, got)
    pv, pm, ps = gpu_solve(pb, pt)
    sign = np.where(pt == solve_ref.mover(t)[pi], 1, -1)
    assert (ps == SOLVED).all() and (pv == sign * got["value"][pi]).all() and (pm == got["line"][pi, pk]).all()
    assert len(pi) == got["length"].sum() and got["length"].max() >= e - 2
    root = pk == 0
    assert (pi[root] == np.arange(len(t))).all() and (pb[root] == b).all()
    assert (got["best_move"] == pm[root]).all() and (got["value"] == pv[root]).all()
    v16 = got["value"].reshape(-1, 16)
    assert (v16 == v16[:, :1]).all()


def test_search_lines_on_the_images_are_ops_searchs():
    b, t, _ = image_roots_with_perm("uniform", 30, 8)
    w = sc.TABLES["default"]
    got = gpu_line.gpu_search_line(b, t, 6, w, node_limit=NODE_LIMIT)
    assert (got["status"] == SEARCHED).all() and (got["length"] >= 6).all()
    gpu_line.assert_padded(got)
    gpu_line.assert_replays(b, t, got, w)
    v, m, s = gpu_search(b, t, 6, "default")
    assert (s == SEARCHED).all() and (got["value"] == v).all() and (got["best_move"] == m).all()
    assert (v.reshape(-1, 16) == v.reshape(-1, 16)[:, :1]).all()


def test_windows_at_10_empties_against_the_rows():
    """4 roots, 64 images: window_ref.expect over the GPU's own rows (which the tests above tie to ops.solve of
    every child), one lane and split."""
    b, t, _ = image_roots_with_perm("uniform", 10, 8)
    b, t = b[:64], t[:64]
    rows, value, move, st, _ = gpu_moves.gpu_solve_moves(b, t, node_limit=NODE_LIMIT)
    assert (st == SOLVED).all()
    ci, csq = np.nonzero(rows != NAM)
    forced, over = sc.root_kinds(b, t)
    r = window_ref.Roots(len(t), value, ~forced & ~over, forced, ci, csq, rows[ci, csq])
    assert ((rows != NAM).any(axis=1) == r.has).all()
    for name in ("wld", "around") + window_ref.ON_BOUND:
        lo, hi, keep = window_ref.family(name, value)
        assert keep.all()
        want = window_ref.expect(r, lo, hi)
        kw = dict(wld=True) if name == "wld" else dict(alpha=lo, beta=hi)
        gpu_window.assert_same(gpu_window.solve(b, t, node_limit=NODE_LIMIT, **kw), want, name)
        gpu_window.assert_same(gpu_window.solve(b, t, node_limit=NODE_LIMIT, task_empties=6, order=1, **kw), want,
                               (name, "split"))
    assert ops.work_word("cuda").item() == 0
