"""The five search entry points on the GPU (ops.solve, ops.solve(task_empties=),
ops.search, ops.search(split=), ops.play) on the positions of
tests/synthetic_cases.py, which no game from the opening reaches: every value,
best move and status against the exhaustive checkers (tests/solve_ref.py,
search_ref.py, play_ref.py), node counts never; then what no checker reaches,
by symmetry: a root's 16 images have one value, and an image's best move leads
to a position worth minus that.

NODE_LIMIT is 2**22 throughout: a defect ends as LIMIT, which every comparison
refuses, not as a long kernel.  runner.do_matches(policy="search") takes no start
positions, so it is not run here."""
import functools

import numpy as np
import pytest
import torch

import oracle
import play_ref
import search_ref
import solve_ref
import synthetic_cases as sc
import tree_cases

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
