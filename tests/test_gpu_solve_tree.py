"""ops.solve(task_empties=...) / othe_solve on the GPU: every value and move
against the exhaustive checker (tests/solve_ref.py) at 0..9 empties, forced
passes and game-overs inside the expanded plies; value, move and status bit for
bit against the one-lane solver (oths_solve) at 10 and 12 empties; against the
deep fixture (tests/golden/solve_deep/solve_deep.npz, a plain recursive alpha-beta's
answers) at 13..16 empties; NOROOM exactly where the header's rule says; ties;
independence of the grid; the node limit and the work word; the engine.

Every comparison asserts status == SOLVED for every root that is not expected
to end as NOROOM: a LIMIT or NOROOM that was not expected is a failure."""
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import oracle
import order_cases
import solve_cases
import solve_ref
import tree_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, codec, engine, ops  # noqa: E402

SKIPPED, SOLVED, INVALID, LIMIT = _lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
NOROOM = _lib.SOLVE_TREE_NOROOM
FULL = (1 << 64) - 1
# per task; the largest task here (12 empties, unordered) needs 2.3 M nodes in the one-lane solver's own
# measurements: a defect ends as LIMIT, which every test below refuses
NODE_LIMIT = 1 << 26
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(boards, turn):
    return (ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda"),
            torch.from_numpy(np.array(turn, np.uint8)).cuda())


def tree_solve(boards, turn, task_empties, order, max_empties=16, node_limit=NODE_LIMIT, **kw):
    b, t = dev(boards, turn)
    r = ops.solve(b, t, max_empties=max_empties, node_limit=node_limit, task_empties=task_empties, order=order, **kw)
    torch.cuda.synchronize()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def lane_solve(e, k):
    """The one-lane solver's answers on solve_cases.ladder(e, k)."""
    b, t = solve_cases.ladder(e, k)
    assert len(t) == k and (solve_ref.empties(b) == e).all()
    bt, tt = dev(b, t)
    r = ops.solve(bt, tt, max_empties=e, node_limit=NODE_LIMIT)
    torch.cuda.synchronize()
    out = (b, t, r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz"))
    out = (fx["boards"], fx["turn"], fx["value"].astype(np.int64), fx["best_move"], fx["empties"].astype(np.int64))
    for a in out:
        a.setflags(write=False)
    return out


def assert_same(got, want, what):
    (v, m, s), (rv, rm) = got, want
    assert (s == SOLVED).all(), (what, np.nonzero(s != SOLVED)[0][:8], s[s != SOLVED][:8])
    bad = np.nonzero((v != rv) | (m != rm))[0]
    assert len(bad) == 0, (what, bad[:8], v[bad[:8]], rv[bad[:8]], m[bad[:8]], rm[bad[:8]])


# ---------------------------------------------------------------- 1. the checker
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3, 6])
def test_matches_the_checker_at_0_to_9_empties(task_empties, order):
    cases = solve_cases.cases()
    assert sorted(cases) == list(range(10))
    assert sum(int(c["forced_pass"].sum()) for c in cases.values()) > 0
    assert sum(int(c["over"].sum()) for e, c in cases.items() if e > 0) > 0
    for e, c in sorted(cases.items()):
        # (4,096 nodes a root: at 9 empties and one-empty tasks the deepest levels do not fit and the tasks start
        # higher, which is part of what is compared)
        got = tree_solve(c["boards"], c["turn"], task_empties, order, nodes_per_position=4096)
        assert_same(got, (c["value"], c["best_move"]), (e, task_empties, order))
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 2. the one-lane solver
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [4, 8, 12])
@pytest.mark.parametrize("e,k", [(10, 64), (12, 16)])
def test_equals_the_one_lane_solver(e, k, task_empties, order):
    b, t, rv, rm, rs = lane_solve(e, k)
    assert (rs == SOLVED).all()
    v, m, s = tree_solve(b, t, task_empties, order, max_empties=e)
    assert (s == rs).all()
    assert_same((v, m, s), (rv, rm), (e, task_empties, order))


# ---------------------------------------------------------------- 3. the fixture
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [8, 10, 12])
def test_matches_the_fixture_at_13_to_16_empties(task_empties, order):
    b, t, rv, rm, emp = fixture()
    assert len(t) == 38 and emp.min() == 13 and emp.max() == 16
    assert_same(tree_solve(b, t, task_empties, order), (rv, rm), (task_empties, order))
    assert ops.work_word("cuda").item() == 0


def test_one_batch_mixed_with_skipped_and_invalid_roots():
    b, t, rv, rm, _ = fixture()
    pool = solve_cases.pool()
    deep_b = np.concatenate([pool[17]["boards"][:3], pool[20]["boards"][:2], pool[40]["boards"][:1]])
    deep_t = np.concatenate([pool[17]["turn"][:3], pool[20]["turn"][:2], pool[40]["turn"][:1]])
    bad_b = np.array([[FULL ^ 0xF, 0x10]], np.uint64)  # overlaps on square 4
    boards = np.concatenate([deep_b[:3], b[:20], bad_b, deep_b[3:], b[20:]])
    turn = np.concatenate([deep_t[:3], t[:20], [1], deep_t[3:], t[20:]]).astype(np.uint8)
    kind = np.concatenate([np.full(3, SKIPPED), np.full(20, SOLVED), [INVALID], np.full(3, SKIPPED), np.full(18, SOLVED)])
    bt, tt = dev(boards, turn)
    r = ops.solve(bt, tt, max_empties=16, node_limit=NODE_LIMIT, task_empties=10, order=1, want_nodes=True)
    torch.cuda.synchronize()
    v, m, s = r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()
    nd = r.nodes.cpu().numpy().view(np.uint32)
    assert (s == kind).all(), (s, kind)
    assert (v[kind == SOLVED] == rv).all() and (m[kind == SOLVED] == rm).all()
    assert (v[kind != SOLVED] == 0).all() and (m[kind != SOLVED] == 255).all() and (nd[kind != SOLVED] == 0).all()
    assert (nd[kind == SOLVED] > 0).all()
    assert ops.work_word("cuda").item() == 0
    # max_empties is a filter of its own: at 14 the deeper fixture roots are skipped too
    v, m, s = tree_solve(b, t, 10, 1, max_empties=14)
    emp = fixture()[4]
    assert (s == np.where(emp <= 14, SOLVED, SKIPPED)).all()
    assert (v == np.where(emp <= 14, rv, 0)).all() and (m == np.where(emp <= 14, rm, 255)).all()


# ---------------------------------------------------------------- 4. NOROOM and small slabs
def expected_noroom(boards, turn, task_empties, slab):
    """Which roots must end as OTHE_NOROOM, by include/othello_solve_tree.h's
    rule stated over the oracle alone: the tree grows a whole level at a time
    (the children of every node of the last level that is not final and is the
    root or has more than task_empties empties; a node that must pass has one
    child, the same board), a level that does not fit `slab` nodes is not made,
    and the root has no room when a node left unexpanded, not final, has more
    than 12 empties."""
    out = np.zeros(len(turn), bool)
    for i in range(len(turn)):
        b = np.asarray(boards[i:i + 1], np.uint64)
        t = solve_ref.mover(turn[i:i + 1])
        used, root = 1, True
        pending = np.zeros(0, np.int64)  # empties of the nodes that stay tasks
        while True:
            own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
            emp = solve_ref.empties(b)
            final = (own == 0) & (opp == 0)
            grow = ~final & ((emp > task_empties) | root)
            pending = np.concatenate([pending, emp[~final & ~grow]])
            passes = grow & (own == 0)
            idx, sq = solve_ref._bits(np.where(grow, own, np.uint64(0)))
            total = len(idx) + int(passes.sum())
            if total == 0 or used + total > slab:
                pending = np.concatenate([pending, emp[grow]])
                break
            kids = oracle.step(b[idx], t[idx], sq)["boards"]
            pi = np.nonzero(passes)[0]
            b, t = np.concatenate([kids, b[pi]]), np.concatenate([3 - t[idx], 3 - t[pi]]).astype(np.uint8)
            used += total
            root = False
        out[i] = (pending > 12).any()
    return out


@pytest.mark.parametrize("slab", [64, 1024])
def test_no_room_exactly_where_a_task_would_have_more_than_12_empties(slab):
    """64 nodes hold the root's level and at times one more; 1,024 two or three
    levels: not enough for every root above 13 empties."""
    b, t, rv, rm, emp = fixture()
    want = expected_noroom(b, t, 10, slab)
    assert 0 < want.sum() < len(t), want.sum()
    assert not want[emp == 13].any()  # the root's level always fits, and leaves 12
    assert not expected_noroom(b, t, 10, _lib.SOLVE_TREE_DEFAULT_NODES).any()
    v, m, s = tree_solve(b, t, 10, 1, nodes_per_position=slab)
    assert (s == np.where(want, NOROOM, SOLVED)).all(), (s, want)
    assert (v[want] == 0).all() and (m[want] == 255).all()
    # the others' tasks started higher: the same answers
    assert (v[~want] == rv[~want]).all() and (m[~want] == rm[~want]).all()
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 5. ties
def test_two_empties_ties_keep_the_lower_square():
    b, t, _, rm, later = order_cases.two_empties()
    assert later.sum() >= 1
    rv, rm2, _ = solve_ref.solve(b, t)
    assert (rm2 == rm).all()
    assert_same(tree_solve(b, t, 1, 1), (rv, rm), "two empties")
    assert_same(tree_solve(b, t, 2, 1), (rv, rm), "two empties, one level")


def test_the_eight_images_of_a_root_keep_their_own_lowest_maximiser():
    """A root and its images under the square's symmetries tie wherever it
    does, and each image's lowest maximiser is its own: against the one-lane
    solver, whose ascending order gives it for free."""
    b, t = solve_cases.ladder(10, 8)
    ib = np.array([[bb, ww] for k in range(8) for bb, ww in
                   zip(tree_cases.symmetries(int(b[k, 0])), tree_cases.symmetries(int(b[k, 1])))], np.uint64)
    it = np.repeat(t, 8)
    bt, tt = dev(ib, it)
    r = ops.solve(bt, tt, max_empties=10, node_limit=NODE_LIMIT)
    torch.cuda.synchronize()
    rv, rm = r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy()
    assert (r.status.cpu().numpy() == SOLVED).all()
    assert (rv.reshape(8, 8) == rv.reshape(8, 8)[:, :1]).all()
    assert max(len(set(row.tolist())) for row in rm.reshape(8, 8)) > 1
    for task_empties in (6, 9):
        assert_same(tree_solve(ib, it, task_empties, 1), (rv, rm), task_empties)


# ---------------------------------------------------------------- 6. timing independence
def test_the_grid_does_not_change_an_answer(monkeypatch):
    b, t, rv, rm, rs = lane_solve(10, 64)
    lib = _lib.load()
    assert lib.othe_solve_grid(1000) == 16
    full = tree_solve(b, t, 6, 1, max_empties=10)
    got = {}
    for blocks in ("1", "4"):
        monkeypatch.setenv("OTH_SOLVE_BLOCKS", blocks)
        assert lib.othe_solve_grid(1000) == int(blocks)
        got[blocks] = tree_solve(b, t, 6, 1, max_empties=10) + tree_solve(b, t, 6, 0, max_empties=10)
        assert ops.work_word("cuda").item() == 0
    for v, m, s in (full, got["1"][:3], got["1"][3:], got["4"][:3], got["4"][3:]):
        assert (s == rs).all()
        assert_same((v, m, s), (rv, rm), "grid")


# ---------------------------------------------------------------- 7. the node limit and the work word
def test_node_limit_one_ends_every_root_as_limit():
    """12 empties, tasks of 10: a position's first tasks start with the full
    window (no best is known yet), and a task with 10 empties makes at least
    two placements: its first node is allowed, its second is not.  The limit
    bit is sticky on the way up, so the root ends as LIMIT."""
    b, t, rv, rm, rs = lane_solve(12, 16)
    for order in (0, 1):
        v, m, s = tree_solve(b, t, 10, order, max_empties=12, node_limit=1)
        assert (s == LIMIT).all() and (v == 0).all() and (m == 255).all()
        assert ops.work_word("cuda").item() == 0


def test_failed_calls_leave_the_work_word_zero():
    b, t, rv, rm, rs = lane_solve(10, 64)
    bt, tt = dev(b, t)
    for bad in (dict(max_empties=17), dict(task_empties=0), dict(task_empties=13), dict(order=2),
                dict(nodes_per_position=63)):
        kw = dict(max_empties=10, task_empties=6, order=0)
        kw.update(bad)
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.solve(bt, tt, **kw)
        torch.cuda.synchronize()
        assert ops.work_word("cuda").item() == 0
    # the call as it was keeps its own limits
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.solve(bt, tt, max_empties=13)
    with pytest.raises(ValueError):
        ops.solve(bt, tt, max_empties=10, order=1)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r = ops.solve(bt, tt, max_empties=10, node_limit=NODE_LIMIT, task_empties=6, order=1, work=w, want_nodes=True)
    g = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert w.item() == 0 and ops.work_word("cuda").item() == 0
    assert_same((r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()), (rv, rm),
                "own work word")
    assert r.value.dtype == torch.int8 and r.nodes.dtype == torch.int32
    assert int(g.hist.sum().item()) > 0
    e = ops.solve(bt[:0], tt[:0], max_empties=10, task_empties=6, want_nodes=True)
    assert e.value.numel() == e.status.numel() == e.nodes.numel() == 0


def test_env_solve_takes_task_empties():
    from subproc_amd.env import VecEnv

    b, t, rv, rm, rs = lane_solve(10, 64)
    env = VecEnv(len(t), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(b), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(t)).cuda())
    r = env.solve(max_empties=10, node_limit=NODE_LIMIT, task_empties=6, order=1)
    torch.cuda.synchronize()
    assert (r.status.cpu().numpy() == SOLVED).all()
    assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()


# ---------------------------------------------------------------- 8. the engine
def test_engine_plays_the_fixtures_move_at_14_empties(monkeypatch, capsys):
    b, t, rv, rm, emp = fixture()
    i = int(np.nonzero((emp == 14) & (rm < 64))[0][0])
    eng = engine.Engine(name="S", policy="greedy", solve_empties=14, solve_task_empties=10)
    text = oracle.serialize_str(b[i, 0], b[i, 1], t[i])
    eng.board.deserialize(text[:64], text[65], 0)
    assert eng.board.bitboards() == (int(b[i, 0]), int(b[i, 1])) and eng.board.turn == int(t[i])
    out = []
    eng.handle("go", out.append)
    assert codec.parse_engine_go("".join(out))[1] == int(rm[i])
    # the line names the new settings after solve_empties=, and only when they are set
    out = []
    eng.handle("verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=14 solve_task_empties=10"]
    out = []
    engine.Engine(name="S", policy="greedy", solve_empties=16, solve_task_empties=12, order=1).handle(
        "verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=16 solve_task_empties=12 solve_order=1"]
    out = []
    engine.Engine(name="S", policy="greedy", solve_empties=12, solve_task_empties=8, order=1, solve_order=0).handle(
        "verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=12 solve_task_empties=8"]
    out = []
    engine.Engine(name="S", policy="greedy", solve_empties=8).handle("verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=8"]
    for bad in (dict(solve_empties=13), dict(solve_empties=17, solve_task_empties=10),
                dict(solve_empties=14, solve_task_empties=13), dict(solve_empties=14, solve_task_empties=0),
                dict(solve_empties=14, solve_task_empties=10, solve_order=2)):
        with pytest.raises(ValueError):
            engine.Engine(**bad)
    monkeypatch.setattr(sys, "stdin", io.StringIO("verbose p\nquit\n"))
    assert engine.main(["--name", "CLI", "--policy", "random", "--solve-empties", "14", "--solve-task-empties", "10",
                        "--order", "1"]) == 0
    assert capsys.readouterr().out.splitlines() == [
        "CLI policy=random solve_empties=14 solve_task_empties=10 solve_order=1", "bye"]
