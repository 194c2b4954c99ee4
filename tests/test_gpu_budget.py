"""The searches by node budget on the GPU (include/othello_budget.h, othb_*:
ops.search_budget, ops.play(budget=...), runner.do_matches(budget=...), the
engine's --nodes) against tests/budget_ref.py's loop over the existing
fixed-depth ops.search, one launch per depth under node_limit = BMAX, and
against tests/play_ref.py's game loop.  DESIGN.md §22."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import budget_ref
import oracle
import play_ref
import search_ref
import solve_cases
import synthetic_cases
import tree_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, codec, ops, runner  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMAX = 65536
LADDER = (32, 256, 2048, 16384, 65536)
CAP = 6
T = search_ref.T
FIELDS = ("value", "best_move", "status", "depth", "nodes")


def dev(boards, turn):
    return ops.from_numpy_u64(np.ascontiguousarray(boards, np.uint64), "cuda"), torch.from_numpy(
        np.ascontiguousarray(turn, np.uint8)).cuda()


def host(r):
    """A BudgetResult (or SearchResult) as numpy, the node counts as unsigned."""
    out = {k: getattr(r, k).cpu().numpy() for k in r._fields if getattr(r, k) is not None}
    if "nodes" in out:
        out["nodes"] = out["nodes"].astype(np.int64) & 0xFFFFFFFF
    return out


def fixed_depth(boards, turn, weights, order, limit=BMAX):
    """search_at(d) of the existing search: one launch per depth for the whole batch, each depth once."""
    b, t = dev(boards, turn)

    @functools.lru_cache(maxsize=None)
    def search_at(d):
        r = host(ops.search(b, t, d, weights=weights, node_limit=limit, want_nodes=True, order=order))
        return r["value"], r["best_move"], r["status"], r["nodes"]

    return search_at


def same(got, want, what):
    for k in FIELDS:
        bad = np.nonzero(np.asarray(got[k], np.int64) != np.asarray(want[k], np.int64))[0]
        assert len(bad) == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:8]], np.asarray(want[k])[bad[:8]])


@functools.lru_cache(maxsize=None)
def midgame():
    g = ops.sample_midgame(256, 0x5EED)
    b, t = ops.to_numpy_u64(g.boards), g.turn.cpu().numpy()
    b.setflags(write=False)
    t.setflags(write=False)
    return b, t


@functools.lru_cache(maxsize=None)
def few_empties():
    """(boards, turn): 8 roots at each of 1..6 empties."""
    cs = solve_cases.cases()
    return (np.concatenate([cs[e]["boards"][:8] for e in range(1, 7)]),
            np.concatenate([cs[e]["turn"][:8] for e in range(1, 7)]))


@functools.lru_cache(maxsize=None)
def other_inputs():
    """(boards, turn) beside the midgame roots: the off-tree boards, two overlapping boards, roots that must
    pass, finished games, and 1 to 6 empties."""
    sb, st = tree_cases.inputs("special3")
    passes = np.nonzero(synthetic_cases.root_kinds(sb, st)[0])[0][::43]
    cs = solve_cases.cases()  # finished games: two full boards, two with an empty square nobody can take
    done = np.nonzero(cs[1]["over"])[0][:2]
    ob = np.concatenate([cs[0]["boards"][:2], cs[1]["boards"][done]])
    ot = np.concatenate([cs[0]["turn"][:2], cs[1]["turn"][done]])
    eb, et, _ = synthetic_cases.edges()
    assert len(passes) == 4 and synthetic_cases.root_kinds(ob, ot)[1].all() and len(ot) == 4
    parts = [(b[:16], t[:16]) for b, t in (synthetic_cases.uniform(20), synthetic_cases.uniform(40),
                                           synthetic_cases.uniform(52), synthetic_cases.lopsided(8),
                                           synthetic_cases.islands(6))]
    parts += [synthetic_cases.wide(8), (eb, et)]
    parts += [(np.array([[3, 1], [1 << 63, (1 << 63) | 5]], np.uint64), np.array([1, 2], np.uint8))]
    parts += [(sb[passes], st[passes]), (ob, ot), few_empties()]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@functools.lru_cache(maxsize=None)
def parity_inputs():
    """(boards, turn, midgame rows): the 256 midgame roots first, then other_inputs()."""
    ob, ot = other_inputs()
    mb, mt = midgame()
    b, t = np.concatenate([mb, ob]), np.concatenate([mt, ot])
    b.setflags(write=False)
    t.setflags(write=False)
    return b, t, len(mt)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("table", tree_cases.BOTH)
def test_every_field_is_the_loops_over_the_fixed_depth_search(order, table):
    b, t, mid = parity_inputs()
    w = tree_cases.TABLES[table]
    db, dt = dev(b, t)
    search_at = fixed_depth(b, t, w, order)
    reached = np.zeros(CAP + 1, np.int64)
    for budget in LADDER:
        want = budget_ref.deepen(search_at, b, budget, CAP)
        got = host(ops.search_budget(db, dt, budget, max_depth=CAP, weights=w, order=order, want_nodes=True))
        same(got, want, (order, table, budget))
        assert (got["nodes"] <= budget).all()
        h = np.bincount(got["depth"][:mid], minlength=CAP + 1)
        assert (h > 0).sum() >= 2, (budget, h)  # the budget splits the midgame set
        reached += h
    # the ladder hides nothing: every depth 1..5 is where at least 5 % of the (position, budget) pairs end
    assert (reached[1:6] >= 0.05 * reached.sum()).all(), reached
    print("n_d means", {d: float(c[:mid].mean()) for d, c in want["counts"].items()}, "reached", reached.tolist())
    assert (want["status"] == budget_ref.INVALID).sum() == 2 and ops.work_word("cuda").item() == 0


def test_value_and_move_are_the_exhaustive_checkers_at_the_depth_reached():
    b, t, mid = parity_inputs()
    keep = (b[:, 0] & b[:, 1]) == 0
    for order, table, budget in ((0, "default", 256), (1, "rng7", 2048)):
        w = tree_cases.TABLES[table]
        got = host(ops.search_budget(*dev(b, t), budget, max_depth=CAP, weights=w, order=order))
        # the checker expands the unpruned tree: the first 48 midgame roots and every other board, where the
        # depth reached is at most 3 or the board has at most 8 empties
        sel = np.nonzero(keep & ((np.arange(len(t)) < 48) | (np.arange(len(t)) >= mid)) &
                         ((got["depth"] <= 3) | (budget_ref.empties(b) <= 8)) & (got["depth"] > 0))[0]
        assert len(sel) >= 100
        for d in np.unique(got["depth"][sel]):
            s = sel[got["depth"][sel] == d]
            v, m, _ = search_ref.search(b[s], t[s], int(d), w)
            assert (got["value"][s] == v).all() and (got["best_move"][s] == m).all(), (order, table, d)


@pytest.mark.parametrize("order", [0, 1])
def test_the_boundary_a_budget_of_exactly_the_nodes_completes_one_less_does_not(order):
    b, t = midgame()
    b, t = b[:64], t[:64]
    search_at = fixed_depth(b, t, None, order)
    n = np.stack([search_at(d)[3] for d in (1, 2, 3, 4)])  # the existing search's n_1..n_4
    assert (search_at(4)[2] == _lib.SEARCH_SEARCHED).all() and (n > 0).all()
    total = np.cumsum(n, axis=0)
    budgets = np.concatenate([np.concatenate([total[k], total[k] - 1]) for k in range(4)])
    bb, tt = np.tile(b, (8, 1)), np.tile(t, 8)
    got = host(ops.search_budget(*dev(bb, tt), torch.from_numpy(budgets).cuda(), max_depth=8, order=order,
                                 want_nodes=True))
    same(got, budget_ref.deepen(fixed_depth(bb, tt, None, order), bb, budgets, 8), "boundary")
    for k in range(4):
        exact, short = slice(128 * k, 128 * k + 64), slice(128 * k + 64, 128 * k + 128)
        assert (got["depth"][exact] == k + 1).all() and (got["nodes"][exact] == budgets[exact]).all(), k
        assert (got["depth"][short] == k).all(), k
        assert (got["value"][exact] == search_at(k + 1)[0]).all() and (got["best_move"][exact] == search_at(k + 1)[1]).all()
    none = slice(64, 128)  # one node short of depth 1 (a budget of 0 where n_1 == 1)
    assert (got["status"][none] == _lib.SEARCH_LIMIT).all() and (got["value"][none] == 0).all()
    assert (got["best_move"][none] == 255).all() and (got["nodes"][none] == 0).all()
    zero = host(ops.search_budget(*dev(b, t), torch.zeros(64, dtype=torch.int32, device="cuda").view(torch.uint32), order=order,
                                  want_nodes=True))
    assert (zero["status"] == _lib.SEARCH_LIMIT).all() and (zero["value"] == 0).all() and (zero["depth"] == 0).all()
    assert (zero["best_move"] == 255).all() and (zero["nodes"] == 0).all()
    # a budget of 1 on a position with two moves or more
    many = np.array([bin(int(m)).count("1") >= 2 for m in oracle.legal(b, t)])
    one = host(ops.search_budget(*dev(b, t), 1, order=order))
    assert many.sum() >= 32 and (one["status"][many] == _lib.SEARCH_LIMIT).all() and (one["depth"][many] == 0).all()
    with pytest.raises(ValueError, match="budget"):
        ops.search_budget(*dev(b, t), 0)
    with pytest.raises(_lib.OthelloCallError):
        ops.search_budget(*dev(b, t), 100, max_depth=9)
    with pytest.raises(_lib.OthelloCallError):
        ops.search_budget(*dev(b, t), 100, order=2)
    assert ops.work_word("cuda").item() == 0


def test_results_do_not_depend_on_the_batch_the_grid_or_a_replay(monkeypatch):
    b, t, _ = parity_inputs()
    n = len(t)
    budgets = np.array([LADDER[i % 5] for i in range(n)], np.int64)
    db, dt = dev(b, t)
    dbud = torch.from_numpy(budgets).cuda()
    base = host(ops.search_budget(db, dt, dbud, max_depth=CAP, want_nodes=True))
    assert ops.work_word("cuda").item() == 0
    perm = np.random.default_rng(3).permutation(n)
    p = host(ops.search_budget(*dev(b[perm], t[perm]), torch.from_numpy(budgets[perm]).cuda(), max_depth=CAP,
                               want_nodes=True))
    h = n // 3
    first = host(ops.search_budget(db[:h], dt[:h], dbud[:h], max_depth=CAP, want_nodes=True))
    assert ops.work_word("cuda").item() == 0
    second = host(ops.search_budget(db[h:], dt[h:], dbud[h:], max_depth=CAP, want_nodes=True))
    monkeypatch.setenv("OTH_BUDGET_BLOCKS", "1")
    narrow = host(ops.search_budget(db, dt, dbud, max_depth=CAP, want_nodes=True))
    assert ops.work_word("cuda").item() == 0
    monkeypatch.delenv("OTH_BUDGET_BLOCKS")
    for k in FIELDS:
        assert (p[k] == base[k][perm]).all() and (narrow[k] == base[k]).all(), k
        assert (np.concatenate([first[k], second[k]]) == base[k]).all(), k
    # a captured launch replays to the same tensors
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    u32 = dbud.to(torch.int32).view(torch.uint32)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.search_budget(db, dt, u32, max_depth=CAP)
        r = ops.search_budget(db, dt, u32, max_depth=CAP, want_nodes=True, work=w)
        s = ops.search_budget(db, dt, 2048, max_depth=CAP, order=1, work=w)
    want_s = host(ops.search_budget(db, dt, 2048, max_depth=CAP, order=1))
    for _ in range(2):
        for x in (r.value, r.best_move, r.status, r.depth, r.nodes, s.value, s.depth):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = host(r)
        assert all((got[k] == base[k]).all() for k in FIELDS) and w.item() == 0
        assert (s.value.cpu().numpy() == want_s["value"]).all() and (s.depth.cpu().numpy() == want_s["depth"]).all()
    env = VecEnv(8)
    e = env.search_budget(500, max_depth=4)
    assert torch.equal(e.best_move, ops.search_budget(env.boards, env.turn, 500, max_depth=4).best_move)


def test_the_whole_tree_at_1_to_6_empties_is_the_solvers():
    b, t = few_empties()
    emp = budget_ref.empties(b)
    solved = ops.solve(*dev(b, t), max_empties=6)
    assert (solved.status.cpu().numpy() == _lib.SOLVE_SOLVED).all()
    for order in (0, 1):
        got = host(ops.search_budget(*dev(b, t), BMAX, max_depth=8, order=order, want_nodes=True))
        assert (got["status"] == _lib.SEARCH_SEARCHED).all() and (got["depth"] == np.maximum(1, emp)).all()
        assert (got["value"] == T * solved.value.cpu().numpy().astype(np.int64)).all()
        assert (got["best_move"] == solved.best_move.cpu().numpy()).all()


# ---------------------------------------------------------------- the games

CAPS, BUDGETS = (6, 6), (512, 2048)


def budget_chooser(tables, caps, budgets, exact, order):
    """tests/play_ref.py's chooser for the budget games: the loop over the existing ops.search on the round's
    positions (the games run in lockstep, so a ply costs one launch per depth and player); one search of
    max(cap, empties) plies, without a budget, at empties <= exact."""
    def choose(boards, turn, player):
        out = np.full(len(turn), 255, np.uint8)
        emp = budget_ref.empties(boards)
        for p in (0, 1):
            for late in (False, True):
                sel = np.nonzero((player == p) & ((emp <= exact) == late))[0]
                if len(sel) == 0:
                    continue
                if late:
                    search_at = fixed_depth(boards[sel], turn[sel], tables[p], order, 0)
                    plies = np.maximum(caps[p], emp[sel])
                    for d in np.unique(plies):
                        out[sel[plies == d]] = search_at(int(d))[1][plies == d]
                else:
                    search_at = fixed_depth(boards[sel], turn[sel], tables[p], order, max(budgets))
                    r = budget_ref.deepen(search_at, boards[sel], budgets[p], caps[p])
                    assert (r["status"] == budget_ref.SEARCHED).all()
                    out[sel] = r["best_move"]
        return out
    return choose


def game_fields(r):
    return dict(a_black=r.a_black.cpu().numpy(), final_boards=ops.to_numpy_u64(r.final_boards),
                diff=r.diff.cpu().numpy(), plies=r.plies.cpu().numpy(), status=r.status.cpu().numpy(),
                moves=r.moves.cpu().numpy(), hist=r.hist.cpu().numpy())


@pytest.mark.parametrize("order,exact", [(0, 0), (0, 6), (1, 0), (1, 6)])
def test_budget_games_are_the_game_loops_move_for_move(order, exact):
    wa, wb = tree_cases.TABLES["default"], tree_cases.TABLES["rng7"]
    mb, mt = midgame()
    for what, kw, ref in (
            ("opening", dict(n_rand_a=3, n_rand_b=3), dict(n_rand_a=3, n_rand_b=3)),
            ("midgame", dict(start=ops.from_numpy_u64(mb[:8].copy(), "cuda"), start_turn=torch.from_numpy(mt[:8].copy()).cuda()),
             dict(start=mb[:8], start_turn=mt[:8]))):
        r = ops.play(8, 77, weights_a=wa, weights_b=wb, depth_a=CAPS[0], depth_b=CAPS[1], exact_empties=exact,
                     swap_colours=True, record_moves=True, want_nodes=True, order=order, budget=BUDGETS, **kw)
        got = game_fields(r)
        want = play_ref.play(8, 77, budget_chooser((wa, wb), CAPS, BUDGETS, exact, order), swap=True, **ref)
        for k in ("a_black", "final_boards", "diff", "plies", "status", "moves", "hist"):
            assert (got[k] == np.asarray(want[k])).all(), (what, k)
        assert (r.nodes.cpu().numpy() > 0).all() and ops.work_word("cuda").item() == 0


def test_no_budget_is_todays_call_and_a_budget_beyond_every_search_is_the_fixed_depth_game():
    mb, mt = midgame()
    start, turn = ops.from_numpy_u64(mb[:32].copy(), "cuda"), torch.from_numpy(mt[:32].copy()).cuda()
    kw = dict(weights_b=tree_cases.TABLES["rng7"], depth_a=3, depth_b=4, exact_empties=5, n_rand_a=1, n_rand_b=2,
              swap_colours=True, start=start, start_turn=turn, record_moves=True, want_nodes=True)
    for order in (0, 1):
        today = ops.play(32, 9, order=order, **kw)
        none = ops.play(32, 9, order=order, budget=None, **kw)
        for x, y in zip(today, none):
            assert torch.equal(x, y)
        big = ops.play(32, 9, order=order, budget=(2**32 - 1, 2**31), **kw)
        for k in ("final_boards", "diff", "plies", "moves", "hist", "a_black", "status"):
            assert torch.equal(getattr(big, k), getattr(today, k)), (order, k)
        assert (big.nodes >= today.nodes).all()  # the shallower iterations are paid for as well


def test_do_matches_passes_the_budget_through():
    conf = {"proc_n_rand_hands_for_a": 2, "proc_n_rand_hands_for_b": 2, "proc_randomize_black_white": 1}
    wb = tree_cases.TABLES["rng7"]
    m = runner.do_matches(conf, None, n=16, seed=21, weights_b=wb, policy="search", depth=(5, 6), budget=(300, 1500),
                          name_a="Hamlet", name_b="GPU")
    r = ops.play(16, 21, 0, None, wb, 5, 6, 0, 2, 2, True, record_moves=True, budget=(300, 1500))
    assert (m.a_black == r.a_black.cpu().numpy().astype(bool)).all()
    for k in ("final_boards", "diff", "plies", "moves", "hist", "a_black", "status"):
        assert torch.equal(getattr(m.games, k), getattr(r, k)), k
    assert m.books.lines(3) == type(m.books).from_rollout(r).lines(3)
    fixed = ops.play(16, 21, 0, None, wb, 5, 6, 0, 2, 2, True, record_moves=True)
    assert not torch.equal(r.moves, fixed.moves)  # the budget is felt
    assert all(" depth=5 nodes=300 weights=" in x["hamletparam"] for x in m.meta)
    plain = runner.do_matches(conf, None, n=4, seed=21, weights_b=wb, policy="search", depth=2)
    assert all("nodes=" not in x["hamletparam"] for x in plain.meta)


def test_an_engine_process_with_nodes_plays_search_budgets_move():
    """python -m subproc_amd.engine --policy search --nodes 2048 --depth 6: three `go`s, between them a move of
    the other side drawn here; each answer is ops.search_budget's move for the position, and "verbose 1" shows
    the depth that search reached."""
    p = subprocess.Popen([sys.executable, "-m", "subproc_amd.engine", "--policy", "search", "--nodes", "2048",
                          "--depth", "6"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=ROOT)

    def ask(cmd, lines):
        p.stdin.write(cmd + "\n")
        p.stdin.flush()
        return [p.stdout.readline().rstrip("\n") for _ in range(lines)]

    try:
        assert ask("init", 1) == ["init done"]
        b, t = np.array([play_ref.OPENING], np.uint64), np.array([1], np.uint8)
        for k in range(3):
            want = host(ops.search_budget(*dev(b, t), 2048, max_depth=6))
            mv = codec.parse_engine_go("".join(ask("go", 3)))[1]
            assert mv == int(want["best_move"][0]) < 64, (k, mv, want)
            shown = ask("verbose 1", 13)
            assert shown[11].endswith("depth=%d" % int(want["depth"][0])) and want["depth"][0] >= 3, shown
            assert ask("verbose 0", 1) == [""]
            st = oracle.step(b, t, np.array([mv], np.uint8))
            b, t = st["boards"], st["turn"]
            own = int(oracle.legal(b, t)[0])
            reply = [q for q in range(64) if own >> q & 1][k % 2]
            ask(codec.move_str(reply), 3)
            st = oracle.step(b, t, np.array([reply], np.uint8))
            b, t = st["boards"], st["turn"]
        assert ask("quit", 1) == ["bye"]
        assert p.wait(timeout=30) == 0
    finally:
        if p.poll() is None:
            p.kill()
