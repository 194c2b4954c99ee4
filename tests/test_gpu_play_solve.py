"""ops.play(solve_empties=E) / othx_play on the GPU (include/othello_play_solve.h,
DESIGN.md §25): search self-play whose last E empties are the exact solver's.

Up to E = 8 the games are those of the existing exact_empties path, field for
field; at E = 9 they are the exhaustive checker's (tests/play_ref.py with
search_ref above the zone and solve_ref inside it); at 10 and 11 the checker's
with ops.solve (one lane, untouched by this, checked in test_gpu_solve.py) as
the zone's chooser; at 12 the recorded games satisfy the solver's invariant.
Then the node limit, the edges, graph capture and the layers above.  Every game
of every case is compared, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import play_cases
import play_ref
import play_solve_cases as cases
import search_ref
import solve_cases
import synthetic_cases as sc

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops, runner  # noqa: E402
from subproc_amd.books import GameBooks  # noqa: E402

SEARCHED, INVALID, LIMIT = _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT
NODE_LIMIT = 1 << 24  # per search and per solve; the hardest 12-empties solve of these cases stays far below
DEFAULT, WB = play_cases.DEFAULT, search_ref.WEIGHTS_B
FULL = (1 << 64) - 1
KEYS = ("a_black", "final_boards", "diff", "plies", "moves", "status", "hist")


def dev_starts(boards, turn):
    b = None if boards is None else ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")
    t = None if turn is None else torch.from_numpy(np.array(turn, np.uint8)).cuda()
    return b, t


def host(r):
    out = {k: getattr(r, k).cpu().numpy() for k in ("a_black", "diff", "plies", "moves", "status", "hist")}
    out["final_boards"] = ops.to_numpy_u64(r.final_boards).reshape(-1, 2)
    out["nodes"] = r.nodes.cpu().numpy().view(np.uint64)
    return out


def gpu_play(n, seed, boards=None, turn=None, node_limit=NODE_LIMIT, **kw):
    """ops.play's result as a dict of numpy arrays; the stream's work word is 0 afterwards."""
    b, t = dev_starts(boards, turn)
    r = ops.play(n, seed, start=b, start_turn=t, record_moves=True, node_limit=node_limit, want_nodes=True, **kw)
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    return host(r)


def assert_same_games(got, ref, keys=KEYS, what=None):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
        assert len(bad) == 0, (what, k, bad[:8], a[bad[:4]], b[bad[:4]])


# ---------------------------------------------------------------- equal to the existing path
KINDS = {"plain": dict(), "ordered": dict(order=1), "budget": dict(budget=(64, 512)),
         "budget_ordered": dict(budget=(64, 512), order=1)}


def twin_args(source, kind):
    """The games' arguments without the zone.  The opening: depth 1, random budgets (2, 3), the swap, 4,096 +
    37 games (many blocks, a ragged last request, a list filled from many blocks).  The midgame starts:
    test_gpu_play.py's arguments.  By budget the depths are caps, 6 plies, so that the budgets decide."""
    if source == "opening":
        a = dict(n=4096 + 37, seed=23, weights_a=DEFAULT, weights_b=WB, depth_a=1, depth_b=1, n_rand_a=2, n_rand_b=3,
                 swap_colours=True)
    else:
        g = play_cases.midgame()
        a = dict(n=4097, seed=7, boards=g["boards"], turn=g["turn"], game_id0=11, weights_a=DEFAULT, weights_b=WB,
                 depth_a=2, depth_b=2, swap_colours=True)
    a.update(KINDS[kind])
    if "budget" in a:
        a.update(depth_a=6, depth_b=6)
    return a


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("source", ["opening", "midgame"])
@pytest.mark.parametrize("e", [1, 4, 8])
def test_up_to_8_empties_the_games_are_the_exact_empties_ones(e, source, kind):
    a = twin_args(source, kind)
    want = gpu_play(exact_empties=e, **a)
    got = gpu_play(solve_empties=e, **a)
    assert (want["status"] == SEARCHED).all()
    assert_same_games(got, want, what=(e, source, kind))
    assert (got["hist"] == play_ref.histogram(got["diff"], got["plies"])).all()
    assert (got["nodes"] > 0).all()
    lib = _lib.load()
    order, budgeted = a.get("order", 0), int("budget" in a)
    assert lib.othx_play_grid(a["n"], order, budgeted) == (lib.othb_play_grid(a["n"]) if budgeted else
                                                           lib.otho_play_ordered_grid(a["n"], order))


@pytest.mark.parametrize("name", sorted(sc.PLAY))
def test_off_tree_boards_at_8_against_the_exact_empties_twin(name):
    c = sc.PLAY[name]
    b, t = sc.play_starts(name)
    a = dict(n=len(t), seed=c["seed"], boards=b, turn=t, weights_a=sc.TABLES["default"], weights_b=sc.TABLES["rng7"],
             depth_a=c["depth"][0], depth_b=c["depth"][1], swap_colours=True)
    assert_same_games(gpu_play(solve_empties=8, **a), gpu_play(exact_empties=8, **a), what=name)


# ---------------------------------------------------------------- above 8: the checkers
def test_9_empties_against_the_exhaustive_checker():
    b, t = solve_cases.ladder(11, 16)
    ref = play_ref.play(16, 31, cases.chooser(DEFAULT, WB, 2, 1, 9), n_rand_a=1, n_rand_b=2, swap=True, start=b,
                        start_turn=t)
    for order in (0, 1):
        got = gpu_play(16, 31, b, t, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1, n_rand_a=1, n_rand_b=2,
                       swap_colours=True, solve_empties=9, order=order)
        assert_same_games(got, ref, what=order)


def merged_solver(max_empties):
    def solver(boards, turn):
        b, t = dev_starts(boards, turn)
        r = ops.solve(b, t, max_empties=max_empties, node_limit=NODE_LIMIT)
        assert bool((r.status == _lib.SOLVE_SOLVED).all())
        return r.best_move.cpu().numpy()
    return solver


@functools.lru_cache(maxsize=None)
def merged_reference(e):
    b, t = solve_cases.ladder(e + 2, 64)
    r = play_ref.play(64, 40 + e, cases.chooser(DEFAULT, WB, 2, 1, e, merged_solver(e)), game_id0=5, n_rand_a=1,
                      n_rand_b=2, swap=True, start=b, start_turn=t)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("e", [10, 11])
def test_10_and_11_empties_against_the_checker_with_the_merged_solver(e, monkeypatch):
    b, t = solve_cases.ladder(e + 2, 64)
    ref = merged_reference(e)
    a = dict(n=64, seed=40 + e, boards=b, turn=t, game_id0=5, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1,
             n_rand_a=1, n_rand_b=2, swap_colours=True, solve_empties=e)
    got = gpu_play(**a)
    assert_same_games(got, ref, what=e)
    assert (got["a_black"] == 0).any() and (got["a_black"] == 1).any()
    if e == 10:  # one block takes the whole list in both phases
        monkeypatch.setenv("OTH_PLAY_BLOCKS", "1")
        assert _lib.load().othx_play_grid(64, 0, 0) == 1
        narrow = gpu_play(**a)
        monkeypatch.delenv("OTH_PLAY_BLOCKS")
        assert_same_games(narrow, got, keys=KEYS + ("nodes",), what="one block")


def test_12_empties_by_the_solvers_invariant():
    """No random moves: from the first recorded position with at most 12 empties both sides play perfectly, so
    the final difference is the solver's value there from its mover's side, and every policy move after it (two
    legal moves or more) is the solver's best move on the replayed position: one batched ops.solve."""
    b, t = solve_cases.ladder(13, 16)
    got = gpu_play(16, 77, b, t, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1, swap_colours=True,
                   solve_empties=12)
    assert (got["status"] == SEARCHED).all()
    db, dt = dev_starts(b, t)
    rp = ops.replay(torch.from_numpy(got["moves"]).cuda(), torch.from_numpy(got["plies"]).cuda(), db, dt)
    pos, turn = ops.to_numpy_u64(rp.boards).reshape(16, -1, 2), rp.turn.cpu().numpy().reshape(16, -1)
    rows, first = [], []
    for g in range(16):
        plies = int(got["plies"][g])
        emp = [64 - bin(int(x[0] | x[1])).count("1") for x in pos[g, :plies + 1]]
        f = next(p for p, e in enumerate(emp) if e <= 12)
        assert f < plies and emp[f] == 12
        first.append(len(rows))
        rows.extend((g, p) for p in range(f, plies))
    gi, pi = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    pb, pt = pos[gi, pi], turn[gi, pi]
    assert pt.min() >= 1 and pt.max() <= 2
    sv = ops.solve(*dev_starts(pb, pt), max_empties=12, node_limit=NODE_LIMIT)
    assert bool((sv.status == _lib.SOLVE_SOLVED).all())
    value, best = sv.value.cpu().numpy().astype(np.int64), sv.best_move.cpu().numpy()
    want = got["diff"].astype(np.int64) * np.where(pt[first] == 1, 1, -1)
    assert (value[first] == want).all()
    own = ops.to_numpy_u64(ops.legal(*dev_starts(pb, pt)))
    policy = (own & (own - np.uint64(1))) != 0
    assert policy.sum() >= 16 * 4
    assert (got["moves"][gi, pi][policy] == best[policy]).all()


# ---------------------------------------------------------------- the node limit
def test_node_limit_1_stops_a_game_at_its_first_solve():
    b, t = solve_cases.ladder(8, 32)
    got = gpu_play(32, 3, b, t, node_limit=1, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1, solve_empties=10)
    own = ops.to_numpy_u64(ops.legal(*dev_starts(b, t)))
    policy = (own & (own - np.uint64(1))) != 0  # no random moves: two legal moves make the first turn a policy turn
    assert policy.sum() >= 16
    assert (got["status"][policy] == LIMIT).all() and (got["plies"][policy] == 0).all()
    assert (got["final_boards"][policy] == b[policy]).all() and (got["moves"][policy] == 255).all()
    assert (got["hist"] == play_ref.histogram(got["diff"][got["status"] == SEARCHED],
                                              got["plies"][got["status"] == SEARCHED])).all()


def test_node_limit_2000_at_10_empties():
    """Depth 1, E = 10, 64 games from 12 empties: every game ends SEARCHED or LIMIT; a LIMIT game's moves are a
    prefix of the unlimited run's game and its final boards that prefix's position, inside the zone; the
    others are the unlimited games and the histogram counts them alone.  The figure 2000 is the one set with
    the feature; on the host build (tools/diag/play_solve_host.cpp, the same arguments) 63 of the 64 games end
    LIMIT there, the hardest whole game needing 250,872 nodes without a limit."""
    b, t = solve_cases.ladder(12, 64)
    a = dict(n=64, seed=9, boards=b, turn=t, weights_a=DEFAULT, weights_b=WB, depth_a=1, depth_b=1, swap_colours=True,
             solve_empties=10)
    full = gpu_play(**a)
    got = gpu_play(node_limit=2000, **a)
    assert (full["status"] == SEARCHED).all() and np.isin(got["status"], (SEARCHED, LIMIT)).all()
    print("LIMIT games at 2000:", int((got["status"] == LIMIT).sum()))
    done = got["status"] == SEARCHED
    for k in KEYS[:-1]:
        assert (got[k][done] == full[k][done]).all(), k
    assert (got["hist"] == play_ref.histogram(full["diff"][done], full["plies"][done])).all()
    db, dt = dev_starts(b, t)
    rp = ops.replay(torch.from_numpy(full["moves"]).cuda(), torch.from_numpy(full["plies"]).cuda(), db, dt)
    pos = ops.to_numpy_u64(rp.boards).reshape(64, -1, 2)
    for g in np.nonzero(~done)[0]:
        p = int(got["plies"][g])
        assert p < full["plies"][g] and got["a_black"][g] == full["a_black"][g]
        assert (got["moves"][g, :p] == full["moves"][g, :p]).all() and (got["moves"][g, p:] == 255).all()
        assert (got["final_boards"][g] == pos[g, p]).all()
        assert 64 - bin(int(pos[g, p, 0] | pos[g, p, 1])).count("1") <= 10
        assert got["diff"][g] == bin(int(pos[g, p, 0])).count("1") - bin(int(pos[g, p, 1])).count("1")


# ---------------------------------------------------------------- edges
def test_empty_batch_failed_calls_overlap_and_a_start_already_over():
    r = ops.play(0, 1, record_moves=True, want_nodes=True, solve_empties=10)
    assert r.final_boards.shape == (0, 2) and r.moves.shape == (0, ops.MOVES_STRIDE) and int(r.hist.sum()) == 0
    for bad in (dict(depth_a=0), dict(depth_a=9), dict(depth_a=2, depth_b=9), dict(n_rand_a=-1), dict(order=2)):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.play(4, 1, solve_empties=10, **bad)
        torch.cuda.synchronize()
        assert ops.work_word("cuda").item() == 0
    # the C call's own checks on the scratch, with games to play: nothing is launched, the word stays 0
    lib, w = _lib.load(), ops.work_word("cuda")
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    wt = ops._weights_ptr(DEFAULT)

    def raw(scratch, size, zone=10, ba=0, bb=0):
        return lib.othx_play(None, None, 1, 0, wt, wt, 2, 2, ba, bb, zone, 0, 0, 0, 0, 0, None, None, None, None, None,
                             None, None, None, scratch, size, w.data_ptr(), 4,
                             torch.cuda.current_stream().cuda_stream)

    E = _lib.OTH_EINVAL
    need = lib.othx_scratch_bytes(4)
    assert raw(None, need) == E and raw(buf.data_ptr() + 8, need) == E and raw(buf.data_ptr(), need - 1) == E
    assert raw(buf.data_ptr(), need, zone=13) == E and raw(buf.data_ptr(), need, ba=3) == E
    assert raw(buf.data_ptr(), need) == 0  # every output NULL
    torch.cuda.synchronize()
    assert w.item() == 0
    # overlapping starts beside played neighbours, and a start already over
    g = play_cases.midgame()
    ob, ot = cases.flagged("over", 8)  # inside the zone: it is parked, and the second phase finds it over
    rows = np.array([[FULL ^ 0xF, 0x10], g["boards"][0], [FULL, FULL], ob, g["boards"][1]], np.uint64)
    turn = np.array([1, g["turn"][0], 2, ot, g["turn"][1]], np.uint8)
    a = dict(game_id0=10, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=2, swap_colours=True)
    r = gpu_play(5, 7, rows, turn, solve_empties=8, **a)
    assert r["status"].tolist() == [INVALID, SEARCHED, INVALID, SEARCHED, SEARCHED]
    assert (r["final_boards"][[0, 2, 3]] == rows[[0, 2, 3]]).all() and r["plies"][[0, 2, 3]].tolist() == [0, 0, 0]
    assert r["diff"][[0, 2]].tolist() == [0, 0] and r["a_black"][[0, 2]].tolist() == [1, 1]
    assert r["nodes"][[0, 2, 3]].tolist() == [0, 0, 0] and (r["moves"][[0, 2, 3]] == 255).all()
    assert_same_games(r, gpu_play(5, 7, rows, turn, exact_empties=8, **a))
    assert r["hist"][129:132].sum() == 3


def test_graph_capture_and_two_replays_give_the_direct_calls_games():
    b, t = solve_cases.ladder(12, 64)
    db, dt = dev_starts(b, t)
    kw = dict(start=db, start_turn=dt, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1, n_rand_a=1, n_rand_b=2,
              swap_colours=True, record_moves=True, want_nodes=True, node_limit=NODE_LIMIT, solve_empties=10)
    direct = host(ops.play(64, 12, **kw))
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    hist = torch.zeros(ops.HIST_BINS, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.play(64, 12, **kw)
        r = ops.play(64, 12, work=w, hist=hist, **kw)
    for _ in range(2):
        for x in (r.final_boards, r.diff, r.plies, r.moves, r.a_black, r.status, r.nodes, hist):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_games(host(r), direct, keys=KEYS + ("nodes",))
        assert w.item() == 0


# ---------------------------------------------------------------- the layers above
def test_do_matches_passes_it_through_and_the_books_take_the_games():
    conf = {"proc_n_rand_hands_for_a": 2, "proc_n_rand_hands_for_b": 3, "proc_randomize_black_white": 1}
    n = 256
    mb = runner.do_matches(conf, DEFAULT, n=n, seed=17, game_id0=300, weights_b=WB, policy="search", depth=(2, 1),
                           solve_empties=10)
    direct = gpu_play(n, 17, game_id0=300, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=1, n_rand_a=2,
                      n_rand_b=3, swap_colours=True, node_limit=0, solve_empties=10)
    r = mb.games
    assert (ops.to_numpy_u64(r.final_boards).reshape(-1, 2) == direct["final_boards"]).all()
    assert (r.moves.cpu().numpy() == direct["moves"]).all() and (r.a_black.cpu().numpy() == direct["a_black"]).all()
    line = "Hamlet policy=search depth=2 weights=%s solve_empties=10" % DEFAULT.reshape(-1).tolist()
    assert all(m["hamletparam"] == line for m in mb.meta)
    books = GameBooks.from_rollout(r)
    for g in (0, 1, n - 1):
        recs = books.records(g)
        assert recs[-1]["end"] and len(recs) == int(direct["plies"][g]) + 1
        assert mb.books.records(g)[-1]["book"] == recs[-1]["book"]
    with pytest.raises(ValueError, match="only one of the two"):
        runner.do_matches(conf, DEFAULT, n=4, policy="search", depth=2, exact_empties=4, solve_empties=10)
