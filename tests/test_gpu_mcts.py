"""ops.mcts / othu_mcts on the GPU (include/othello_mcts.h)
against tests/mcts_ref.py's checker over the oracle, field for field, whatever
the grid and the launch plumbing; the rule's symmetries and invariants; and one
answer that is not the project's own playouts: with one empty square every
playout is forced, so the half-points are the exact solver's signs.  All
comparisons are exact."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcts_cases
import oracle
import solve_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402
from subproc_amd.codec import handstr_from_coord  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

SEED, ID0 = mcts_cases.SEED, mcts_cases.GAME_ID0


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def unpack(r):
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy().astype(np.int64) for k, v in r._asdict().items()}


def gpu(boards, turn, T, c, M, game_id0=ID0, **kw):
    return unpack(ops.mcts(*dev(boards, turn), T, explore=c, seed=SEED, game_id0=game_id0, max_nodes=M,
                           want_nodes=True, **kw))


@pytest.mark.parametrize("name", ["small", "explore", "long"])
def test_every_set_equals_the_checker_on_every_field(name):
    b, t = mcts_cases.inputs(name)
    for T, c, M in mcts_cases.runs(name):
        mcts_cases.same(gpu(b, t, T, c, M), mcts_cases.reference(name, T, c, M), (name, T, c, M))


def test_three_blocks_walk_the_batch_and_a_row_alone_is_the_batchs_row(monkeypatch):
    b, t = mcts_cases.inputs("small")
    (T, c, M), = mcts_cases.runs("small")
    want = mcts_cases.reference("small", T, c, M)
    monkeypatch.setenv("OTH_MCTS_BLOCKS", "3")
    assert _lib.load().othu_mcts_grid(len(t)) == 3  # each wave walks about 14 trees
    mcts_cases.same(gpu(b, t, T, c, M), want, "three blocks")
    monkeypatch.delenv("OTH_MCTS_BLOCKS")
    assert _lib.load().othu_mcts_grid(len(t)) == len(t)
    bt, tt = dev(b, t)
    for i in (0, 5, 13, 20, 33, len(t) - 2):
        got = unpack(ops.mcts(bt[i:i + 1], tt[i:i + 1], T, explore=c, seed=SEED, game_id0=ID0 + i * T * 64,
                              max_nodes=M, want_nodes=True))
        for k in mcts_cases.FIELDS:
            assert (got[k][0] == want[k][i]).all(), (i, k)


def test_two_calls_give_the_same_bytes_and_the_default_arguments_are_the_documented_ones():
    b, t = mcts_cases.inputs("explore")
    bt, tt = dev(b, t)
    r1 = ops.mcts(bt, tt, 40, seed=SEED, game_id0=ID0, want_nodes=True)
    r2 = ops.mcts(bt, tt, 40, seed=SEED, game_id0=ID0, want_nodes=True)
    torch.cuda.synchronize()
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    table = torch.from_numpy(ops.mcts_log_table(40)).cuda()
    r3 = unpack(ops.mcts(bt, tt, 40, explore=0.5, seed=SEED, game_id0=ID0, max_nodes=1 + 16 * 40, log_table=table,
                         want_nodes=True))
    for k, v in unpack(r1).items():
        assert (v == r3[k]).all(), k
    assert ops.mcts(bt, tt, 40).nodes is None
    # another table walks another tree: the library takes the logarithms as given
    r4 = unpack(ops.mcts(bt, tt, 40, seed=SEED, game_id0=ID0, log_table=table * 50, want_nodes=True))
    assert (r4["visits"] != r3["visits"]).any()
    e = ops.mcts(bt[:0], tt[:0], 40, want_nodes=True)
    assert e.visits.shape == (0, 64) and e.best_move.numel() == 0 and e.nodes.numel() == 0


def test_swapping_the_colours_and_the_mover_changes_nothing():
    b, t = mcts_cases.inputs("small")
    T, c, M = mcts_cases.runs("small")[0]
    want = mcts_cases.reference("small", T, c, M)
    got = gpu(b[:, ::-1], 3 - t.astype(np.int64), T, c, M)
    mcts_cases.same(got, want, "colour swap",
                    ("visits", "wins", "diffs", "root_wins", "root_diffs", "best_move", "nodes", "status"))


def test_the_invariants_on_256_midgame_roots():
    T = 32
    M = 1 + 16 * T
    g = oracle.sample_midgame(256, 0x5EED)
    r = gpu(g["boards"], g["turn"], T, 0.5, M)
    has_move = oracle.legal(g["boards"], g["turn"]) != 0
    assert has_move.sum() > 200
    assert (r["status"] == _lib.MCTS_SEARCHED).all()
    assert (r["visits"].sum(1)[has_move] == T).all()
    assert (r["root_wins"][has_move] == r["wins"].sum(1)[has_move]).all()
    assert (r["root_diffs"][has_move] == r["diffs"].sum(1)[has_move]).all()
    assert (r["wins"] <= 128 * r["visits"]).all() and (r["wins"] >= 0).all()
    assert (abs(r["diffs"]) <= 64 * 64 * r["visits"]).all()
    assert (r["nodes"] <= M).all() and (r["nodes"] >= 1).all()
    legal = (oracle.legal(g["boards"], g["turn"])[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    assert not r["visits"][legal == 0].any()
    best = r["best_move"][has_move]
    assert (best < 64).all() and (r["visits"][has_move, best] == r["visits"][has_move].max(1)).all()
    # every root child is visited once before any is visited twice
    kids = legal.sum(1).astype(np.int64)
    few = has_move & (kids <= T)
    assert ((r["visits"] > 0).sum(1)[few] == kids[few]).all()


def test_with_one_empty_square_the_half_points_are_the_solvers_signs():
    """An answer that is not the project's own playouts: every playout from a
    child of a one-empty root is forced, so wins = 128 * visits * [0, 1/2, 1]
    by the sign of the exact solver's value for that move."""
    cs = solve_cases.cases()[1]
    b, t = cs["boards"], cs["turn"]
    T = 16
    r = gpu(b, t, T, 0.5, 1 + 16 * T)
    sv = ops.solve_moves(*dev(b, t), max_empties=1)
    torch.cuda.synchronize()
    value = sv.move_value.cpu().numpy().astype(np.int64)
    moves = value != _lib.MOVES_NOT_A_MOVE
    assert moves.any() and (value[moves] != _lib.MOVES_UNKNOWN).all()
    assert ((r["visits"] > 0) == moves).all()
    half = np.where(value > 0, 128, np.where(value == 0, 64, 0))
    assert (r["wins"][moves] == (half * r["visits"])[moves]).all()
    assert (r["diffs"][moves] == (64 * value * r["visits"])[moves]).all()


def test_a_captured_graph_replays_to_the_eager_calls_bytes():
    b, t = mcts_cases.inputs("explore")
    T, c, M = mcts_cases.runs("explore")[1]
    want = mcts_cases.reference("explore", T, c, M)
    bt, tt = dev(b, t)
    table = torch.from_numpy(ops.mcts_log_table(T)).cuda()
    eager = ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M, log_table=table, want_nodes=True)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        r = ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M, log_table=table, want_nodes=True)
    for _ in range(2):
        for x in r:
            x.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(r, eager):
            assert torch.equal(x, y)
    mcts_cases.same(unpack(r), want, "replay")


def test_null_outputs_null_turn_and_bad_arguments():
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    b, t = mcts_cases.inputs("explore")
    n = len(t)
    T, c, M = mcts_cases.runs("explore")[1]
    bt, tt = dev(b, np.ones(n, np.uint8))
    table = torch.from_numpy(ops.mcts_log_table(T)).cuda()
    size = lib.othu_mcts_scratch_bytes(n, M)
    scratch = torch.empty(size // 8, dtype=torch.int64, device="cuda")
    visits = torch.full((n, 64), 77, dtype=torch.int32, device="cuda")
    good = [bt.data_ptr(), None, T, c, table.data_ptr(), SEED, ID0, M, None, None, None, None, None, None, None, None,
            scratch.data_ptr(), size, n, stream]
    assert lib.othu_mcts(*good) == 0  # every output NULL, turn NULL
    a = list(good)
    a[8] = visits.data_ptr()
    assert lib.othu_mcts(*a) == 0  # turn NULL: Black everywhere
    torch.cuda.synchronize()
    black = unpack(ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M))
    assert (visits.cpu().numpy() == black["visits"]).all()
    for k, v in ((0, None), (2, 0), (2, 65537), (4, None), (7, 0), (7, (1 << 20) + 1), (16, None),
                 (16, scratch.data_ptr() + 8), (17, size - 1), (18, -1)):
        a = list(good)
        a[k] = v
        assert lib.othu_mcts(*a) == _lib.OTH_EINVAL, (k, v)
    with pytest.raises(ValueError, match="iterations must lie"):
        ops.mcts(bt, tt, 0)
    with pytest.raises(ValueError, match="shape"):
        ops.mcts(bt, tt, T, log_table=table[:-1].contiguous())


def test_vecenv_mcts():
    env = VecEnv(4)
    r = env.mcts(16, seed=3, want_nodes=True)
    torch.cuda.synchronize()
    assert (r.visits.sum(dim=1) == 16).all() and (r.status == _lib.MCTS_SEARCHED).all()
    assert set(r.best_move.cpu().tolist()) <= {19, 26, 37, 44}  # d3, c4, f5, e6
    assert (r.visits[:, [19, 26, 37, 44]] >= 1).all() and (r.nodes >= 5).all()
    # the games' ids differ (game i takes its own), so four games from one position are four searches
    assert len({tuple(row) for row in r.wins.cpu().tolist()}) > 1


def test_the_engines_policy_mcts_plays_ops_mcts_best_move_with_an_id_of_its_own_per_go():
    T, seed = 24, 11
    p = subprocess.run([sys.executable, "-m", "subproc_amd.engine", "--policy", "mcts", "--iterations", str(T),
                        "--seed", str(seed)], input="go\ngo\nquit\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    played = [ln.split()[-1] for ln in p.stdout.splitlines() if " plays " in ln]
    assert len(played) == 2
    env = VecEnv(1)
    want = []
    for k in range(2):
        r = ops.mcts(env.boards, env.turn, T, seed=seed, game_id0=k * T * 64)
        sq = int(r.best_move.cpu()[0])
        want.append(("B" if k == 0 else "W") + handstr_from_coord(sq & 7, sq >> 3).upper())
        env.step(r.best_move)
    assert played == want
    # the second go's ids are its own: with the first go's ids it is another search
    other = ops.mcts(env.boards, env.turn, T, seed=seed, game_id0=0, want_nodes=True)
    mine = ops.mcts(env.boards, env.turn, T, seed=seed, game_id0=2 * T * 64, want_nodes=True)
    assert not torch.equal(other.wins, mine.wins)
