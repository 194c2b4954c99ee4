"""ops.mcts(..., leaves=L) / othv_mcts_wide on the GPU
(include/othello_mcts_wide.h) against tests/mcts_wide_ref.py's
checker over the oracle, field for field, whatever the grid and the launch
plumbing; with one leaf a round, ops.mcts's own bytes; the rule's symmetries
and invariants; and the answer that is not the project's own playouts: with one
empty square every playout is forced.  All comparisons are exact."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import codeobj
import mcts_cases
import mcts_wide_cases as cases
import oracle
import solve_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402
from subproc_amd.codec import handstr_from_coord  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

SEED, ID0 = cases.SEED, cases.GAME_ID0


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def unpack(r):
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy().astype(np.int64) for k, v in r._asdict().items()}


def gpu(boards, turn, R, L, c, M, game_id0=ID0, **kw):
    return unpack(ops.mcts(*dev(boards, turn), R, explore=c, seed=SEED, game_id0=game_id0, max_nodes=M,
                           want_nodes=True, leaves=L, **kw))


@pytest.mark.parametrize("name", cases.SETS)
def test_every_set_equals_the_checker_on_every_field(name):
    for rows, R, L, c, M in cases.runs(name):
        b, t = cases.inputs(name, rows)
        cases.same(gpu(b, t, R, L, c, M), cases.reference(name, rows, R, L, c, M), (name, R, L, c, M))


def test_one_leaf_a_round_gives_ops_mcts_bytes():
    b, t = mcts_cases.inputs("small")
    (T, c, M), = mcts_cases.runs("small")
    bt, tt = dev(b, t)
    one = ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M, want_nodes=True)
    wide = ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M, want_nodes=True, leaves=1)
    torch.cuda.synchronize()
    for k, x, y in zip(one._fields, one, wide):
        assert x.dtype == y.dtype and torch.equal(x, y), k
    # the defaults are the one-wave search's for T = R L
    dflt = ops.mcts(bt, tt, T, explore=c, seed=SEED, game_id0=ID0, leaves=1)
    torch.cuda.synchronize()
    assert dflt.nodes is None and torch.equal(dflt.visits, one.visits) and torch.equal(dflt.wins, one.wins)


def test_three_blocks_walk_the_batch(monkeypatch):
    rows, R, L, c, M = cases.runs("small")[0]
    b, t = cases.inputs("small", rows)
    monkeypatch.setenv("OTH_MCTS_WIDE_BLOCKS", "3")
    assert _lib.load().othv_mcts_wide_grid(len(t), L) == 3  # each block walks 15 trees
    cases.same(gpu(b, t, R, L, c, M), cases.reference("small", rows, R, L, c, M), "three blocks")
    monkeypatch.delenv("OTH_MCTS_WIDE_BLOCKS")
    assert _lib.load().othv_mcts_wide_grid(len(t), L) == len(t)


def test_a_row_alone_with_its_own_id_is_the_batchs_row():
    rows, R, L, c, M = cases.runs("small")[0]
    b, t = cases.inputs("small", rows)
    want = cases.reference("small", rows, R, L, c, M)
    bt, tt = dev(b, t)
    for i in (0, 5, 13, 20, 33, len(t) - 2):
        got = unpack(ops.mcts(bt[i:i + 1], tt[i:i + 1], R, explore=c, seed=SEED, game_id0=ID0 + i * R * L * 64,
                              max_nodes=M, want_nodes=True, leaves=L))
        for k in cases.FIELDS:
            assert (got[k][0] == want[k][i]).all(), (i, k)


def test_two_calls_give_the_same_bytes():
    rows, R, L, c, M = cases.runs("long")[0]
    bt, tt = dev(*cases.inputs("long", rows))
    r1 = ops.mcts(bt, tt, R, seed=SEED, game_id0=ID0, want_nodes=True, leaves=L)
    r2 = ops.mcts(bt, tt, R, seed=SEED, game_id0=ID0, want_nodes=True, leaves=L)
    torch.cuda.synchronize()
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    cases.same(unpack(r1), cases.reference("long", rows, R, L, c, M), "the defaults")
    e = ops.mcts(bt[:0], tt[:0], R, want_nodes=True, leaves=L)
    assert e.visits.shape == (0, 64) and e.best_move.numel() == 0 and e.nodes.numel() == 0


def test_a_captured_graph_replays_to_the_eager_calls_bytes():
    rows, R, L, c, M = cases.runs("explore")[1]
    want = cases.reference("explore", rows, R, L, c, M)
    bt, tt = dev(*cases.inputs("explore", rows))
    table = torch.from_numpy(ops.mcts_log_table(R * L)).cuda()
    kw = dict(explore=c, seed=SEED, game_id0=ID0, max_nodes=M, log_table=table, want_nodes=True, leaves=L)
    eager = ops.mcts(bt, tt, R, **kw)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        r = ops.mcts(bt, tt, R, **kw)
    for _ in range(2):
        for x in r:
            x.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(r, eager):
            assert torch.equal(x, y)
    cases.same(unpack(r), want, "replay")


def test_swapping_the_colours_and_the_mover_changes_nothing():
    rows, R, L, c, M = cases.runs("small")[0]
    b, t = cases.inputs("small", rows)
    got = gpu(b[:, ::-1], 3 - t.astype(np.int64), R, L, c, M)
    cases.same(got, cases.reference("small", rows, R, L, c, M), "colour swap")


def test_the_invariants_on_256_midgame_roots():
    R, L = 8, 8
    M = 1 + 16 * R * L
    g = oracle.sample_midgame(256, 0x5EED)
    r = gpu(g["boards"], g["turn"], R, L, 0.5, M)
    has_move = oracle.legal(g["boards"], g["turn"]) != 0
    assert has_move.sum() > 200
    assert (r["status"] == _lib.MCTS_SEARCHED).all()
    assert (r["visits"].sum(1)[has_move] == R * L).all()
    assert (r["root_wins"][has_move] == r["wins"].sum(1)[has_move]).all()
    assert (r["root_diffs"][has_move] == r["diffs"].sum(1)[has_move]).all()
    assert (r["wins"] <= 128 * r["visits"]).all() and (r["wins"] >= 0).all()
    assert (abs(r["diffs"]) <= 64 * 64 * r["visits"]).all()
    assert (r["nodes"] <= M).all() and (r["nodes"] >= 1).all()
    legal = (oracle.legal(g["boards"], g["turn"])[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    assert not r["visits"][legal == 0].any()
    best = r["best_move"][has_move]
    assert (best < 64).all() and (r["visits"][has_move, best] == r["visits"][has_move].max(1)).all()


def test_with_one_empty_square_the_half_points_are_the_solvers_signs():
    """An answer that is not the project's own playouts: every playout from a
    child of a one-empty root is forced, so wins = 128 * visits * [0, 1/2, 1]
    by the sign of the exact solver's value for that move."""
    cs = solve_cases.cases()[1]
    b, t = cs["boards"], cs["turn"]
    R, L = 4, 4
    r = gpu(b, t, R, L, 0.5, 1 + 16 * R * L)
    sv = ops.solve_moves(*dev(b, t), max_empties=1)
    torch.cuda.synchronize()
    value = sv.move_value.cpu().numpy().astype(np.int64)
    moves = value != _lib.MOVES_NOT_A_MOVE
    assert moves.any() and (value[moves] != _lib.MOVES_UNKNOWN).all()
    assert ((r["visits"] > 0) == moves).all()
    half = np.where(value > 0, 128, np.where(value == 0, 64, 0))
    assert (r["wins"][moves] == (half * r["visits"])[moves]).all()
    assert (r["diffs"][moves] == (64 * value * r["visits"])[moves]).all()


def test_bad_arguments_are_refused():
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    rows, R, L, c, M = cases.runs("explore")[1]
    b, t = cases.inputs("explore", rows)
    n = len(t)
    bt, tt = dev(b, t)
    table = torch.from_numpy(ops.mcts_log_table(65536)).cuda()
    size = lib.othv_mcts_wide_scratch_bytes(n, M, L)
    assert size == lib.othu_mcts_scratch_bytes(n, M)
    scratch = torch.empty(size // 8, dtype=torch.int64, device="cuda")
    good = [bt.data_ptr(), None, R, L, c, table.data_ptr(), SEED, ID0, M, None, None, None, None, None, None, None,
            None, scratch.data_ptr(), size, n, stream]
    assert lib.othv_mcts_wide(*good) == 0  # every output NULL, turn NULL
    torch.cuda.synchronize()
    E = _lib.OTH_EINVAL
    for k, v in ((3, 0), (3, 17), (3, -1), (2, 0), (5, None), (8, 0), (17, None), (18, size - 1), (19, -1)):
        a = list(good)
        a[k] = v
        assert lib.othv_mcts_wide(*a) == E, (k, v)
    a = list(good)
    a[2], a[3] = 65537, 1
    assert lib.othv_mcts_wide(*a) == E
    a[2], a[3] = 4097, 16  # R L = 65,552
    assert lib.othv_mcts_wide(*a) == E
    assert lib.othv_mcts_wide_scratch_bytes(n, M, 0) == E and lib.othv_mcts_wide_scratch_bytes(n, M, 17) == E
    assert lib.othv_mcts_wide_grid(n, 0) == E and lib.othv_mcts_wide_grid(n, 17) == E
    assert lib.othv_mcts_wide_grid(0, 4) == 0 and lib.othv_mcts_wide_grid(-1, 4) == E
    assert lib.othv_mcts_wide_scratch_bytes(100000, 7, 16) == _lib.MCTS_WIDE_MAX_BLOCKS * 7 * 32
    for kw in (dict(leaves=0), dict(leaves=17)):
        with pytest.raises(ValueError, match="leaves must lie"):
            ops.mcts(bt, tt, R, **kw)
    with pytest.raises(ValueError, match="iterations must lie"):
        ops.mcts(bt, tt, 65537, leaves=1)  # R L = 65,537
    with pytest.raises(ValueError, match="iterations must lie"):
        ops.mcts(bt, tt, 4097, leaves=16)
    with pytest.raises(ValueError, match="shape"):
        ops.mcts(bt, tt, R, leaves=L, log_table=table[:R + 1].contiguous())  # the table has R L + 1 entries


def test_vecenv_mcts_takes_leaves():
    env = VecEnv(4)
    r = env.mcts(4, seed=3, want_nodes=True, leaves=4)
    torch.cuda.synchronize()
    assert (r.visits.sum(dim=1) == 16).all() and (r.status == _lib.MCTS_SEARCHED).all()
    assert (r.visits[:, [19, 26, 37, 44]] >= 1).all() and (r.nodes >= 5).all()


def test_the_engines_leaves_plays_ops_mcts_move_with_an_id_of_its_own_per_go_and_refuses_reuse():
    R, L, seed = 6, 4, 11
    cmd = [sys.executable, "-m", "subproc_amd.engine", "--policy", "mcts", "--iterations", str(R), "--leaves", str(L),
           "--seed", str(seed)]
    p = subprocess.run(cmd, input="go\ngo\nquit\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    played = [ln.split()[-1] for ln in p.stdout.splitlines() if " plays " in ln]
    assert len(played) == 2
    env = VecEnv(1)
    want = []
    for k in range(2):
        r = ops.mcts(env.boards, env.turn, R, seed=seed, game_id0=k * R * L * 64, leaves=L)
        sq = int(r.best_move.cpu()[0])
        want.append(("B" if k == 0 else "W") + handstr_from_coord(sq & 7, sq >> 3).upper())
        env.step(r.best_move)
    assert played == want
    other = ops.mcts(env.boards, env.turn, R, seed=seed, game_id0=0, leaves=L)
    mine = ops.mcts(env.boards, env.turn, R, seed=seed, game_id0=2 * R * L * 64, leaves=L)
    assert not torch.equal(other.wins, mine.wins)
    p = subprocess.run(cmd + ["--reuse", "1"], input="quit\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--leaves" in p.stderr


def test_the_kernel_uses_no_scratch_and_the_lds_the_header_states():
    found = codeobj.named(("mcts_wide_rounds",))
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == _lib.MCTS_WIDE_LDS_BYTES == 14912, name
        assert k["vgpr_count"] <= 128, name  # sixteen waves a block: four a SIMD
    src = open(_lib.MCTS_WIDE_HEADER).read()
    assert "#define OTHV_LDS_BYTES %d " % _lib.MCTS_WIDE_LDS_BYTES in src
    assert "#define OTHV_MAX_LEAVES %d " % _lib.MCTS_WIDE_MAX_LEAVES in src
    assert "#define OTHV_MAX_BLOCKS %d " % _lib.MCTS_WIDE_MAX_BLOCKS in src
