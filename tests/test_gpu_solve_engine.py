"""The solver through the public interface: VecEnv.solve, the package-level
export, and the Edax-protocol engine's perfect endgame (Engine(solve_empties=K),
--solve-empties K)."""
import io
import sys

import numpy as np
import pytest
import torch

import oracle
import solve_cases

pytestmark = pytest.mark.gpu

import subproc_amd  # noqa: E402
from subproc_amd import _lib, codec, engine, ops  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

GAME_SEED = 0x501E


def recorded_game(g=0):
    """Move codes of one seeded random game (the oracle's record)."""
    r = oracle.rollout(g + 1, GAME_SEED, record_moves=True)
    return r["moves"][g, :int(r["plies"][g])].tolist()


def feed(eng, moves, empties):
    """Play the recorded moves into the engine until `empties` squares are empty."""
    sink = []
    eng.handle("init", sink.append)
    for code in moves:
        bl, wh = eng.board.bitboards()
        if 64 - bin(bl | wh).count("1") <= empties:
            break
        eng.handle(codec.move_str(code), sink.append)
    bl, wh = eng.board.bitboards()
    assert 64 - bin(bl | wh).count("1") == empties
    return bl, wh, eng.board.turn


def go(eng):
    out = []
    eng.handle("go", out.append)
    return codec.parse_engine_go("".join(out))[1]


def solve_one(bl, wh, turn, **kw):
    b = ops.from_numpy_u64(np.array([[bl, wh]], np.uint64), "cuda")
    r = ops.solve(b, torch.tensor([turn], dtype=torch.uint8, device="cuda"), **kw)
    return int(r.value.cpu()[0]), int(r.best_move.cpu()[0]), int(r.status.cpu()[0])


def test_package_exports_solve():
    assert subproc_amd.solve is ops.solve and subproc_amd.SolveResult is ops.SolveResult
    assert "solve" in subproc_amd.__all__ and "solve" in ops.__all__


def test_vecenv_solve_equals_ops_solve():
    c = solve_cases.cases()
    b = np.concatenate([c[e]["boards"][:40] for e in (3, 5, 7, 9)])
    t = np.concatenate([c[e]["turn"][:40] for e in (3, 5, 7, 9)])
    want_v = np.concatenate([c[e]["value"][:40] for e in (3, 5, 7, 9)])
    env = VecEnv(len(t))
    env.boards, env.turn = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    r = env.solve(max_empties=7, node_limit=1 << 18)
    o = ops.solve(env.boards, env.turn, max_empties=7, node_limit=1 << 18)
    for x, y in zip(r[:3], o[:3]):
        assert torch.equal(x, y)
    s = r.status.cpu().numpy()
    assert (s[:120] == _lib.SOLVE_SOLVED).all() and (s[120:] == _lib.SOLVE_SKIPPED).all()
    assert (r.value.cpu().numpy()[:120] == want_v[:120]).all()
    full = env.solve()
    assert (full.value.cpu().numpy() == want_v).all()


def test_engine_plays_the_solvers_move():
    moves = recorded_game()
    eng = engine.Engine(policy="greedy", solve_empties=8)
    bl, wh, turn = feed(eng, moves, 8)
    value, best, status = solve_one(bl, wh, turn, max_empties=8)
    assert status == _lib.SOLVE_SOLVED
    puts = eng.board.puttables(eng.board.turn)
    assert puts and best < 64
    assert go(eng) == best


@pytest.mark.parametrize("empties,k", [(9, 8), (8, 0), (20, 8)])
def test_engine_is_unchanged_outside_the_solved_range(empties, k):
    moves = recorded_game()
    for policy in ("greedy", "eval", "random"):
        a = engine.Engine(policy=policy, seed=3, solve_empties=k)
        b = engine.Engine(policy=policy, seed=3)
        feed(a, moves, empties)
        feed(b, moves, empties)
        assert go(a) == go(b), policy


def test_two_solving_engines_reach_the_solved_value():
    moves = recorded_game(1)
    a = engine.Engine(name="A", policy="random", seed=1, solve_empties=8)
    b = engine.Engine(name="B", policy="random", seed=2, solve_empties=8)
    bl, wh, turn = feed(a, moves, 8)
    feed(b, moves, 8)
    value, _, status = solve_one(bl, wh, turn, max_empties=8)
    assert status == _lib.SOLVE_SOLVED
    sink = []
    atk, dfn = a, b
    for _ in range(40):
        if atk.board.is_game_over():
            break
        code = go(atk)
        dfn.handle(codec.move_str(code), sink.append)
        atk, dfn = dfn, atk
    assert a.board.is_game_over() and a.board.bitboards() == b.board.bitboards()
    diff = a.board.n_black() - a.board.n_white()
    assert (diff if turn == 1 else -diff) == value


def test_engine_names_the_setting(monkeypatch, capsys):
    out = []
    engine.Engine(name="E", policy="greedy", solve_empties=8).handle("verbose p", out.append)
    assert out == ["E policy=greedy solve_empties=8"]
    out = []
    engine.Engine(name="E", policy="greedy").handle("verbose p", out.append)
    assert out == ["E policy=greedy"]
    with pytest.raises(ValueError):
        engine.Engine(solve_empties=13)
    monkeypatch.setattr(sys, "stdin", io.StringIO("verbose p\nquit\n"))
    assert engine.main(["--name", "CLI", "--policy", "random", "--solve-empties", "6"]) == 0
    assert capsys.readouterr().out.splitlines() == ["CLI policy=random solve_empties=6", "bye"]
