"""The depth-limited search through the Edax-protocol engine
(Engine(policy="search", depth=D), --policy search --depth D) and the package."""
import io
import sys

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

import subproc_amd  # noqa: E402
from subproc_amd import _lib, codec, engine, ops  # noqa: E402


def go(eng):
    out = []
    eng.handle("go", out.append)
    return codec.parse_engine_go("".join(out))[1]


def state(eng):
    bl, wh = eng.board.bitboards()
    return np.array([[bl, wh]], np.uint64), np.array([eng.board.turn], np.uint8)


def engine_at(black, white, turn, **kw):
    """An engine whose board is the given position (through Board.deserialize, the reference's own way in)."""
    eng = engine.Engine(**kw)
    text = oracle.serialize_str(black, white, turn)
    eng.board.deserialize(text[:64], text[65], 0)
    assert eng.board.bitboards() == (int(black), int(white)) and eng.board.turn == int(turn)
    return eng


def test_package_exports_search():
    assert subproc_amd.search is ops.search and subproc_amd.SearchResult is ops.SearchResult
    assert "search" in subproc_amd.__all__ and "search" in ops.__all__


@pytest.mark.parametrize("engine_side", [1, 2])
def test_depth_1_plays_the_eval_policys_game(engine_side):
    """One full game against a seeded random opponent (its moves drawn here
    from the oracle's legal mask): the search engine at depth 1 and the eval
    engine answer every `go` alike, passes included."""
    rng = np.random.default_rng(0)
    s = engine.Engine(name="S", policy="search", depth=1)
    e = engine.Engine(name="E", policy="eval")
    sink = []
    for eng in (s, e):
        eng.handle("init", sink.append)
    asked = 0
    for _ in range(130):
        if s.board.is_game_over():
            break
        assert s.board.bitboards() == e.board.bitboards() and s.board.turn == e.board.turn
        if s.board.turn == engine_side:
            a, b = go(s), go(e)
            assert a == b, (asked, a, b)
            asked += 1
        else:
            b, t = state(s)
            own = int(oracle.legal(b, t)[0])
            sqs = [q for q in range(64) if own >> q & 1]
            code = sqs[int(rng.integers(len(sqs)))] if sqs else 64
            for eng in (s, e):
                eng.handle(codec.move_str(code), sink.append)
    assert s.board.is_game_over() and e.board.is_game_over() and asked >= 25


def test_depth_3_plays_ops_searchs_move():
    g = oracle.sample_midgame(16, 0x5EED)
    r = ops.search(ops.from_numpy_u64(g["boards"], "cuda"), torch.from_numpy(g["turn"]).cuda(), 3, node_limit=1 << 22)
    assert (r.status.cpu().numpy() == _lib.SEARCH_SEARCHED).all()
    best = r.best_move.cpu().numpy()
    assert (best < 64).all()
    for i in range(16):
        eng = engine_at(g["boards"][i, 0], g["boards"][i, 1], g["turn"][i], policy="search", depth=3)
        assert go(eng) == int(best[i]), i


def test_solve_empties_still_wins_below_its_threshold():
    import solve_cases

    b, t = solve_cases.ladder(6, 8)
    r = ops.solve(ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda(), max_empties=6)
    want = r.best_move.cpu().numpy()
    s3 = ops.search(ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda(), 1).best_move.cpu().numpy()
    assert (want != s3).any()  # the two differ somewhere, so the precedence shows
    for i in range(8):
        eng = engine_at(b[i, 0], b[i, 1], t[i], policy="search", depth=1, solve_empties=6)
        assert go(eng) == int(want[i]), i
        # above the threshold: the search's move
        eng = engine_at(b[i, 0], b[i, 1], t[i], policy="search", depth=1, solve_empties=5)
        assert go(eng) == int(s3[i]), i


def test_engine_names_the_depth(monkeypatch, capsys):
    out = []
    engine.Engine(name="E", policy="search", depth=4).handle("verbose p", out.append)
    assert len(out) == 1 and out[0].startswith("E policy=search depth=4 weights=[")
    out = []
    engine.Engine(name="E", policy="search", depth=2, solve_empties=8).handle("verbose p", out.append)
    assert out[0].startswith("E policy=search depth=2 weights=[") and out[0].endswith(" solve_empties=8")
    out = []
    engine.Engine(name="E", policy="eval").handle("verbose p", out.append)
    assert "depth" not in out[0]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            engine.Engine(policy="search", depth=bad)
    monkeypatch.setattr(sys, "stdin", io.StringIO("verbose p\nquit\n"))
    assert engine.main(["--name", "CLI", "--policy", "search", "--depth", "5"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("CLI policy=search depth=5 weights=[") and lines[1] == "bye"
