"""The Monte Carlo tree search on the host (tools/diag/mcts_host.cpp:
mcts_core.hpp's walk in plain C++ with a plain random playout) against
tests/mcts_ref.py's checker over the oracle, field for field on every set of
tests/mcts_cases.py; and the same under -fsanitize=address,undefined, as a
process of its own.  DESIGN.md §28.  CPU only."""
import struct

import numpy as np
import pytest

import host_programs as hp
import mcts_cases
import mcts_ref

@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "mcts_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "mcts_host", hp.SANITIZED)


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def run(exe, tmp, boards, turn, T, c, M, seed=mcts_cases.SEED, game_id0=mcts_cases.GAME_ID0, table=None):
    inp, out = str(tmp / "min"), str(tmp / "mout")
    table = mcts_ref.log_table(T) if table is None else table
    hp.write_positions(inp, boards, turn)
    with open(inp, "a") as f:
        for x in table:
            f.write("L %x\n" % bits(x))
    hp.run([exe, inp, out, T, "%x" % bits(c), seed, game_id0, M, 8])
    a, last = hp.read_rows(out, (len(turn), 5 + 192), trailer=True)
    return dict(status=a[:, 0], best_move=a[:, 1], nodes=a[:, 2], root_wins=a[:, 3], root_diffs=a[:, 4],
                visits=a[:, 5:69], wins=a[:, 69:133], diffs=a[:, 133:197], plies=int(last[1]))


@pytest.mark.parametrize("name", ["small", "explore", "long"])
def test_the_host_build_equals_the_checker_on_every_field(binary, tmp_path, name):
    b, t = mcts_cases.inputs(name)
    for T, c, M in mcts_cases.runs(name):
        want = mcts_cases.reference(name, T, c, M)
        mcts_cases.same(run(binary, tmp_path, b, t, T, c, M), want, (name, T, c, M))


def test_the_sets_hold_what_they_are_there_for():
    """The branches the sets exist for occur in the checker's own answers."""
    b, t = mcts_cases.inputs("small")
    (T, c, M), = mcts_cases.runs("small")
    want = mcts_cases.reference("small", T, c, M)
    assert want["status"][-1] == mcts_ref.INVALID and want["best_move"][-1] == mcts_ref.NO_MOVE
    assert not any(want[k][-1].any() for k in ("visits", "wins", "diffs", "root_wins", "root_diffs", "nodes"))
    ok = want["status"] == mcts_ref.SEARCHED
    assert ok[:-1].all()
    assert (want["best_move"][ok] == mcts_ref.PASS).any() and (want["best_move"][ok] == mcts_ref.NO_MOVE).any()
    kids = (want["visits"] > 0).sum(1)
    assert kids.max() >= 32  # the wide roots: more children than half a wave
    has_move = want["best_move"] < 64
    assert (want["visits"].sum(1)[has_move] == T).all() and (want["visits"].sum(1)[~has_move] == 0).all()
    assert (want["root_wins"][has_move] == want["wins"].sum(1)[has_move]).all()
    assert (want["nodes"][ok] <= M).all() and (want["nodes"][ok] >= 1).all()
    # the two exploration constants walk different trees; the small tree runs out of room
    (T, c0, M0), (_, c1, _) = mcts_cases.runs("explore")
    r0, r1 = mcts_cases.reference("explore", T, c0, M0), mcts_cases.reference("explore", T, c1, M0)
    assert (r0["visits"] != r1["visits"]).any() and (r0["visits"].max(1) > r1["visits"].max(1)).all()
    (T, c, big), (_, _, tiny) = mcts_cases.runs("long")
    full, cut = mcts_cases.reference("long", T, c, big), mcts_cases.reference("long", T, c, tiny)
    assert (cut["nodes"] <= tiny).all() and (full["nodes"] > tiny).all() and (cut["visits"].sum(1) == T).all()


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    for name in ("small", "explore", "long"):
        b, t = mcts_cases.inputs(name)
        for T, c, M in mcts_cases.runs(name):
            want = mcts_cases.reference(name, T, c, M)
            mcts_cases.same(run(binary_asan, tmp_path, b, t, T, c, M), want, ("asan", name, T, c, M))


def test_the_row_alone_with_its_own_id_is_the_batchs_row(binary, tmp_path):
    b, t = mcts_cases.inputs("explore")
    T, c, M = mcts_cases.runs("explore")[1]
    want = mcts_cases.reference("explore", T, c, M)
    for i in (1, 4):
        got = run(binary, tmp_path, b[i:i + 1], t[i:i + 1], T, c, M, game_id0=mcts_cases.GAME_ID0 + i * T * 64)
        for k in mcts_cases.FIELDS:
            assert (got[k][0] == want[k][i]).all(), (i, k)
