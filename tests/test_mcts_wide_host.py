"""The wide Monte Carlo tree search on the host (tools/diag/mcts_wide_host.cpp:
mcts_wide_core.hpp's rounds in plain C++) against tests/mcts_wide_ref.py's
checker over the oracle, field for field on every set of
tests/mcts_wide_cases.py; the same under -fsanitize=address,undefined, as a
process of its own; and with one leaf a round it is the existing checker of
the one-wave search.  DESIGN.md §31.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import host_programs as hp
import mcts_cases
import mcts_ref
import mcts_wide_cases as cases

PROGRAM = "mcts_wide_host"


def compiled(tmp_path_factory, flags):
    """The program under `flags`, with the scores' -ffp-contract=off (a compile line of this module's own)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    name = PROGRAM + hp.SUFFIX[flags]
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe,
                           os.path.join(hp.DIAG, PROGRAM + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return compiled(tmp_path_factory, hp.PLAIN)


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return compiled(tmp_path_factory, hp.SANITIZED)


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def run(exe, tmp, boards, turn, R, L, c, M, seed=cases.SEED, game_id0=cases.GAME_ID0):
    inp, out = str(tmp / "win"), str(tmp / "wout")
    hp.write_positions(inp, boards, turn)
    with open(inp, "a") as f:
        for x in mcts_ref.log_table(R * L):
            f.write("L %x\n" % bits(x))
    hp.run([exe, inp, out, R, L, "%x" % bits(c), seed, game_id0, M, 8])
    a, last = hp.read_rows(out, (len(turn), 5 + 192), trailer=True)
    return dict(status=a[:, 0], best_move=a[:, 1], nodes=a[:, 2], root_wins=a[:, 3], root_diffs=a[:, 4],
                visits=a[:, 5:69], wins=a[:, 69:133], diffs=a[:, 133:197], plies=int(last[1]))


@pytest.mark.parametrize("name", cases.SETS)
def test_the_host_build_equals_the_checker_on_every_field(binary, tmp_path, name):
    for rows, R, L, c, M in cases.runs(name):
        b, t = cases.inputs(name, rows)
        cases.same(run(binary, tmp_path, b, t, R, L, c, M), cases.reference(name, rows, R, L, c, M), (name, R, L, c, M))


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    for name in cases.SETS:
        for rows, R, L, c, M in cases.runs(name):
            b, t = cases.inputs(name, rows)
            cases.same(run(binary_asan, tmp_path, b, t, R, L, c, M), cases.reference(name, rows, R, L, c, M),
                       ("asan", name, R, L, c, M))


def test_with_one_leaf_a_round_it_is_the_one_wave_searchs_checker(binary, tmp_path):
    b, t = mcts_cases.inputs("small")
    (T, c, M), = mcts_cases.runs("small")
    cases.same(run(binary, tmp_path, b, t, T, 1, c, M), mcts_cases.reference("small", T, c, M), "L = 1")


def test_the_sets_hold_what_they_are_there_for():
    """The branches the sets exist for occur in the checker's own answers."""
    (rows, R, L, c, M), = cases.runs("wide")
    want = cases.reference("wide", rows, R, L, c, M)
    kids = (want["visits"] > 0).sum(1)
    # rounds 0 and 1 put their 16 walkers on 16 fresh children of the root, one each: 32 before anybody is scored
    assert (kids[:4] >= 32).all() and (want["visits"][:4].sum(1) == 48).all()
    over = want["best_move"] == mcts_ref.NO_MOVE  # the finished game, the full boards: 16 walkers at a terminal root
    assert over.sum() >= 2 and (want["nodes"][over] == 1).all() and not want["visits"][over].any()
    assert (want["root_wins"][over] % 64 == 0).all()  # 48 x 64 forced games, the same result each
    # the virtual loss spreads a round: no root child takes all of a round's walkers where there are several
    (rows, R, L, c, M), _ = cases.runs("small")
    want = cases.reference("small", rows, R, L, c, M)
    has_move = want["best_move"] < 64
    assert (want["visits"].sum(1)[has_move] == R * L).all() and (want["visits"].sum(1)[~has_move] == 0).all()
    assert (want["root_wins"][has_move] == want["wins"].sum(1)[has_move]).all()
    assert want["status"][-1] == mcts_ref.INVALID
    # the full tree: no expansion, every walker of a round ends in the 24 nodes
    (rows, R, L, c, big), (_, _, _, _, tiny) = cases.runs("long")
    full, cut = cases.reference("long", rows, R, L, c, big), cases.reference("long", rows, R, L, c, tiny)
    assert (cut["nodes"] <= tiny).all() and (full["nodes"] > tiny).all() and (cut["visits"].sum(1) == R * L).all()
    # the answer depends on L: 10 x 4 is not the one-wave search of 40 iterations
    one = mcts_cases.reference("small", 40, 0.5, mcts_ref.default_nodes(40))
    assert (one["visits"] != want["visits"]).any()


def test_the_row_alone_with_its_own_id_is_the_batchs_row(binary, tmp_path):
    rows, R, L, c, M = cases.runs("explore")[1]
    b, t = cases.inputs("explore", rows)
    want = cases.reference("explore", rows, R, L, c, M)
    for i in (1, 4):
        got = run(binary, tmp_path, b[i:i + 1], t[i:i + 1], R, L, c, M, game_id0=cases.GAME_ID0 + i * R * L * 64)
        for k in cases.FIELDS:
            assert (got[k][0] == want[k][i]).all(), (i, k)
