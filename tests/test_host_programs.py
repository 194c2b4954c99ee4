"""tests/host_programs.py and tools/diag/host_io.hpp, the two halves of the host
programs' harness: every tools/diag/*_host.cpp compiles and
states its usage, a positions file written here is read there and the rows
written there are read here, and run() fails what it must.  CPU only."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import host_programs as hp
import perft_ref
import search_ref
import solve_cases
import solve_ref
import tree_cases

PROGRAMS = sorted(os.path.basename(p)[:-len(".cpp")] for p in glob.glob(os.path.join(hp.DIAG, "*_host.cpp")))
SOLVED = SEARCHED = 1
SKIPPED, INVALID = 0, 2


def test_the_glob_finds_the_programs():
    assert len(PROGRAMS) >= 14 and {"solve_host", "search_host", "mcts_tree_host"} <= set(PROGRAMS)


@pytest.mark.parametrize("program", PROGRAMS)
def test_every_program_compiles_and_without_arguments_states_its_usage(tmp_path_factory, tmp_path, program):
    exe = hp.compiled(tmp_path_factory, program)
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("usage: ") and r.stdout == ""
    assert os.listdir(tmp_path) == []


def positions():
    """The opening for each side, a finished board (all black), an overlapping board."""
    ob, _ = perft_ref.opening()
    b = np.array([ob[0], ob[0], [0xFFFFFFFFFFFFFFFF, 0], [3, 1]], np.uint64)
    return b, np.array([1, 2, 1, 1], np.uint8)


def test_positions_written_here_are_read_there_and_the_rows_come_back(tmp_path_factory, tmp_path):
    b, t = positions()
    inp, out, wf = (str(tmp_path / x) for x in ("in", "out", "w"))
    hp.write_positions(inp, b, t)
    assert open(inp).read().splitlines()[2:] == ["ffffffffffffffff 0 1", "3 1 1"]
    # search_host at depth 1: the three valid boards are the exhaustive checker's, the overlap INVALID
    w = tree_cases.TABLES["default"]
    hp.write_weights(wf, w)
    hp.run([hp.compiled(tmp_path_factory, "search_host"), inp, out, wf, 1, 0, 2])
    rows = hp.read_rows(out, (4, 4))
    v, m, _ = search_ref.search(b[:3], t[:3], 1, w)
    assert rows[:, 2].tolist() == [SEARCHED, SEARCHED, SEARCHED, INVALID]
    assert (rows[:3, 0] == v).all() and (rows[:3, 1] == m).all() and rows[3, :2].tolist() == [0, 255]
    assert rows[2, 0] == 64 * search_ref.T and rows[2, 1] == 255 and rows[0, 1] != rows[1, 1]
    # solve_host: the opening has more empties than any max_empties and is SKIPPED, which is not the issue of
    # this test; the finished board is solve_ref's, and so are two boards of three empties added for it
    hp.run([hp.compiled(tmp_path_factory, "solve_host"), inp, out, 12, 0, 2])
    rows = hp.read_rows(out, (4, 4))
    v, m, _ = solve_ref.solve(b[2:3], t[2:3])
    assert rows[:, 2].tolist() == [SKIPPED, SKIPPED, SOLVED, INVALID]
    assert rows[2, 0] == v[0] == 64 and rows[2, 1] == m[0] == 255
    c = solve_cases.cases()[3]
    hp.write_positions(inp, c["boards"][:2], c["turn"][:2])
    hp.run([hp.compiled(tmp_path_factory, "solve_host"), inp, out, 12, 0, 2])
    rows = hp.read_rows(out, (2, 4))
    assert (rows[:, 2] == SOLVED).all() and (rows[:, 0] == c["value"][:2]).all() and (rows[:, 1] == c["best_move"][:2]).all()


def test_the_extra_columns_and_the_order_option_of_read_rows(tmp_path):
    b, t = positions()
    path = str(tmp_path / "p")
    hp.write_positions(path, b[:2], t[:2], [7, 9])
    assert [ln.split()[3] for ln in open(path)] == ["7", "9"]
    hp.write_positions(path, b[:2], t[:2], np.array([[-1, 1], [-64, 64]]))
    assert [ln.split()[3:] for ln in open(path)] == [["-1", "1"], ["-64", "64"]]
    with open(path, "w") as f:
        f.write("1 2 3 4 5 6 7 8\n9 10 11 12 13 14 15 16\nlevels 2\n")
    rows, last = hp.read_rows(path, trailer=True)
    assert rows.shape == (2, 8) and last == ["levels", "2"]
    with open(path, "w") as f:
        f.write("1 2 3 4 5 6 7 8\n9 10 11 12 13 14 15 16\n")
    value, move, status, nodes = hp.read_rows(path, orders=2)
    assert value.tolist() == [[1, 9], [5, 13]] and nodes.tolist() == [[4, 12], [8, 16]]


def test_run_fails_a_non_zero_exit_status_and_a_sanitizers_report(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "solve_host")
    with pytest.raises(AssertionError, match="exit status 1"):
        hp.run([exe, tmp_path / "missing", tmp_path / "out"])
    assert not os.path.exists(tmp_path / "out")
    # a stub that only prints the word: nothing runs under a sanitizer here
    stub = [sys.executable, "-c", "import sys; sys.stderr.write('==1==ERROR: AddressSanitizer: stub\\n')"]
    with pytest.raises(AssertionError, match="AddressSanitizer: stub"):
        hp.run(stub)
    assert hp.run([sys.executable, "-c", "import sys; sys.stderr.write('fine\\n')"]).stderr == "fine\n"
