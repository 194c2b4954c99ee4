"""The per-move values on the host (tools/diag/moves_host.cpp: moves.hip's
expand / tasks / finish scheme in plain C++ around solve_core.hpp's machine and
search_core.hpp's machine started by start_child()), against tests/moves_ref.py.
DESIGN.md §21.

Exact rows at 0..8 empties; search rows of mid3, mid4 and special3 with both
tables at depths 1..4; depth 8 at 6 empties, where the rows are T times the
exact ones.  The same under -fsanitize=address,undefined, as a process of its
own.  CPU only."""
import numpy as np
import pytest

import host_programs as hp
import moves_ref
import solve_cases
import tree_cases

from subproc_amd import _lib

T = moves_ref.T


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "moves_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "moves_host", hp.SANITIZED)


def run(binary, tmp_path, mode, boards, turn, level, weights=None, limit=0):
    """(value, move, status, nodes, rows (n, 64)) of the host program."""
    inp, out, wf = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "w")
    hp.write_positions(inp, boards, turn)
    args = [binary, mode, inp, out]
    if mode == "search":
        hp.write_weights(wf, weights)
        args.append(wf)
    hp.run(args + [level, limit, 8])
    a = hp.read_rows(out, (len(turn), 68))
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4:]


def check(got, want, status, what):
    value, move, st, nodes, rows = got
    wrows, wvalue, wmove = want
    assert (st == status).all(), what
    assert (rows == wrows).all(), (what, np.nonzero((rows != wrows).any(axis=1))[0][:8])
    assert (value == wvalue).all() and (move == wmove).all(), what
    # a task per legal move, one for a pass
    fill = moves_ref.NOT_A_MOVE32 if (wrows == moves_ref.NOT_A_MOVE32).any() else moves_ref.NOT_A_MOVE
    tasks = np.maximum((wrows != fill).sum(axis=1), wmove == 64)
    assert (nodes >= tasks).all(), what


def exact_batch(hi):
    b, t, rows, value, move, forced, over = moves_ref.exact_cases(0, hi)
    assert len(t) == sum(len(solve_cases.cases()[e]["turn"]) for e in range(hi + 1))  # no position dropped
    assert forced.any() and over.any()
    return b, t, (rows, value, move)


def test_exact_rows_at_0_to_8_empties(binary, tmp_path):
    b, t, want = exact_batch(8)
    check(run(binary, tmp_path, "solve", b, t, 8), want, _lib.SOLVE_SOLVED, "solve")
    # more empties than max_empties: skipped, the row empty
    value, move, st, nodes, rows = run(binary, tmp_path, "solve", b, t, 5)
    big = np.array([64 - bin(int(x) | int(y)).count("1") > 5 for x, y in b.tolist()])
    assert big.any() and (st[big] == _lib.SOLVE_SKIPPED).all() and (st[~big] == _lib.SOLVE_SOLVED).all()
    assert (rows[big] == moves_ref.NOT_A_MOVE).all() and (value[big] == 0).all() and (move[big] == 255).all()
    assert (nodes[big] == 0).all() and (rows[~big] == want[0][~big]).all()


SEARCH_CASES = [(name, depth, table) for name in ("mid3", "mid4", "special3") for table in tree_cases.BOTH
                for depth in (1, 2, 3, 4)]


@pytest.mark.parametrize("name,depth,table", SEARCH_CASES)
def test_search_rows(binary, tmp_path, name, depth, table):
    b, t = tree_cases.inputs(name)
    assert len(t) == tree_cases.MID_ROOTS.get(name, len(t)) and len(t) >= 32
    got = run(binary, tmp_path, "search", b, t, depth, tree_cases.TABLES[table])
    check(got, moves_ref.search_case(name, depth, table), _lib.SEARCH_SEARCHED, (name, depth, table))


def test_depth_8_at_6_empties_is_the_exact_rows_times_T(binary, tmp_path):
    c = solve_cases.cases()[6]
    rows, value, move = moves_ref.exact(moves_ref.window_ref.case_roots(6))
    assert len(value) == len(c["turn"]) >= 256
    want = (np.where(rows == moves_ref.NOT_A_MOVE, moves_ref.NOT_A_MOVE32, rows * T), value * T, move)
    for table in tree_cases.BOTH:
        got = run(binary, tmp_path, "search", c["boards"], c["turn"], 8, tree_cases.TABLES[table])
        check(got, want, _lib.SEARCH_SEARCHED, table)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    b, t, want = exact_batch(7)
    check(run(binary_asan, tmp_path, "solve", b, t, 7), want, _lib.SOLVE_SOLVED, "asan solve")
    for name, depth, table in (("mid3", 3, "rng7"), ("mid4", 4, "default"), ("special3", 3, "rng7"),
                               ("special3", 1, "default")):
        bb, tt = tree_cases.inputs(name)
        got = run(binary_asan, tmp_path, "search", bb, tt, depth, tree_cases.TABLES[table])
        check(got, moves_ref.search_case(name, depth, table), _lib.SEARCH_SEARCHED, ("asan", name, depth))
    c = solve_cases.cases()[6]
    got = run(binary_asan, tmp_path, "search", c["boards"][:64], c["turn"][:64], 8, tree_cases.TABLES["default"])
    assert (got[2] == _lib.SEARCH_SEARCHED).all()
    # an overlapping board and a node limit of one: INVALID, and every move with a subtree unknown
    bad = np.array([[3, 1]], np.uint64)
    value, move, st, nodes, rows = run(binary_asan, tmp_path, "solve", bad, [1], 12)
    assert st[0] == _lib.SOLVE_INVALID and (rows == moves_ref.NOT_A_MOVE).all() and move[0] == 255
    bb, tt = tree_cases.inputs("mid3")
    value, move, st, nodes, rows = run(binary_asan, tmp_path, "search", bb, tt, 3, tree_cases.TABLES["default"], limit=1)
    assert (st == _lib.SEARCH_LIMIT).all() and (value == 0).all() and (move == 255).all()
    assert ((rows == moves_ref.UNKNOWN32) | (rows == moves_ref.NOT_A_MOVE32)).all()
