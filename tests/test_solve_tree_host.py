"""The split solver's cores on the host (tools/diag/solve_tree_host.cpp: plain
C++ rules, plain loads and stores): all four task orders (forward, reverse,
shuffled, nothing shared) and both move orders against the exhaustive checker
(tests/solve_ref.py) at 3..8 empties and against the deep fixture
(tests/golden/solve_deep/solve_deep.npz) at 13 and 14 empties.  CPU only."""
import os

import numpy as np
import pytest

import host_programs as hp
import solve_cases
import solve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
SOLVED, NOROOM = 1, 4
DEFAULT_NODES = 65536
THREADS = 8


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_tree_host")


def run(binary, tmp_path, boards, turn, max_empties, task_empties, npp, order):
    """(value, move, status), each [4 task orders][n]."""
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    hp.write_positions(inp, boards, turn)
    hp.run([binary, inp, out, max_empties, task_empties, npp, 0, 7, order, THREADS])
    return hp.read_rows(out, orders=4)[:3]


def test_the_default_slab_is_the_bindings():
    from subproc_amd import _lib

    assert DEFAULT_NODES == _lib.SOLVE_TREE_DEFAULT_NODES


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("npp", [64, DEFAULT_NODES])
@pytest.mark.parametrize("task_empties", [1, 3])
def test_host_build_matches_the_checker(binary, tmp_path, task_empties, npp, order):
    cases = solve_cases.cases()
    for e in range(3, 9):
        c = cases[e]
        v, m, s = run(binary, tmp_path, c["boards"], c["turn"], 16, task_empties, npp, order)
        for o in range(4):
            # (at most 8 empties: whatever the slab, no task has more than 12)
            assert (s[o] == SOLVED).all(), (e, o)
            bad = np.nonzero((v[o] != c["value"]) | (m[o] != c["best_move"]))[0]
            assert len(bad) == 0, (e, o, bad[:8], v[o][bad[:8]], c["value"][bad[:8]], m[o][bad[:8]],
                                   c["best_move"][bad[:8]])


def test_the_fixture_is_what_it_claims():
    fx = np.load(FIXTURE)
    assert set(fx.files) == {"boards", "turn", "empties", "value", "best_move"}
    assert len(fx["turn"]) == 38 and os.path.getsize(FIXTURE) < 16384
    emp = solve_ref.empties(fx["boards"])
    assert (emp == fx["empties"]).all()
    assert [int((emp == e).sum()) for e in (13, 14, 15, 16)] == [16 + 3, 8 + 1, 4 + 0, 4 + 2]
    assert int((fx["best_move"] == 64).sum()) == 6 and (fx["best_move"] != 255).all()
    at = 0
    for e, k in ((13, 16), (14, 8), (15, 4), (16, 4)):
        b, t = solve_cases.ladder(e, k)
        assert (fx["boards"][at:at + k] == b).all() and (fx["turn"][at:at + k] == t).all()
        at += k
    for e in range(13, 17):
        p = solve_cases.pool()[e]
        k = int(p["forced_pass"].sum())
        assert (fx["boards"][at:at + k] == p["boards"][p["forced_pass"]]).all()
        at += k
    assert at == 38


@pytest.mark.parametrize("order", [0, 1])
def test_host_build_matches_the_fixture_at_13_and_14_empties(binary, tmp_path, order):
    """In a slab of 512 nodes: two levels of every one of these roots fit (three of the forced passes), so no task
    has more than 12 empties and some have more than task_empties; with the default slab the shuffled and the
    unshared runs make 1.1e9 nodes for these 28 roots, 4.4e8 here (tools/diag/solve_tree_host_check.py runs the
    default slab too)."""
    fx = np.load(FIXTURE)
    sel = fx["empties"] <= 14
    assert sel.sum() == 28
    v, m, s = run(binary, tmp_path, fx["boards"][sel], fx["turn"][sel], 14, 10, 512, order)
    for o in range(4):
        assert (s[o] == SOLVED).all(), o
        assert (v[o] == fx["value"][sel]).all() and (m[o] == fx["best_move"][sel]).all(), o
