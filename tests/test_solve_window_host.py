"""The exact solvers' root window on the host (tools/diag/solve_window_host.cpp:
solve_core.hpp's machine started with a window and solve_tree_core.hpp's tree
whose root hands its window down, with plain C++ rules).  DESIGN.md §20.

Mode a: the one-lane machine and the split cores in four task orders (forward,
reverse, shuffled, nothing shared) under both move orders, against
tests/window_ref.py at 0..8 empties for every position x every window family,
and against the deep fixture at 13 and 14 empties; the one-lane node count under
a window is never above the full window's.  The same under
-fsanitize=address,undefined.  Mode b: the hashed cores with windows, eight
threads on one table under -fsanitize=thread, a table filled by full-window
solves first and the other way round.  CPU only."""
import os

import numpy as np
import pytest

import host_programs as hp
import solve_cases
import window_ref

from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
SOLVED = _lib.SOLVE_SOLVED
THREADS = 8
RUNS = ["order %d, %s" % (o, k) for o in (0, 1) for k in ("forward", "reverse", "shuffled", "nothing shared")]


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_window_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_window_host", hp.SANITIZED)


@pytest.fixture(scope="module")
def binary_tsan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_window_host", hp.THREAD_SANITIZED)


def run(binary, tmp_path, args, boards, turn, alpha, beta):
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    hp.write_positions(inp, boards, turn, np.stack([np.asarray(alpha), np.asarray(beta)], axis=1))
    hp.run([binary, args[0], inp, out, *args[1:]])
    return hp.read_rows(out, (len(turn), -1))


def check_mode_a(rows, value, move, what):
    """the one-lane columns, then the eight split runs, against (value, move)"""
    assert rows.shape[1] == 5 + 3 * 8
    assert (rows[:, 2] == SOLVED).all(), what
    bad = np.nonzero((rows[:, 0] != value) | (rows[:, 1] != move))[0]
    assert len(bad) == 0, (what, "one lane", bad[:8], rows[bad[:8], :3], value[bad[:8]], move[bad[:8]])
    for k, name in enumerate(RUNS):
        s = rows[:, 5 + 3 * k:8 + 3 * k]
        assert (s[:, 2] == SOLVED).all(), (what, name)
        bad = np.nonzero((s[:, 0] != value) | (s[:, 1] != move))[0]
        assert len(bad) == 0, (what, name, bad[:8], s[bad[:8]], value[bad[:8]], move[bad[:8]])


@pytest.mark.parametrize("npp", [64, 4096])
@pytest.mark.parametrize("task_empties", [1, 3, 6])
def test_every_position_in_every_family_at_0_to_8_empties(binary, tmp_path, task_empties, npp):
    b, t, a, be, v, m, fam = window_ref.case_batch(0, 8)
    assert len(t) == 9 * sum(len(solve_cases.cases()[e]["turn"]) for e in range(9))  # no position, no family dropped
    rows = run(binary, tmp_path, ("a", 16, task_empties, npp, THREADS), b, t, a, be)
    check_mode_a(rows, v, m, (task_empties, npp))
    # alpha-beta with a fixed move order searches, under a narrower window, a subtree of the full window's
    assert (rows[:, 3] <= rows[:, 4]).all(), np.nonzero(rows[:, 3] > rows[:, 4])[0][:8]
    full = fam == 0
    assert (rows[full, 3] == rows[full, 4]).all() and rows[~full, 3].sum() < rows[~full, 4].sum()


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    b, t, a, be, v, m, fam = window_ref.case_batch(0, 7)
    rows = run(binary_asan, tmp_path, ("a", 16, 3, 4096, 1), b, t, a, be)
    check_mode_a(rows, v, m, "asan")
    bad = np.array([[0, 0], [3, 3], [5, -5], [66, 67], [-66, 0]])
    rows = run(binary_asan, tmp_path, ("a", 16, 3, 4096, 1), b[:5], t[:5], bad[:, 0], bad[:, 1])
    want = [0, 255, _lib.SOLVE_BADWINDOW]
    assert (rows[:, :3] == want).all() and (rows[:, 3] == 0).all()
    assert (rows[:, 5:].reshape(5, 8, 3) == want).all()


def deep():
    fx = np.load(FIXTURE)
    sel = fx["empties"] <= 14
    assert sel.sum() == 28
    return fx["boards"][sel], fx["turn"][sel], fx["value"][sel].astype(np.int64), fx["best_move"][sel].astype(np.int64)


def test_the_deep_fixture_at_13_and_14_empties(binary, tmp_path):
    """(-1, 1), (V - 1, V + 1) and the two families with V on a bound.  The
    values are clamp(V); the move is checked where the fixture determines it:
    inside the window its own, 255 on a fail-low, 64 at a forced pass.  On a
    fail-high the nine runs must agree with each other."""
    b, t, V, M = deep()
    bb, tt, aa, be, vv, mm, kk = [], [], [], [], [], [], []
    for name in ("wld", "around") + window_ref.ON_BOUND:
        a, c, keep = window_ref.family(name, V)
        assert keep.all()
        known = (M == 64) | (V <= a) | (V < c)
        bb.append(b), tt.append(t), aa.append(a), be.append(c), vv.append(np.clip(V, a, c)), kk.append(known)
        mm.append(np.where(M == 64, 64, np.where(V <= a, 255, M)))
    bb, tt, aa, be, vv, mm, kk = (np.concatenate(x) for x in (bb, tt, aa, be, vv, mm, kk))
    rows = run(binary, tmp_path, ("a", 14, 10, 512, THREADS), bb, tt, aa, be)
    assert (rows[:, 2] == 0).all()  # above 12 empties the one-lane machine skips
    runs = rows[:, 5:].reshape(len(tt), 8, 3)
    assert (runs[:, :, 2] == SOLVED).all()
    assert (runs[:, :, 0] == vv[:, None]).all()
    assert (runs[kk][:, :, 1] == mm[kk][:, None]).all()
    assert (runs[:, :, 1] == runs[:, :1, 1]).all()
    assert (~kk).sum() > 0 and (runs[~kk][:, 0, 1] < 64).all()


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("bits", [_lib.SOLVE_HASH_MIN_BITS, 20])
def test_hashed_cores_with_windows_under_the_thread_sanitizer(binary_tsan, tmp_path, bits, phase):
    """Phase 0: every position under the full window first, then under its own,
    on the one table; phase 1 the other way round.  hash_min_empties 1: every
    frame probes and stores.  Both move orders."""
    b, t, a, be, v, m, fam = window_ref.case_batch(8, 8)
    c = solve_cases.cases()[8]
    fv = np.concatenate([c["value"]] * 9).astype(np.int64)
    fm = np.concatenate([c["best_move"]] * 9).astype(np.int64)
    assert len(fv) == len(t)
    for order in (0, 1):
        rows = run(binary_tsan, tmp_path, ("b", 16, 3, 4096, order, bits, 1, phase, THREADS), b, t, a, be)
        assert (rows[:, 2] == SOLVED).all() and (rows[:, 5] == SOLVED).all()
        assert (rows[:, 0] == v).all() and (rows[:, 1] == m).all(), order
        assert (rows[:, 3] == fv).all() and (rows[:, 4] == fm).all(), order
