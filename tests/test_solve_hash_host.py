"""The split solver's transposition table on the host
(tools/diag/solve_hash_host.cpp: solve_hash_core.hpp's probe, store and hashed
machines with plain C++ rules).  Mode a, one thread: three task orders on one
table nothing clears, both move orders, against the exhaustive checker
(tests/solve_ref.py) at 3..8 empties, on the smallest table and on 2**16
entries.  Mode b, eight threads on the smallest table through atomics with the
device's orderings, against the checker and the deep fixture.  The subset
property: in forward task order the hashed search's nodes are no more than the
unhashed search's for every 13-empties root of the fixture, and fewer in total.
And the C-ABI (include/othello_solve_hash.h, othh_*) as a set.  CPU only."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import host_programs as hp
import solve_cases

from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
SOLVED = 1
SMALLEST = _lib.SOLVE_HASH_MIN_BITS
DEFAULT_NODES = _lib.SOLVE_TREE_DEFAULT_NODES
THREADS = 8


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "solve_hash_host")


def run(binary, tmp_path, mode, boards, turn, max_empties, task_empties, npp, order, bits, gate=1, task_orders=3,
        plain=0):
    """rows [n][runs][value, move, status, nodes] and the program's JSON line."""
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    hp.write_positions(inp, boards, turn)
    r = hp.run([binary, mode, inp, out, max_empties, task_empties, npp, order, bits, gate, task_orders, plain, THREADS])
    return hp.read_rows(out, (len(turn), -1, 4)), json.loads(r.stderr.strip().splitlines()[-1])


def checker_cases(lo, hi):
    cases = solve_cases.cases()
    keys = ("boards", "turn", "value", "best_move")
    return tuple(np.concatenate([cases[e][k] for e in range(lo, hi + 1)]) for k in keys)


def thirteen():
    fx = np.load(FIXTURE)
    sel = fx["empties"] == 13
    assert sel.sum() == 19
    return fx["boards"][sel], fx["turn"][sel], fx["value"][sel].astype(np.int64), fx["best_move"][sel]


def test_smallest_table_has_at_most_16_entries_and_the_largest_a_couple_of_gib():
    assert (1 << SMALLEST) <= 16
    assert 1 << 30 <= _lib.SOLVE_HASH_ENTRY_BYTES << _lib.SOLVE_HASH_MAX_BITS <= 4 << 30


@pytest.mark.parametrize("bits", [SMALLEST, 16])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("npp", [64, DEFAULT_NODES])
@pytest.mark.parametrize("task_empties", [1, 3])
def test_mode_a_matches_the_checker(binary, tmp_path, task_empties, npp, order, bits):
    """3..8 empties in one run, so the table also carries over from one
    emptiness to the next; hash_min_empties 1: every frame probes and stores."""
    b, t, rv, rm = checker_cases(3, 8)
    rows, _ = run(binary, tmp_path, "a", b, t, 16, task_empties, npp, order, bits, plain=1)
    assert rows.shape[1] == 4  # forward, reverse, shuffled on the table; forward without it
    for o in range(4):
        assert (rows[:, o, 2] == SOLVED).all(), o
        bad = np.nonzero((rows[:, o, 0] != rv) | (rows[:, o, 1] != rm))[0]
        assert len(bad) == 0, (o, bad[:8], rows[bad[:8], o], rv[bad[:8]], rm[bad[:8]])
    # the subset property on the way: forward with the table against forward without it
    assert (rows[:, 0, 3] <= rows[:, 3, 3]).all()


@pytest.mark.parametrize("order", [0, 1])
def test_mode_b_threads_on_the_smallest_table_match_the_checker(binary, tmp_path, order):
    b, t, rv, rm = checker_cases(6, 8)
    for task_empties in (1, 3):
        rows, info = run(binary, tmp_path, "b", b, t, 16, task_empties, DEFAULT_NODES, order, SMALLEST)
        assert info["threads"] == THREADS
        assert (rows[:, 0, 2] == SOLVED).all()
        assert (rows[:, 0, 0] == rv).all() and (rows[:, 0, 1] == rm).all(), task_empties


@pytest.mark.parametrize("order", [0, 1])
def test_mode_b_threads_match_the_fixture_at_13_empties(binary, tmp_path, order):
    b, t, rv, rm = thirteen()
    rows, _ = run(binary, tmp_path, "b", b, t, 13, 10, 512, order, SMALLEST)
    assert (rows[:, 0, 2] == SOLVED).all()
    assert (rows[:, 0, 0] == rv).all() and (rows[:, 0, 1] == rm).all()


@pytest.mark.parametrize("order", [0, 1])
def test_hashed_nodes_are_a_subset_of_the_unhashed(binary, tmp_path, order):
    """Forward task order, one thread, the fixture's 19 roots at 13 empties,
    tasks of 10 in slabs of 512, 2**20 entries, hash_min_empties 1.  The totals
    are DESIGN.md §19's (order 1: 4,866,420 nodes with the table against
    8,750,350 without; order 0: 10,093,366 against 24,114,811; some 13 s of
    one host thread for both)."""
    b, t, rv, rm = thirteen()
    rows, info = run(binary, tmp_path, "a", b, t, 13, 10, 512, order, 20, task_orders=1, plain=1)
    assert (rows[:, :, 2] == SOLVED).all()
    assert (rows[:, :, 0] == rv[:, None]).all() and (rows[:, :, 1] == rm[:, None]).all()
    hashed, unhashed = rows[:, 0, 3], rows[:, 1, 3]
    print("hashed", hashed.tolist(), "unhashed", unhashed.tolist())
    assert (hashed <= unhashed).all(), np.nonzero(hashed > unhashed)[0]
    assert hashed.sum() < unhashed.sum()
    assert info["hashed_nodes"] == hashed.sum() and info["unhashed_nodes"] == unhashed.sum()


# ---------------------------------------------------------------- the C-ABI
def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def test_hash_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.SOLVE_HASH_HEADER, "othh")
    assert names == ["othh_hash_bytes", "othh_solve_hashed"] == sorted(_lib.SOLVE_HASH_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (othh_\w+)$", out, re.M)) == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.SOLVE_HASH_SIGNATURES[name][1], name
        assert fn.restype == _lib.SOLVE_HASH_SIGNATURES[name][0], name
    # othe_solve's arguments, the table's four, the stream
    assert _lib.SOLVE_HASH_SIGNATURES["othh_solve_hashed"][1][:15] == _lib.SOLVE_TREE_SIGNATURES["othe_solve"][1][:15]
    for prefix in ("oth", "oths", "othm", "othp", "otht", "otho", "othe"):
        assert not header_functions(_lib.SOLVE_HASH_HEADER, prefix)


def test_hash_constants_match_the_binding_and_the_core():
    src = open(_lib.SOLVE_HASH_HEADER).read()

    def const(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, src).group(1))

    assert const("OTHH_MIN_BITS") == _lib.SOLVE_HASH_MIN_BITS
    assert const("OTHH_MAX_BITS") == _lib.SOLVE_HASH_MAX_BITS
    assert const("OTHH_ENTRY_BYTES") == _lib.SOLVE_HASH_ENTRY_BYTES == 32
    assert const("OTHH_MIN_EMPTIES_LO") == _lib.SOLVE_HASH_MIN_EMPTIES_LO == 1
    assert const("OTHH_MIN_EMPTIES_HI") == _lib.SOLVE_HASH_MIN_EMPTIES_HI == 12
    assert const("OTHH_DEFAULT_MIN_EMPTIES") == _lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES
    assert 4 <= _lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES <= 8
    core = open(os.path.join(ROOT, "subproc_amd", "csrc", "solve_hash_core.hpp")).read()
    for name, value in (("kMinBits", _lib.SOLVE_HASH_MIN_BITS), ("kMaxBits", _lib.SOLVE_HASH_MAX_BITS),
                        ("kDefaultGate", _lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES), ("kEntryBytes", 32)):
        assert re.search(r"%s = %d;" % (name, value), core), name
    assert "speed knob" in src.lower().replace("\n * ", " ") and "overlap" in src.lower()


def test_hash_bytes_agrees_with_the_table_class_and_bad_arguments_are_refused_before_any_launch():
    import torch

    from subproc_amd import ops

    lib = _lib.load()
    for bits in (_lib.SOLVE_HASH_MIN_BITS, 10, _lib.SOLVE_HASH_MAX_BITS):
        assert lib.othh_hash_bytes(bits) == _lib.SOLVE_HASH_ENTRY_BYTES << bits
    t = ops.SolveTable(10, device="cpu")  # (the class only; no call takes a host table)
    assert t.nbytes == lib.othh_hash_bytes(10) == t.data.numel() * 8 and t.bits == 10
    assert t.data.dtype == torch.int64 and int(t.data.abs().sum()) == 0
    E = _lib.OTH_EINVAL
    assert lib.othh_hash_bytes(_lib.SOLVE_HASH_MIN_BITS - 1) == E and lib.othh_hash_bytes(_lib.SOLVE_HASH_MAX_BITS + 1) == E
    for bits in (_lib.SOLVE_HASH_MIN_BITS - 1, _lib.SOLVE_HASH_MAX_BITS + 1):
        with pytest.raises(ValueError):
            ops.SolveTable(bits, device="cpu")
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    mem = (ctypes.c_uint64 * (4 * 16 + 4))()
    base = (ctypes.addressof(mem) + 31) & ~31
    w, b = ctypes.addressof(word), ctypes.addressof(boards)

    def call(bits=4, gate=6, table=base, size=512, n=0, task_empties=10):
        return lib.othh_solve_hashed(b, None, 14, task_empties, 0, 0, None, None, None, None, None, 0, 64, w, n, bits,
                                     gate, table, size, None)

    assert call() == _lib.OTH_OK  # n == 0: nothing launched
    assert call(bits=3) == E and call(bits=27) == E and call(gate=0) == E and call(gate=13) == E
    assert call(table=None) == E and call(table=base + 8) == E and call(size=511) == E
    assert call(bits=5, size=512) == E and call(bits=5, size=1024, table=None) == E
    assert call(task_empties=0) == E and call(n=-1) == E  # othe_solve's own checks hold
    assert call(n=1) == E  # valid table, no scratch
    assert word.value == 0
