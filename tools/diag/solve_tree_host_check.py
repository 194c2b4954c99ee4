#!/usr/bin/env python
"""Run the host build of the split solver (tools/diag/solve_tree_host.cpp,
usually built with -fsanitize=address,undefined) on every input of the GPU
tests (tests/test_gpu_solve_tree.py) and compare value, move and status of all
four task orders (forward, reverse, shuffled, nothing shared) at move order 0
and 1 with tests/solve_ref.py (0..9 empties), with the deep fixture
(tests/golden/solve_deep/solve_deep.npz, 13..16 empties) and, on the roots the
GPU tests compare with the one-lane solver, with each other.  The binary runs
as a child process: nothing is loaded into Python under a sanitizer.  CPU
only; meant to be run before the kernels' first GPU run after a change to
solve_tree_core.hpp or solve_order_core.hpp.

    python tools/diag/solve_tree_host_check.py [BINARY=tools/diag/solve_tree_host_asan] [quick]

quick: the fixture's 13-empties roots only, at task_empties 10 (what a
sanitizer build gets through in a few minutes).
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_programs as hp  # noqa: E402
import solve_cases  # noqa: E402

SOLVED, NOROOM = 1, 4
DEFAULT_NODES = 65536
ORDERS = ("forward", "reverse", "shuffled", "nothing shared")
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")


def run(binary, boards, turn, max_empties, task_empties, npp=DEFAULT_NODES, node_limit=0, seed=1, order=0, threads=16,
        task_orders=4):
    """(value, move, status, nodes), each [task_orders][n]."""
    with tempfile.TemporaryDirectory() as d:
        inp, out = os.path.join(d, "in"), os.path.join(d, "out")
        hp.write_positions(inp, boards, turn)
        hp.run([binary, inp, out, max_empties, task_empties, npp, node_limit, seed, order, threads, task_orders])
        return hp.read_rows(out, orders=task_orders)


def compare(label, got, rv, rm, allow_noroom=False):
    v, m, s, nd = got
    bad = 0
    for o in range(len(v)):
        ok = (s[o] == SOLVED) & (v[o] == rv) & (m[o] == rm)
        same = True
        if allow_noroom:
            ok |= (s[o] == NOROOM) & (v[o] == 0) & (m[o] == 255)
            same = (s[o] == s[0]).all()
        if not ok.all() or not same:
            bad += 1
            i = int(np.nonzero(~ok)[0][0]) if not ok.all() else -1
            print("  %s, %s: DIFFERS at %d: got %s, expected %s" % (
                label, ORDERS[o], i, (v[o][i], m[o][i], s[o][i]), (rv[i], rm[i])), flush=True)
    return bad, nd


def main(argv):
    binary = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tools", "diag", "solve_tree_host_asan")
    quick = "quick" in argv[2:]
    bad = 0
    cases = solve_cases.cases()
    for e in sorted(cases):
        c = cases[e]
        for task_empties in (1, 3, 6):
            for npp in (DEFAULT_NODES, 64):
                for order in (0, 1):
                    label = "cases %d empties, task %d, slab %d, order %d" % (e, task_empties, npp, order)
                    t0 = time.time()
                    wrong, nd = compare(label, run(binary, c["boards"], c["turn"], 16, task_empties, npp, order=order),
                                        c["value"], c["best_move"])
                    bad += wrong
                    print("%-52s %4d roots %.1f s  nodes %s  %s" % (
                        label, len(c["turn"]), time.time() - t0, "/".join(str(int(x.sum())) for x in nd),
                        "DIFFERS" if wrong else "equal"), flush=True)
    # the roots the GPU tests compare with the one-lane solver: no checker reaches them, so every configuration
    # must agree with the first one (the GPU test then pins that one to oths_solve)
    for e, k in ((10, 64), (12, 16)):
        b, t = solve_cases.ladder(e, k)
        first = None
        for task_empties in (4, 8, 12):
            for order in (0, 1):
                label = "ladder(%d, %d), task %d, order %d" % (e, k, task_empties, order)
                got = run(binary, b, t, e, task_empties, order=order)
                if first is None:
                    first = (got[0][0], got[1][0])
                wrong, nd = compare(label, got, first[0], first[1])
                bad += wrong
                print("%-52s %4d roots  nodes %s  %s" % (label, k, "/".join(str(int(x.sum())) for x in nd),
                                                         "DIFFERS" if wrong else "equal"), flush=True)
    fx = np.load(FIXTURE)
    # all four task orders up to 13 (quick: what a sanitizer build gets through in minutes) or 14 empties; the
    # roots above forward and reversed only (at 14 empties the shuffled and the unshared runs already make 8 and 19
    # times the forward run's nodes)
    top = 13 if quick else 14
    for lo, hi, task_orders in ((13, top, 4),) + (() if quick else ((15, 16, 2),)):
        sel = (fx["empties"] >= lo) & (fx["empties"] <= hi)
        b, t, rv, rm = fx["boards"][sel], fx["turn"][sel], fx["value"][sel].astype(np.int64), fx["best_move"][sel]
        for task_empties in ((10,) if quick else (8, 10, 12)):
            for npp in (DEFAULT_NODES, 1024, 64) if task_orders == 4 else (DEFAULT_NODES,):
                for order in (0, 1):
                    label = "fixture %d..%d, task %d, slab %d, order %d" % (lo, hi, task_empties, npp, order)
                    t0 = time.time()
                    got = run(binary, b, t, 16, task_empties, npp, order=order, threads=16, task_orders=task_orders)
                    wrong, nd = compare(label, got, rv, rm, allow_noroom=npp != DEFAULT_NODES)
                    bad += wrong
                    print("%-52s %4d roots %.1f s  nodes %s  %s" % (
                        label, len(t), time.time() - t0, "/".join(str(int(x.sum())) for x in nd),
                        "DIFFERS" if wrong else "equal"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
