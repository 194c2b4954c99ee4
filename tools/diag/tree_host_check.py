#!/usr/bin/env python
"""Run the host build of the split search (tools/diag/tree_host.cpp, usually
built with -fsanitize=address,undefined) on every input of the GPU tests'
checker comparisons (tests/tree_cases.py), on the tied roots and with the
smallest slab, and compare value, move and status of all four task orders
(forward, reverse, shuffled, nothing shared) with tests/search_ref.py.  CPU
only; meant to be run before the kernels' first GPU run after a change to
tree_core.hpp.

    python tools/diag/tree_host_check.py [BINARY=tools/diag/tree_host_asan] [case ...]
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_programs as hp  # noqa: E402
import search_ref  # noqa: E402
import solve_cases  # noqa: E402
import tree_cases  # noqa: E402

SEARCHED, NOROOM = 1, 4
ORDERS = ("forward", "reverse", "shuffled", "nothing shared")


def run(binary, boards, turn, weights, depth, split, npp=32768, node_limit=1 << 22, seed=1):
    """(value, move, status, nodes), each [4 orders][n]."""
    with tempfile.TemporaryDirectory() as d:
        inp, out, wf = (os.path.join(d, x) for x in ("in", "out", "w"))
        hp.write_positions(inp, boards, turn)
        hp.write_weights(wf, weights, end="\n")
        sys.stderr.write(hp.run([binary, inp, out, wf, depth, split, npp, node_limit, seed]).stderr)
        return hp.read_rows(out, orders=4)


def compare(label, got, rv, rm, allow_noroom=False):
    v, m, s, nd = got
    bad = 0
    for o, name in enumerate(ORDERS):
        ok = (s[o] == SEARCHED) & (v[o] == rv) & (m[o] == rm)
        if allow_noroom:
            ok |= (s[o] == NOROOM) & (v[o] == 0) & (m[o] == 255)
            same = (s[o] == s[0]).all()
        else:
            same = True
        if not ok.all() or not same:
            bad += 1
            i = int(np.nonzero(~ok)[0][0]) if not ok.all() else -1
            print("  %s, %s: DIFFERS at %d: got %s, checker %s" % (
                label, name, i, (v[o][i], m[o][i], s[o][i]), (rv[i], rm[i])), flush=True)
    return bad, nd


def main(argv):
    binary = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tools", "diag", "tree_host_asan")
    want = argv[2:]
    bad = 0
    for name, (depth, splits, tables) in tree_cases.CASES.items():
        if want and name not in want:
            continue
        b, t = tree_cases.inputs(name)
        for table in tables:
            t0 = time.time()
            rv, rm, _ = tree_cases.reference(name, table)
            t1 = time.time()
            for split in splits:
                for npp in (32768, 64):
                    label = "%s %s depth %d split %d slab %d" % (name, table, depth, split, npp)
                    t2 = time.time()
                    wrong, nd = compare(label, run(binary, b, t, tree_cases.TABLES[table], depth, split, npp), rv, rm,
                                        allow_noroom=npp == 64)
                    bad += wrong
                    print("%-44s %4d roots  host %.1f s  checker %.1f s  nodes fwd/rev/shuf/none %s  %s" % (
                        label, len(t), time.time() - t2, t1 - t0, "/".join(str(int(x.sum())) for x in nd),
                        "DIFFERS" if wrong else "equal"), flush=True)
    if not want or "ties" in want:
        ob, ot = tree_cases.opening_ties()
        for depth, value in ((4, 560), (5, 900), (6, 660)):
            rv, rm, _ = search_ref.search(ob, ot, depth, tree_cases.TABLES["default"])
            assert rv[0] == value and rm[0] == 19 and (rv == value).all(), (rv, rm)
            for split in (1, 2, 3):
                label = "opening x16 depth %d split %d" % (depth, split)
                wrong, _ = compare(label, run(binary, ob, ot, tree_cases.TABLES["default"], depth, split), rv, rm)
                bad += wrong
                print("%-44s %s" % (label, "DIFFERS" if wrong else "equal"), flush=True)
        p = solve_cases.pool()[2]
        b, t = p["boards"][:64], p["turn"][:64]
        rv, rm, _ = search_ref.search(b, t, 2, tree_cases.TABLES["default"])
        wrong, _ = compare("two empties", run(binary, b, t, tree_cases.TABLES["default"], 2, 1), rv, rm)
        bad += wrong
        print("%-44s %s" % ("two empties x64 depth 2 split 1", "DIFFERS" if wrong else "equal"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
