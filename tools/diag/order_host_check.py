#!/usr/bin/env python
"""Run the host builds of the three searches (tools/diag/search_host.cpp,
play_host.cpp, tree_host.cpp; usually built stand-alone with
-fsanitize=address,undefined) with order = 1 on every input of the GPU tests'
comparisons (tests/order_cases.py, tests/tree_cases.py) and compare them with
the checkers (tests/search_ref.py, tests/play_ref.py, which know no order) and
with order = 0.  CPU only; meant to be run before the ordered kernels' first GPU
run after a change to order_core.hpp.

    python tools/diag/order_host_check.py [DIR=tools/diag] [SUFFIX=_asan] [part ...]

parts: search versus end ties play tree ratio (default: all but ratio, which
runs the 4,096 roots at depth 5 and wants the optimised build: SUFFIX "")
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import host_programs as hp  # noqa: E402
import order_cases  # noqa: E402
import play_host_check  # noqa: E402
import search_ref  # noqa: E402
import solve_cases  # noqa: E402
import tree_cases  # noqa: E402
import tree_host_check  # noqa: E402

T = search_ref.T
LIMIT = 1 << 26


def search(binary, boards, turn, depth, weights, order, node_limit=LIMIT, threads=8):
    """(value, move, status, nodes) of search_host."""
    with tempfile.TemporaryDirectory() as d:
        inp, out, wf = (os.path.join(d, x) for x in ("in", "out", "w"))
        hp.write_positions(inp, boards, turn)
        hp.write_weights(wf, weights, end="\n")
        hp.run([binary, inp, out, wf, depth, node_limit, threads, order])
        rows = hp.read_rows(out, (-1, 4))
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def tree(binary, boards, turn, weights, depth, split, npp, order):
    """tree_host_check.run with the order argument: (value, move, status, nodes), each [4 task orders][n]."""
    with tempfile.TemporaryDirectory() as d:
        inp, out, wf = (os.path.join(d, x) for x in ("in", "out", "w"))
        hp.write_positions(inp, boards, turn)
        hp.write_weights(wf, weights, end="\n")
        sys.stderr.write(hp.run([binary, inp, out, wf, depth, split, npp, 1 << 22, 1, order]).stderr)
        return hp.read_rows(out, orders=4)


def play(binary, c, boards, turn, order, threads=8, tables=order_cases.TABLES):
    return play_host_check.play(binary, c, boards, turn, tables, threads, order)


def report(label, ok, extra=""):
    print("%-52s %s %s" % (label, "equal" if ok else "DIFFERS", extra), flush=True)
    return 0 if ok else 1


def main(argv):
    where = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tools", "diag")
    suffix = argv[2] if len(argv) > 2 else "_asan"
    parts = argv[3:] or ["search", "versus", "end", "ties", "play", "tree"]
    sh, ph, th = (os.path.join(where, x + "_host" + suffix) for x in ("search", "play", "tree"))
    bad = 0
    if "search" in parts:  # against the checker
        for depth in sorted(order_cases.MID):
            b, t = order_cases.mid(depth)
            for table in order_cases.BOTH:
                rv, rm = order_cases.mid_reference(depth, table)
                v, m, s, nd = search(sh, b, t, depth, order_cases.TABLES[table], 1)
                bad += report("checker: midgame depth %d %s x%d" % (depth, table, len(t)),
                              (s == 1).all() and (v == rv).all() and (m == rm).all())
    if "versus" in parts:  # against order 0 (the sanitised build takes the first 512 of the large sets)
        for depth in sorted(order_cases.VERSUS):
            b, t = order_cases.versus(depth)
            if suffix and depth >= 4:  # (the optimised build, SUFFIX "", runs all 4,096 at every depth)
                b, t = b[:512 >> (depth - 4)], t[:512 >> (depth - 4)]
            t0 = time.time()
            r0 = search(sh, b, t, depth, order_cases.TABLES["default"], 0)
            r1 = search(sh, b, t, depth, order_cases.TABLES["default"], 1)
            ok = all((x == y).all() for x, y in zip(r0[:3], r1[:3]))
            bad += report("order 0: midgame depth %d x%d" % (depth, len(t)), ok,
                          "nodes %d -> %d (%.3f)  %.1f s" % (r0[3].sum(), r1[3].sum(), r1[3].sum() / r0[3].sum(),
                                                            time.time() - t0))
    if "end" in parts:
        b, t = order_cases.endgame(8)
        cs = solve_cases.cases()
        sv = np.concatenate([cs[e]["value"] for e in sorted(cs) if e <= 8]).astype(np.int64)
        sm = np.concatenate([cs[e]["best_move"] for e in sorted(cs) if e <= 8])
        v, m, s, nd = search(sh, b, t, 8, order_cases.TABLES["default"], 1)
        bad += report("solver: <= 8 empties depth 8 x%d" % len(t),
                      (s == 1).all() and (v == T * sv).all() and (m == sm).all())
        b, t = order_cases.endgame(10)
        r0 = tree(th, b, t, order_cases.TABLES["default"], 10, 2, 32768, 0)
        r1 = tree(th, b, t, order_cases.TABLES["default"], 10, 2, 32768, 1)
        ok = all((r1[k] == r0[k][0]).all() for k in range(3)) and (r1[0][0][:len(sv)] == T * sv).all() and (
            r1[1][0][:len(sv)] == sm).all()
        bad += report("solver and order 0: <= 10 empties depth 10 split 2 x%d" % len(t), ok)
    if "ties" in parts:
        ob, ot = tree_cases.opening_ties()
        for depth in (4, 5, 6):
            rv, rm, _ = search_ref.search(ob, ot, depth, order_cases.TABLES["default"])
            v, m, s, _ = search(sh, ob, ot, depth, order_cases.TABLES["default"], 1)
            bad += report("ties: opening x16 depth %d" % depth, (v == rv).all() and (m == rm).all())
        b, t, rv, rm, later = order_cases.two_empties()
        v, m, s, _ = search(sh, b, t, 2, order_cases.TABLES["default"], 1)
        bad += report("ties: two empties x64 depth 2", (v == rv).all() and (m == rm).all(),
                      "(%d with the lowest maximiser in a later class)" % later.sum())
        for table in order_cases.BOTH:
            b, t, rv, rm, later = order_cases.depth1_ties(table)
            v, m, s, _ = search(sh, b, t, 1, order_cases.TABLES[table], 1)
            bad += report("ties: depth 1 %s x%d" % (table, len(t)), (v == rv).all() and (m == rm).all(),
                          "(%d with the lowest maximiser in a later class)" % later.sum())
        for depth, roots in ((3, 1024), (4, 128)):
            b, t, rv, rm = order_cases.mobility_ties(depth, roots)
            v, m, s, _ = search(sh, b, t, depth, order_cases.TABLES["default"], 1)
            bad += report("ties: mobility-ordered roots, depth %d x%d" % (depth, len(t)),
                          (v == rv).all() and (m == rm).all())
    if "play" in parts:
        keys = ("a_black", "final_boards", "diff", "plies", "status", "moves")
        for case, c in order_cases.PLAY.items():
            b, t = order_cases.play_starts(case)
            t0 = time.time()
            g0, g1 = play(ph, c, b, t, 0), play(ph, c, b, t, 1)
            t1 = time.time()
            ref = order_cases.play_reference(case)
            ok = all((g1[k] == g0[k]).all() and (g1[k] == ref[k]).all() for k in keys)
            bad += report("play: %s" % case, ok, "nodes %d -> %d  host %.1f s  checker %.1f s" % (
                g0["nodes"].sum(), g1["nodes"].sum(), t1 - t0, time.time() - t1))
        for case in play_host_check.play_cases.CASES:
            c = play_host_check.play_cases.CASES[case]
            b, t = play_host_check.play_cases.starts(case)
            g1 = play(ph, c, b, t, 1, tables=play_host_check.play_cases.TABLES)
            ref = play_host_check.play_cases.reference(case)
            bad += report("play: %s" % case, all((g1[k] == ref[k]).all() for k in keys))
    if "tree" in parts:  # the four task orders, both slabs
        for name, (depth, splits, tables) in tree_cases.CASES.items():
            b, t = tree_cases.inputs(name)
            for table in tables:
                rv, rm, _ = tree_cases.reference(name, table)
                for split in splits:
                    for npp in (32768, 64):
                        r0 = tree(th, b, t, tree_cases.TABLES[table], depth, split, npp, 0)
                        r1 = tree(th, b, t, tree_cases.TABLES[table], depth, split, npp, 1)
                        label = "tree: %s %s depth %d split %d slab %d" % (name, table, depth, split, npp)
                        wrong, nd = tree_host_check.compare(label, r1, rv, rm, allow_noroom=npp == 64)
                        same = all((r1[k] == r0[k]).all() for k in range(3))
                        bad += report(label, not wrong and same, "nodes %d -> %d" % (r0[3][0].sum(), nd[0].sum()))
    if "ratio" in parts:
        b, t = order_cases.versus(5)
        n0 = search(sh, b, t, 5, order_cases.TABLES["default"], 0)[3]
        n1 = search(sh, b, t, 5, order_cases.TABLES["default"], 1)[3]
        print("depth 5 x%d: nodes %d -> %d, ratio %.4f, max/mean %.1f -> %.1f" % (
            len(t), n0.sum(), n1.sum(), n1.sum() / n0.sum(), n0.max() / n0.mean(), n1.max() / n1.mean()), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
