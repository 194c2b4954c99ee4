#!/usr/bin/env python
"""Write tests/golden/solve_deep/solve_deep.npz: the exact values and best moves of 38
roots at 13 to 16 empties, from tools/diag/solve_deep_ref.cpp (a plain
recursive alpha-beta, compiled here with g++ -O2 -fopenmp).  CPU only; a few
minutes on 16 threads.

Roots: solve_cases.ladder(13, 16), ladder(14, 8), ladder(15, 4), ladder(16, 4)
and every forced-pass root of solve_cases.pool() at 13..16 empties.

    python tools/diag/solve_deep_gen.py [OUT=tests/golden/solve_deep/solve_deep.npz] [threads=16]
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_programs as hp  # noqa: E402
import solve_cases  # noqa: E402
import solve_ref  # noqa: E402

LADDERS = ((13, 16), (14, 8), (15, 4), (16, 4))


def roots():
    bs, ts = [], []
    for e, k in LADDERS:
        b, t = solve_cases.ladder(e, k)
        assert len(t) == k
        bs.append(b)
        ts.append(t)
    for e in range(13, 17):
        p = solve_cases.pool()[e]
        bs.append(p["boards"][p["forced_pass"]])
        ts.append(p["turn"][p["forced_pass"]])
    return np.concatenate(bs), np.concatenate(ts)


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
    threads = argv[2] if len(argv) > 2 else "16"
    boards, turn = roots()
    with tempfile.TemporaryDirectory() as d:
        exe, inp, res = (os.path.join(d, x) for x in ("ref", "in", "out"))
        hp.build("solve_deep_ref", hp.PLAIN, exe)
        hp.write_positions(inp, boards, turn)
        hp.run([exe, inp, res, threads])
        rows = hp.read_rows(res)
    assert rows.shape == (len(turn), 4)
    emp = solve_ref.empties(boards)
    for e in range(13, 17):
        sel = emp == e
        print("%d empties: %d roots, nodes ascending %s, ordered %s" % (
            e, sel.sum(), rows[sel, 2].tolist(), rows[sel, 3].tolist()))
    np.savez_compressed(out, boards=boards, turn=turn.astype(np.uint8), empties=emp.astype(np.uint8),
                        value=rows[:, 0].astype(np.int8), best_move=rows[:, 1].astype(np.uint8))
    print("wrote %s: %d roots, %d bytes" % (out, len(turn), os.path.getsize(out)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
