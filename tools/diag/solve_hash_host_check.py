#!/usr/bin/env python
"""Build tools/diag/solve_hash_host.cpp twice, with -fsanitize=address,undefined
and with -fsanitize=thread, and run each ONCE as a stand-alone child process
(nothing is loaded into Python under a sanitizer): mode a (one thread, three
task orders on one table, then without it) under the first, mode b (8 threads
on a 16-entry table) under the second, against tests/solve_ref.py at 3..8
empties and the deep fixture's 13-empties roots.  Any sanitizer report fails
the run (the child's exit status, and its stderr is shown).  CPU only; meant
to be run before the hashed kernels' first GPU run after a change to
solve_hash_core.hpp.

    python tools/diag/solve_hash_host_check.py

ThreadSanitizer does not model a stand-alone fence: mode b carries the
orderings on the accesses, so this run checks the protocol, not the device's
spelling of it with fences (DESIGN.md §19 argues that one).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_programs as hp  # noqa: E402
import solve_cases  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
BUILDS = {"asan": hp.SANITIZED, "tsan": hp.THREAD_SANITIZED}


def run(binary, mode, boards, turn, rv, rm, max_empties, task_empties, npp, order, bits, label):
    with tempfile.TemporaryDirectory() as d:
        inp, out = os.path.join(d, "in"), os.path.join(d, "out")
        hp.write_positions(inp, boards, turn)
        try:
            hp.run([binary, mode, inp, out, max_empties, task_empties, npp, order, bits, 1, 3, 1, 8])
        except hp.ProgramFailed as e:  # a non-zero exit status or a sanitizer's report
            print(e.result.stderr)
            print("%-60s FAILED (exit %d)" % (label, e.result.returncode))
            return 1
        rows = hp.read_rows(out, (len(turn), -1, 4))
    ok = (rows[:, :, 2] == 1).all() and (rows[:, :, 0] == rv[:, None]).all() and (rows[:, :, 1] == rm[:, None]).all()
    print("%-60s %4d roots  nodes %s  %s" % (label, len(turn), "/".join(str(int(x)) for x in rows[:, :, 3].sum(0)),
                                           "equal" if ok else "DIFFERS"), flush=True)
    return 0 if ok else 1


def main():
    cases = solve_cases.cases()

    def pool(lo, hi):
        return tuple(np.concatenate([cases[e][k] for e in range(lo, hi + 1)])
                     for k in ("boards", "turn", "value", "best_move"))

    fx = np.load(FIXTURE)
    sel = fx["empties"] == 13
    deep = (fx["boards"][sel], fx["turn"][sel], fx["value"][sel].astype(np.int64), fx["best_move"][sel])
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        exe = {}
        for name, flags in BUILDS.items():
            exe[name] = hp.build("solve_hash_host", flags, os.path.join(d, "solve_hash_host_" + name))
        for order in (0, 1):
            bad += run(exe["asan"], "a", *pool(3, 8), 16, 3, 64, order, 4, "asan, a, 3..8 empties, slab 64, 16 entries, order %d" % order)
            bad += run(exe["asan"], "a", *pool(6, 8), 16, 3, 65536, order, 16, "asan, a, 6..8 empties, 2^16 entries, order %d" % order)
            bad += run(exe["tsan"], "b", *pool(6, 8), 16, 3, 65536, order, 4, "tsan, b, 6..8 empties, 16 entries, order %d" % order)
        bad += run(exe["tsan"], "b", *deep, 13, 10, 512, 1, 4, "tsan, b, fixture 13 empties, slab 512, 16 entries, order 1")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
