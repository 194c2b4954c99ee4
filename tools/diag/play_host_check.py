#!/usr/bin/env python
"""Run the host build of the self-play driver (tools/diag/play_host.cpp,
usually built with -fsanitize=address,undefined) on every case of
tests/play_cases.py and compare its games with the checker's (tests/play_ref.py)
byte for byte.  CPU only; meant to be run before the kernel's first GPU run
after a change to play_core.hpp.

    python tools/diag/play_host_check.py [BINARY=tools/diag/play_host_asan] [case ...]
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import play_cases  # noqa: E402


def write_args(path, n, seed, game_id0, depth, exact, n_rand, swap, node_limit, wa, wb, boards=None, turn=None):
    """The ARGS file of play_host.cpp."""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d %d %d\n" % (n, seed, game_id0, depth[0], depth[1], exact, n_rand[0],
                                                     n_rand[1], int(swap), node_limit, int(boards is not None)))
        for w in (wa, wb):
            f.write(" ".join(str(int(x)) for x in np.asarray(w).reshape(-1)) + "\n")
        if boards is not None:
            for (b, w), t in zip(np.asarray(boards, np.uint64).tolist(), np.asarray(turn).tolist()):
                f.write("%x %x %d\n" % (b, w, t))


def read_out(path):
    """dict of arrays from play_host.cpp's OUT file."""
    rows = [ln.split() for ln in open(path)]
    return dict(a_black=np.array([int(r[0]) for r in rows], np.uint8),
                final_boards=np.array([[int(r[1], 16), int(r[2], 16)] for r in rows], np.uint64).reshape(-1, 2),
                diff=np.array([int(r[3]) for r in rows], np.int8),
                plies=np.array([int(r[4]) for r in rows], np.uint8),
                status=np.array([int(r[5]) for r in rows], np.uint8),
                nodes=np.array([int(r[6]) for r in rows], np.uint64),
                moves=np.array([list(bytes.fromhex(r[7])) for r in rows], np.uint8).reshape(-1, 128))


def run_case(binary, case, threads=16):
    c = play_cases.CASES[case]
    b, t = play_cases.starts(case)
    with tempfile.TemporaryDirectory() as d:
        args, out = os.path.join(d, "args"), os.path.join(d, "out")
        write_args(args, c["n"], c["seed"], c["game_id0"], c["depth"], c["exact"], c["n_rand"], c["swap"], 1 << 22,
                   play_cases.TABLES[c["tables"][0]], play_cases.TABLES[c["tables"][1]], b, t)
        subprocess.run([binary, args, out, str(threads)], check=True, stderr=subprocess.DEVNULL)
        return read_out(out)


def main(argv):
    binary = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tools", "diag", "play_host_asan")
    bad = 0
    for case in argv[2:] or play_cases.CASES:
        t0 = time.time()
        got = run_case(binary, case)
        t1 = time.time()
        ref = play_cases.reference(case)
        keys = ("a_black", "final_boards", "diff", "plies", "status", "moves")
        wrong = [k for k in keys if not (got[k] == ref[k]).all()]
        bad += bool(wrong)
        print("%-20s %3d games  host %.1f s  checker %.1f s  max game nodes %d  %s" % (
            case, len(got["plies"]), t1 - t0, time.time() - t1, int(got["nodes"].max()),
            "DIFFERS in " + ", ".join(wrong) if wrong else "equal"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
