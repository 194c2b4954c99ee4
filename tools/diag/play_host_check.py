#!/usr/bin/env python
"""Run the host build of the self-play driver (tools/diag/play_host.cpp,
usually built with -fsanitize=address,undefined) on every case of
tests/play_cases.py and compare its games with the checker's (tests/play_ref.py)
byte for byte.  CPU only; meant to be run before the kernel's first GPU run
after a change to play_core.hpp.

    python tools/diag/play_host_check.py [BINARY=tools/diag/play_host_asan] [case ...]
"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_programs as hp  # noqa: E402
import play_cases  # noqa: E402


def write_args(path, n, seed, game_id0, depth, exact, n_rand, swap, node_limit, wa, wb, boards=None, turn=None):
    """The ARGS file of play_host.cpp (tools/play_bench.py writes it through here too)."""
    hp.write_game_args(path, n, seed, depth, exact, n_rand, swap, node_limit, wa, wb, boards, turn, game_id0=game_id0)


read_out = hp.read_games  # dict of arrays from play_host.cpp's OUT file


def play(binary, c, boards, turn, tables, threads=16, order=0):
    """The games of case `c` from the given starts, as a dict of arrays."""
    with tempfile.TemporaryDirectory() as d:
        args, out = os.path.join(d, "args"), os.path.join(d, "out")
        write_args(args, c["n"], c["seed"], c["game_id0"], c["depth"], c["exact"], c["n_rand"], c["swap"], 1 << 22,
                   tables[c["tables"][0]], tables[c["tables"][1]], boards, turn)
        hp.run([binary, args, out, threads, order])
        return read_out(out)


def run_case(binary, case, threads=16):
    return play(binary, play_cases.CASES[case], *play_cases.starts(case), play_cases.TABLES, threads)


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
