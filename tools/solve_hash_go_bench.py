#!/usr/bin/env python
"""Wall time of successive `go`s of one endgame in the engine, with and without
the split solver's transposition table (--solve-hash-bits): the engine solves a
16-empties root of tests/solve_cases.ladder(16, 64) and then the position after
each of the next --plies - 1 plies (it plays both sides, so every `go` is one
solve one ply further down the same game).  One JSON line per (root, setting):
the ms of each `go` (host clock around Engine.handle, which ends in a copy to
the host), the moves, library_sha16.  The moves of the two settings must agree;
the tool says so on every line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
import solve_cases  # noqa: E402

from subproc_amd import _lib, engine  # noqa: E402


def play(eng, b, w, turn, plies):
    text = oracle.serialize_str(b, w, turn)
    eng.board.deserialize(text[:64], text[65], 0)
    ms, moves = [], []
    for _ in range(plies):
        if eng.board.is_game_over():
            break
        out = []
        t0 = time.perf_counter()
        eng.handle("go", out.append)
        ms.append((time.perf_counter() - t0) * 1e3)
        moves.append("".join(out).split()[-1])
    return ms, moves


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--roots", type=int, default=4)
    p.add_argument("--plies", type=int, default=5)
    p.add_argument("--task-empties", type=int, default=8)
    p.add_argument("--hash-bits", type=int, default=22)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    b, t = solve_cases.ladder(16, 64)
    sha = _lib.library_sha16()
    # one untimed game first: the library's and the allocator's first use
    play(engine.Engine(solve_empties=16, solve_task_empties=a.task_empties, order=1, solve_hash_bits=a.hash_bits),
         int(b[a.roots, 0]), int(b[a.roots, 1]), int(t[a.roots]), 2)
    for i in range(a.roots):
        runs = {}
        for bits in (None, a.hash_bits):
            eng = engine.Engine(solve_empties=16, solve_task_empties=a.task_empties, order=1, solve_hash_bits=bits)
            runs[bits] = play(eng, int(b[i, 0]), int(b[i, 1]), int(t[i]), a.plies)
        for bits, (ms, moves) in runs.items():
            print(json.dumps({"root": i, "hash_bits": bits, "task_empties": a.task_empties,
                              "hash_min_empties": _lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES if bits else None, "go_ms": ms,
                              "ms_sum": sum(ms), "moves": moves, "same_moves": moves == runs[None][1], "tag": a.tag,
                              "library_sha16": sha}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
