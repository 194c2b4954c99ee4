#!/usr/bin/env python
"""What perft costs (ops.perft): the node rate of the bare tree
walker.  One JSON line per measurement, each with the library_sha16: wall ms
around a synchronise, the median of --reps launches after one warm-up and the
worst beside, leaves/s and visits/s (visits = the positions the count kernel
generated moves for, ops.perft's nodes).

  opening  the opening at --depths with --splits: one position over the device
  levels   the same calls at depth = split: the expand levels alone (every task
           is final, the count kernel adds a 1 per task)
  batch    ops.sample_midgame(--positions, 0x5EED) at --batch-depths, split 0
  host     tools/diag/perft_host.cpp at --host-threads threads on the opening
           at --host-depths (split 5) and on the first --host-positions of the
           batch: the host baseline, built into a temporary directory
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, ops  # noqa: E402

OPENING = (4, 12, 56, 244, 1396, 8200, 55092, 390216, 3005288, 24571284, 212258800, 1939886636)  # tests/perft_ref.py


def timed(fn, reps):
    """(median ms, worst ms, the last result) of fn() after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), max(ms), r


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["opening", "levels", "batch", "host"])
    p.add_argument("--depths", type=int, nargs="+", default=[8, 9, 10, 11, 12, 13])
    p.add_argument("--splits", type=int, nargs="+", default=[5, 6, 7, 8])
    p.add_argument("--max-tasks", type=int, default=1 << 22)
    p.add_argument("--batch-depths", type=int, nargs="+", default=[3, 4, 5])
    p.add_argument("--positions", type=int, default=32768)
    p.add_argument("--host-depths", type=int, nargs="+", default=[10, 11])
    p.add_argument("--host-positions", type=int, default=4096)
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    base = {"library_sha16": _lib.library_sha16(), "reps": a.reps, "tag": a.tag}

    def emit(**kw):
        print(json.dumps({**kw, **base}), flush=True)

    ob, ot, _ = ops.reset(1)
    if "opening" in a.sections:
        for d in a.depths:
            for s in a.splits:
                ms, mx, r = timed(lambda: ops.perft(ob, ot, d, split=s, max_tasks=a.max_tasks, want_nodes=True), a.reps)
                leaves, visits = int(r.leaves[0]), int(r.nodes[0])
                assert int(r.status[0]) == _lib.PERFT_COUNTED and (d > len(OPENING) or leaves == OPENING[d - 1]), (d, s)
                emit(section="opening", depth=d, split=s, max_tasks=a.max_tasks, ms=ms, ms_max=mx, leaves=leaves,
                     visits=visits, leaves_per_s=leaves / ms * 1e3, visits_per_s=visits / ms * 1e3)
    if "levels" in a.sections:
        for s in a.splits:
            ms, mx, r = timed(lambda: ops.perft(ob, ot, s, split=s, max_tasks=a.max_tasks, want_nodes=True), a.reps)
            emit(section="levels", split=s, max_tasks=a.max_tasks, ms=ms, ms_max=mx, tasks=int(r.leaves[0]),
                 visits=int(r.nodes[0]))
    pos = None
    if "batch" in a.sections or "host" in a.sections:
        pos = ops.sample_midgame(a.positions, 0x5EED)
    if "batch" in a.sections:
        for d in a.batch_depths:
            ms, mx, r = timed(lambda: ops.perft(pos.boards, pos.turn, d, split=0, want_nodes=True), a.reps)
            leaves, visits = int(r.leaves.sum()), int(r.nodes.sum())
            assert bool((r.status == _lib.PERFT_COUNTED).all())
            emit(section="batch", depth=d, positions=a.positions, ms=ms, ms_max=mx, leaves=leaves, visits=visits,
                 leaves_per_s=leaves / ms * 1e3, visits_per_s=visits / ms * 1e3,
                 position_visits_max=int(r.nodes.max()), position_visits_mean=float(r.nodes.float().mean()))
    if "host" in a.sections:
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "perft_host")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-o", exe,
                                   os.path.join(ROOT, "tools", "diag", "perft_host.cpp")])

            def host(boards, turn, depth, split, max_tasks):
                inp, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
                with open(inp, "w") as f:
                    for (b, w), t in zip(boards.tolist(), turn.tolist()):
                        f.write("%x %x %d\n" % (b, w, t))
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    subprocess.check_call([exe, inp, out, str(depth), str(split), str(max_tasks), "0", "0",
                                           str(a.host_threads)])
                    ms.append((time.perf_counter() - t0) * 1e3)
                rows = np.array([[int(x) for x in ln.split()[:3]] for ln in open(out).read().splitlines()[:-1]], np.int64)
                return statistics.median(ms), max(ms), int(rows[:, 0].sum()), int(rows[:, 2].sum())

            b1, t1 = ops.to_numpy_u64(ob), ot.cpu().numpy()
            for d in a.host_depths:
                ms, mx, leaves, visits = host(b1, t1, d, 5, 1 << 16)
                assert d > len(OPENING) or leaves == OPENING[d - 1]
                emit(section="host", what="opening", depth=d, split=5, threads=a.host_threads, ms=ms, ms_max=mx,
                     leaves=leaves, visits=visits, leaves_per_s=leaves / ms * 1e3, visits_per_s=visits / ms * 1e3)
            k = min(a.host_positions, a.positions)
            bk, tk = ops.to_numpy_u64(pos.boards[:k]), pos.turn[:k].cpu().numpy()
            for d in a.batch_depths:
                ms, mx, leaves, visits = host(bk, tk, d, 0, k)
                emit(section="host", what="batch", depth=d, positions=k, threads=a.host_threads, ms=ms, ms_max=mx,
                     leaves=leaves, visits=visits, leaves_per_s=leaves / ms * 1e3, visits_per_s=visits / ms * 1e3)
    return 0


if __name__ == "__main__":
    sys.exit(main())
