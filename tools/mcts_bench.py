#!/usr/bin/env python
"""What the Monte Carlo tree search costs (ops.mcts).  One JSON
line per measurement, each with the library_sha16: wall ms around a
synchronise, the median of --reps calls after one warm-up and the worst beside.

  rate     ops.mcts on the first n of ops.sample_midgame(.., 0x5EED) for n in
           --positions and T in --iterations: playouts/s, ms per call, us per
           iteration; beside it ops.rollout playing as many games (at most
           --rollout-cap in one launch) from the same roots in the same
           process: games/s, env-steps/s from its histogram, and the fraction
           of that rate the search reaches
  replay   tools/diag/mcts_host.cpp on the first --host-positions roots at
           each T: the same trees, so the same leaves, replayed with the plies
           counted: env-steps per playout and the share of lane-steps that 64
           games in lockstep with no hand-over spend playing (the rest waits
           for the iteration's longest game); its wall time at --host-threads
           threads is the host baseline
"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, ops  # noqa: E402

SEED = 0xC0FFEE


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


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["rate", "replay"])
    p.add_argument("--positions", type=int, nargs="+", default=[1, 64, 4096, 32768])
    p.add_argument("--iterations", type=int, nargs="+", default=[64, 256, 1024])
    p.add_argument("--explore", type=float, default=0.5)
    p.add_argument("--rollout-cap", type=int, default=1 << 24)
    p.add_argument("--host-positions", type=int, default=64)
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    base = {"library_sha16": _lib.library_sha16(), "reps": a.reps, "tag": a.tag, "explore": a.explore}

    def emit(**kw):
        print(json.dumps({**kw, **base}), flush=True)

    pos = ops.sample_midgame(max(a.positions + [a.host_positions]), seed=0x5EED)
    if "rate" in a.sections:
        for n in a.positions:
            b, t = pos.boards[:n].contiguous(), pos.turn[:n].contiguous()
            for T in a.iterations:
                ms, mx, r = timed(lambda: ops.mcts(b, t, T, explore=a.explore, seed=SEED, want_nodes=True), a.reps)
                assert bool((r.status == _lib.MCTS_SEARCHED).all())
                playouts = n * T * 64
                games = min(playouts, a.rollout_cap)
                idx = torch.arange(games, device=b.device) % n
                sb, st = b[idx].contiguous(), t[idx].contiguous()
                rms, rmx, g = timed(lambda: ops.rollout(games, SEED, start=sb, start_turn=st, want_boards=False,
                                                        want_diff=False, want_plies=False), a.reps)
                steps = int(g.hist[132])
                emit(section="rate", positions=n, iterations=T, grid=_lib.load().othu_mcts_grid(n), ms=ms, ms_max=mx,
                     playouts=playouts, playouts_per_s=playouts / ms * 1e3, us_per_iteration=ms * 1e3 / T,
                     nodes_mean=float(r.nodes.float().mean()), rollout_games=games, rollout_ms=rms,
                     rollout_ms_max=rmx, rollout_games_per_s=games / rms * 1e3,
                     rollout_env_steps_per_s=steps / rms * 1e3, rollout_plies_per_game=steps / games,
                     fraction_of_rollout=(playouts / ms) / (games / rms))
    if "replay" in a.sections:
        k = a.host_positions
        b, t = pos.boards[:k].contiguous(), pos.turn[:k].contiguous()
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "mcts_host")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-o", exe,
                                   os.path.join(ROOT, "tools", "diag", "mcts_host.cpp")])
            inp, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            for T in a.iterations:
                with open(inp, "w") as f:
                    for (bl, wh), tn in zip(ops.to_numpy_u64(b).tolist(), t.cpu().tolist()):
                        f.write("%x %x %d\n" % (bl, wh, tn))
                    for x in ops.mcts_log_table(T):
                        f.write("L %x\n" % bits(x))
                M = min(1 + 16 * T, _lib.MCTS_MAX_NODES)
                t0 = time.perf_counter()
                subprocess.check_call([exe, inp, out, str(T), "%x" % bits(a.explore), str(SEED), "0", str(M),
                                       str(a.host_threads)])
                hms = (time.perf_counter() - t0) * 1e3
                lines = open(out).read().splitlines()
                rows = np.array([[int(x) for x in ln.split()] for ln in lines[:-1]], np.int64)
                r = ops.mcts(b, t, T, explore=a.explore, seed=SEED, want_nodes=True)
                torch.cuda.synchronize()
                assert (rows[:, 5:69] == r.visits.cpu().numpy()).all() and (rows[:, 2] == r.nodes.cpu().numpy()).all()
                meta = lines[-1].split()
                plies, wave_plies = int(meta[1]), int(meta[3])
                playouts = k * T * 64
                emit(section="replay", positions=k, iterations=T, threads=a.host_threads, host_ms=hms,
                     host_playouts_per_s=playouts / hms * 1e3, playouts=playouts, env_steps=plies,
                     plies_per_playout=plies / playouts, lockstep_lane_share=plies / (64 * wave_plies))
    return 0


if __name__ == "__main__":
    sys.exit(main())
