#!/usr/bin/env python
"""Search by node budget against fixed depth: one JSON line per
measurement, printed and appended to --out (default profiles/budget_bench.jsonl).

  batch     ops.sample_midgame(--positions, 0x5EED): ops.search at each of
            --depths (time, total nodes, nodes per position max / mean) and
            ops.search_budget at a budget equal to that depth's mean nodes per
            position, taken from ops.search's own want_nodes output in this
            process (time, nodes of the completed iterations, the depth
            histogram, max / mean).  What a budget lane WORKS is its completed
            nodes plus the iteration that ran into the limit, below 2 B in all.
  play      ops.play from the same starts at depths (d, d) against budgets of
            that run's mean nodes per ply, cap --cap: time, nodes per game
            max / mean
  strength  runner.do_matches from the opening, --games games, colours drawn,
            --n-rand random moves a side: player A by budget B (cap --cap)
            against player B at fixed depth d (a budget no search reaches, cap
            d), B = the fixed-depth games' mean nodes per ply; A's wins,
            losses, draws

Times are wall ms around a device synchronise, the median of --reps.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, ops, runner  # noqa: E402


def timed(fn, reps):
    ms, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), ms


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--positions", type=int, default=32768)
    p.add_argument("--depths", type=int, nargs="+", default=[4, 5])
    p.add_argument("--cap", type=int, default=8)
    p.add_argument("--games", type=int, default=4096)
    p.add_argument("--n-rand", type=int, default=3)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--order", type=int, choices=[0, 1], default=0)
    p.add_argument("--node-limit", type=int, default=1 << 22)
    p.add_argument("--skip", nargs="*", default=[], choices=["batch", "play", "strength"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_bench.jsonl"))
    a = p.parse_args()
    n = a.positions
    sha = _lib.library_sha16()

    def emit(line):
        line.update({"order": a.order, "library_sha16": sha})
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    mid = ops.sample_midgame(n, seed=0x5EED)
    ops.search_budget(mid.boards[:64].contiguous(), mid.turn[:64].contiguous(), 100)  # loads the code object
    ops.play(64, 1, depth_a=2, budget=100)
    torch.cuda.synchronize()
    if "batch" not in a.skip:
        for d in a.depths:
            r, ms, all_ms = timed(lambda: ops.search(mid.boards, mid.turn, d, node_limit=a.node_limit, want_nodes=True,
                                                     order=a.order), a.reps)
            nd = u32(r.nodes)
            emit({"what": "batch_fixed", "positions": n, "depth": d, "ms": ms, "ms_all": all_ms,
                  "nodes": int(nd.sum()), "nodes_mean": float(nd.mean()), "nodes_max": int(nd.max()),
                  "tail_ratio": float(nd.max() / nd.mean()),
                  "limit_hits": int((r.status != _lib.SEARCH_SEARCHED).sum())})
            budget = max(1, int(round(nd.mean())))
            r, ms, all_ms = timed(lambda: ops.search_budget(mid.boards, mid.turn, budget, max_depth=a.cap,
                                                            want_nodes=True, order=a.order), a.reps)
            nb = u32(r.nodes)
            emit({"what": "batch_budget", "positions": n, "budget": budget, "budget_of_depth": d, "cap": a.cap, "ms": ms,
                  "ms_all": all_ms, "nodes": int(nb.sum()), "nodes_mean": float(nb.mean()), "nodes_max": int(nb.max()),
                  "tail_ratio": float(nb.max() / nb.mean()),
                  "depth_hist": np.bincount(r.depth.cpu().numpy(), minlength=9).tolist(),
                  "limit_hits": int((r.status == _lib.SEARCH_LIMIT).sum())})
    if "play" not in a.skip:
        for d in a.depths:
            kw = dict(start=mid.boards, start_turn=mid.turn, want_nodes=True, order=a.order, node_limit=a.node_limit)
            r, ms, all_ms = timed(lambda: ops.play(n, 0x5EED, depth_a=d, depth_b=d, **kw), a.reps)
            nd, pl = r.nodes.cpu().numpy(), r.plies.cpu().numpy().astype(np.int64)
            emit({"what": "play_fixed", "games": n, "depth": d, "ms": ms, "ms_all": all_ms, "nodes": int(nd.sum()),
                  "game_nodes_mean": float(nd.mean()), "game_nodes_max": int(nd.max()),
                  "tail_ratio": float(nd.max() / nd.mean()), "plies": int(pl.sum()),
                  "nodes_per_ply": float(nd.sum() / pl.sum()),
                  "limit_hits": int((r.status != _lib.SEARCH_SEARCHED).sum())})
            budget = max(1, int(round(nd.sum() / pl.sum())))
            r, ms, all_ms = timed(lambda: ops.play(n, 0x5EED, depth_a=a.cap, depth_b=a.cap, budget=budget, **kw), a.reps)
            nb, pl = r.nodes.cpu().numpy(), r.plies.cpu().numpy().astype(np.int64)
            emit({"what": "play_budget", "games": n, "budget": budget, "budget_of_depth": d, "cap": a.cap, "ms": ms,
                  "ms_all": all_ms, "nodes": int(nb.sum()), "game_nodes_mean": float(nb.mean()),
                  "game_nodes_max": int(nb.max()), "tail_ratio": float(nb.max() / nb.mean()), "plies": int(pl.sum()),
                  "nodes_per_ply": float(nb.sum() / pl.sum()),
                  "limit_hits": int((r.status != _lib.SEARCH_SEARCHED).sum())})
    if "strength" not in a.skip:
        conf = {"proc_n_rand_hands_for_a": a.n_rand, "proc_n_rand_hands_for_b": a.n_rand,
                "proc_randomize_black_white": 1}
        for d in a.depths:
            r = ops.play(a.games, 0xB0D6E7, depth_a=d, depth_b=d, n_rand_a=a.n_rand, n_rand_b=a.n_rand, swap_colours=True,
                         want_nodes=True, order=a.order)
            budget = max(1, int(round(float(r.nodes.sum()) / float(r.plies.long().sum()))))
            t0 = time.perf_counter()
            m = runner.do_matches(conf, None, n=a.games, seed=0xB0D6E7, policy="search", depth=(a.cap, d),
                                  budget=(budget, 2**32 - 1), record=False, order=a.order)
            torch.cuda.synchronize()
            won, lost, drawn = runner.wins_of_a(m)
            emit({"what": "strength", "games": a.games, "budget_a": budget, "cap_a": a.cap, "depth_b": d,
                  "n_rand": a.n_rand, "a_wins": won, "a_losses": lost, "draws": drawn,
                  "s": time.perf_counter() - t0})
    return 0


if __name__ == "__main__":
    sys.exit(main())
