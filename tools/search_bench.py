#!/usr/bin/env python
"""Throughput of the depth-limited search (ops.search) by depth.

Positions: ops.sample_midgame(32768, seed=0x5EED) (11..50 empties), the default
eval table.  One launch per depth from 1 up (--depths), one JSON line each:
positions, ms per launch (median of --reps after one warm-up), positions/s,
nodes/s, mean and max nodes per position and their ratio (the slowest position
bounds a launch from below), positions that hit the node limit, library_sha16.
Every launch carries --node-limit, which bounds its slowest lane; the tool
stops after the first launch that takes more than --stop-ms.

With tools/diag/search_host built (see its header), each line also carries the
16-thread host figure on the first positions of the same set: --host-positions
of them, fewer once their node count (known from the GPU run) would pass
--host-nodes.  OTH_SEARCH_BLOCKS in the environment caps the grid (recorded).
--order 0 1 runs every depth at each order in turn, in one process (order 1:
include/othello_order.h; its nodes count the scoring placements too).

--engine times one `go` of the Edax-protocol engine per depth instead (policy
search at depths 1..6 beside policy eval), on --engine-positions midgame
positions: the median wall time of Engine.choose().
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
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, codec, ops, params  # noqa: E402

HOST = os.path.join(ROOT, "tools", "diag", "search_host")


def host_line(boards, turn, depth, limit, threads, order=0):
    if not os.path.exists(HOST) or boards.shape[0] == 0:
        return {}
    b = ops.to_numpy_u64(boards)
    t = turn.cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        src, dst, wts = os.path.join(d, "in.txt"), os.path.join(d, "out.txt"), os.path.join(d, "w.txt")
        with open(src, "w") as f:
            for (bl, wh), tt in zip(b, t):
                f.write("%x %x %d\n" % (int(bl), int(wh), int(tt)))
        with open(wts, "w") as f:
            f.write(" ".join(str(int(x)) for x in params.as_weights(params.DEFAULT_WEIGHTS).reshape(-1)))
        r = subprocess.run([HOST, src, dst, wts, str(depth), str(limit), str(threads), str(order)], capture_output=True,
                           text=True, check=True)
        h = json.loads(r.stderr.strip().splitlines()[-1])
        got = np.loadtxt(dst, dtype=np.int64).reshape(-1, 4)
    return {"host_threads": threads, "host_positions": h["positions"], "host_positions_per_s": h["positions_per_s"],
            "host_nodes_per_s": h["nodes"] / h["seconds"] if h["seconds"] > 0 else 0.0, "_host_rows": got}


def engine_times(a):
    from subproc_amd import engine

    pos = ops.sample_midgame(a.engine_positions, seed=a.seed)
    b = ops.to_numpy_u64(pos.boards)
    t = pos.turn.cpu().numpy()
    for policy, depth, order in [("eval", 1, 0)] + [("search", d, o) for d in a.depths if d <= 6 for o in a.order]:
        eng = engine.Engine(policy=policy, depth=depth, order=order)
        us = []
        for i in range(len(t)):
            text = codec.serialize_str(int(b[i, 0]), int(b[i, 1]), int(t[i]), True)
            eng.board.deserialize(text[:64], text[65], 0)
            eng.board.puttables(eng.board.turn)  # (the board's own analysis is not the policy's time)
            if i == 0:
                eng.choose()  # warm-up
            t0 = time.perf_counter()
            eng.choose()
            us.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({"engine_policy": policy, "depth": depth if policy == "search" else None, "order": order,
                          "positions": len(t), "us_per_go_median": statistics.median(us), "us_per_go_max": max(us),
                          "library_sha16": _lib.library_sha16()}), flush=True)
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--depths", type=int, nargs="+", default=list(range(1, _lib.SEARCH_MAX_DEPTH + 1)))
    p.add_argument("--positions", type=int, default=32768)
    p.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--node-limit", type=int, default=1 << 20)
    p.add_argument("--stop-ms", type=float, default=500.0)
    p.add_argument("--host-positions", type=int, default=2048)
    p.add_argument("--host-nodes", type=float, default=2e8, help="host node budget per depth")
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--order", type=int, nargs="+", choices=[0, 1], default=[0], help="move ordering(s) to run")
    p.add_argument("--engine", action="store_true", help="time the engine's `go` per depth instead")
    p.add_argument("--engine-positions", type=int, default=64)
    a = p.parse_args()
    if a.node_limit <= 0:
        p.error("every launch carries a node limit")
    if a.engine:
        return engine_times(a)
    pos = ops.sample_midgame(a.positions, seed=a.seed)
    boards, turn = pos.boards, pos.turn
    n = boards.shape[0]
    stopped = set()
    for depth, order in [(d, o) for d in sorted(a.depths) for o in a.order]:
        if order in stopped:
            continue
        r = ops.search(boards, turn, depth, node_limit=a.node_limit, want_nodes=True, order=order)  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = ops.search(boards, turn, depth, node_limit=a.node_limit, want_nodes=True, order=order)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        nodes = r.nodes.cpu().numpy().view(np.uint32).astype(np.int64)
        status = r.status.cpu().numpy()
        line = {"depth": depth, "order": order, "positions": n, "ms_per_launch": med, "ms_all": ms,
                "positions_per_s": n / (med * 1e-3), "nodes_per_s": int(nodes.sum()) / (med * 1e-3),
                "nodes_mean": float(nodes.mean()), "nodes_max": int(nodes.max()),
                "tail_ratio": float(nodes.max() / max(nodes.mean(), 1e-9)),
                "limit_hits": int((status == _lib.SEARCH_LIMIT).sum()), "node_limit": a.node_limit,
                "grid": _lib.load().otho_search_ordered_grid(n, order), "search_blocks": os.environ.get("OTH_SEARCH_BLOCKS"),
                "library_sha16": _lib.library_sha16()}
        k = min(n, a.host_positions)
        while k > 16 and nodes[:k].sum() > a.host_nodes:
            k //= 2
        h = host_line(boards[:k], turn[:k], depth, a.node_limit, a.host_threads, order)
        rows = h.pop("_host_rows", None)
        if rows is not None:  # the same state machine: the two builds agree on everything
            same = ((rows[:, 0] == r.value[:k].cpu().numpy()) & (rows[:, 1] == r.best_move[:k].cpu().numpy())
                    & (rows[:, 2] == status[:k]) & (rows[:, 3] == nodes[:k]))
            h["host_agrees"] = bool(same.all())
        line.update(h)
        print(json.dumps(line), flush=True)
        if med > a.stop_ms:
            print(json.dumps({"stopped_after_depth": depth, "order": order,
                              "reason": "launch took more than %.0f ms" % a.stop_ms}), flush=True)
            stopped.add(order)
            if len(stopped) == len(set(a.order)):
                break
    return 0


if __name__ == "__main__":
    sys.exit(main())
