#!/usr/bin/env python
"""Throughput of the exact endgame solver (ops.solve) by number of empties.

Positions are cut from seeded random rollouts (ops.rollout(record_moves=True)
+ ops.replay): from each game the first recorded position with exactly E empty
squares.  For E = 6, 8, 10, 12 (--empties) one JSON line: positions, ms per
launch (median of --reps after one warm-up), positions/s, nodes/s, mean and max
nodes per position and their ratio (the slowest position bounds a launch from
below), positions that hit the node limit, library_sha16.  The kernel does not
count its iterations, so there is no lane-busy share.  Every launch carries
--node-limit, which bounds its slowest lane; the tool stops raising E once a
launch has taken more than --stop-ms.

With tools/diag/solve_host built (see its header), each line also carries the
16-thread host figure on the first --host-positions positions of the same set.
OTH_SOLVE_BLOCKS / OTH_SOLVE_REFILL=1..64 in the environment select the grid
cap and the refill threshold (A/B runs); both are recorded in the line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, ops  # noqa: E402

HOST = os.path.join(ROOT, "tools", "diag", "solve_host")


def positions(games, seed, wanted):
    """dict E -> (boards (k,2) int64 device, turn (k,) uint8 device)"""
    g = ops.rollout(games, seed, record_moves=True, want_boards=False, want_diff=False)
    rp = ops.replay(g.moves, g.plies)
    b = ops.to_numpy_u64(rp.boards.reshape(games, -1, 2))
    occ = b[:, :, 0] | b[:, :, 1]
    cnt = np.zeros(occ.shape, np.int64)
    for k in range(64):
        cnt += ((occ >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    live = np.arange(occ.shape[1])[None, :] <= g.plies.cpu().numpy().astype(np.int64)[:, None]
    turn = rp.turn.reshape(games, -1).cpu().numpy()
    out = {}
    for e in wanted:
        hit = live & (cnt == 64 - e)
        has = hit.any(axis=1)
        first = hit.argmax(axis=1)
        rows = np.nonzero(has)[0]
        out[e] = (ops.from_numpy_u64(np.ascontiguousarray(b[rows, first[rows]]), "cuda"),
                  torch.from_numpy(np.ascontiguousarray(turn[rows, first[rows]])).cuda())
    return out


def host_line(boards, turn, e, limit, threads):
    if not os.path.exists(HOST) or boards.shape[0] == 0:
        return {}
    b = ops.to_numpy_u64(boards)
    t = turn.cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.txt"), os.path.join(d, "out.txt")
        with open(src, "w") as f:
            for (bl, wh), tt in zip(b, t):
                f.write("%x %x %d\n" % (int(bl), int(wh), int(tt)))
        r = subprocess.run([HOST, src, dst, str(e), str(limit), str(threads)], capture_output=True, text=True,
                           check=True)
        h = json.loads(r.stderr.strip().splitlines()[-1])
        got = np.loadtxt(dst, dtype=np.int64).reshape(-1, 4)
    return {"host_threads": threads, "host_positions": h["positions"], "host_positions_per_s": h["positions_per_s"],
            "host_nodes_per_s": h["nodes"] / h["seconds"] if h["seconds"] > 0 else 0.0, "_host_rows": got}


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--empties", type=int, nargs="+", default=[6, 8, 10, 12])
    p.add_argument("--games", type=int, default=32768)
    p.add_argument("--seed", type=int, default=0x501E)
    p.add_argument("--repeat", type=int, default=1,
                   help="launch the position set this many times over in one batch (more positions than lanes: "
                        "the refill path at the full grid)")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--node-limit", type=int, default=1 << 20)
    p.add_argument("--stop-ms", type=float, default=500.0)
    p.add_argument("--host-positions", type=int, default=2048)
    p.add_argument("--host-threads", type=int, default=16)
    a = p.parse_args()
    if a.node_limit <= 0:
        p.error("every launch carries a node limit")
    es = sorted(a.empties)
    pos = positions(a.games, a.seed, es)
    for e in es:
        boards, turn = pos[e]
        boards, turn = boards.repeat(a.repeat, 1), turn.repeat(a.repeat)
        n = boards.shape[0]
        r = ops.solve(boards, turn, max_empties=e, node_limit=a.node_limit, want_nodes=True)  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = ops.solve(boards, turn, max_empties=e, node_limit=a.node_limit, want_nodes=True)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        nodes = r.nodes.cpu().numpy().view(np.uint32).astype(np.int64)
        status = r.status.cpu().numpy()
        line = {"empties": e, "positions": n, "ms_per_launch": med, "ms_all": ms,
                "positions_per_s": n / (med * 1e-3), "nodes_per_s": int(nodes.sum()) / (med * 1e-3),
                "nodes_mean": float(nodes.mean()), "nodes_max": int(nodes.max()),
                "tail_ratio": float(nodes.max() / max(nodes.mean(), 1e-9)),
                "limit_hits": int((status == _lib.SOLVE_LIMIT).sum()), "node_limit": a.node_limit,
                "grid": _lib.load().oths_solve_grid(n), "solve_blocks": os.environ.get("OTH_SOLVE_BLOCKS"),
                "refill": os.environ.get("OTH_SOLVE_REFILL"), "library_sha16": _lib.library_sha16()}
        k = min(n, a.host_positions)
        h = host_line(boards[:k], turn[:k], e, a.node_limit, a.host_threads)
        rows = h.pop("_host_rows", None)
        if rows is not None:  # the same state machine: the two builds agree on everything
            same = ((rows[:, 0] == r.value[:k].cpu().numpy()) & (rows[:, 1] == r.best_move[:k].cpu().numpy())
                    & (rows[:, 2] == status[:k]) & (rows[:, 3] == nodes[:k]))
            h["host_agrees"] = bool(same.all())
        line.update(h)
        print(json.dumps(line), flush=True)
        if med > a.stop_ms:
            print(json.dumps({"stopped_after_empties": e, "reason": "launch took more than %.0f ms" % a.stop_ms}),
                  flush=True)
            break
    return 0


if __name__ == "__main__":
    sys.exit(main())
