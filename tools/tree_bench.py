#!/usr/bin/env python
"""Latency of the split search (ops.search(split=S)) against the one-lane
search (split=0) in the same process, by depth and batch size.

Positions: the first --positions of ops.sample_midgame(64, seed=0x5EED), the
positions behind DESIGN.md §13's `go` timings, cycled up to --batch per launch;
the default eval table.  For each depth of --depths and each split of --splits
that is valid at that depth (0 = othm_search, up to depth 8), the positions are
searched --batch at a time; one JSON line per (depth, split, batch): median and
worst wall time of a launch (host clock around the call and a synchronise,
after one warm-up launch per configuration), the nodes of all launches, their
ratio to split 0's at that depth (the search overhead of the wider windows;
nodes under a split depend on timing), the statuses, library_sha16.  Every
launch carries --node-limit (per position for split 0, per task otherwise); a
configuration stops early once it has used --budget-s seconds, and says how
many launches it timed.

--lib PATH loads another build of the library (the "nothing shared" variant of
tools/diag/tree_snapshot.patch) so that both are measured on the same inputs.
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

from subproc_amd import _lib  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--depths", type=int, nargs="+", default=[4, 5, 6, 7, 8, 9, 10])
    p.add_argument("--splits", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    p.add_argument("--positions", type=int, default=64)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    p.add_argument("--node-limit", type=int, default=1 << 24)
    p.add_argument("--nodes-per-position", type=int, default=_lib.TREE_DEFAULT_NODES)
    p.add_argument("--budget-s", type=float, default=20.0)
    p.add_argument("--lib", default=None, help="another build of the library")
    p.add_argument("--order", type=int, nargs="+", choices=[0, 1], default=[0], help="move ordering(s), each a line")
    p.add_argument("--tag", default="shared", help="recorded on every line (shared / snapshot)")
    a = p.parse_args()
    if a.node_limit <= 0:
        p.error("every launch carries a node limit")
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from subproc_amd import ops

    pos = ops.sample_midgame(64, seed=a.seed)
    k = min(a.positions, 64)
    pick = torch.arange(max(a.batch, k), device=pos.boards.device) % k
    boards, turn = pos.boards[pick].contiguous(), pos.turn[pick].contiguous()
    launches = [(i, i + a.batch) for i in range(0, boards.shape[0] - a.batch + 1, a.batch)]
    sha = _lib.library_sha16(_lib.LIB_PATH)
    for depth in sorted(a.depths):
        base_nodes = None
        for split, order in [(s, o) for s in sorted(a.splits) for o in a.order]:
            if split == 0 and depth > _lib.SEARCH_MAX_DEPTH:
                continue
            if split and not (split < depth <= split + _lib.SEARCH_MAX_DEPTH):
                continue
            kw = dict(node_limit=a.node_limit, want_nodes=True, split=split, order=order)
            if split:
                kw["nodes_per_position"] = a.nodes_per_position
            ops.search(boards[:a.batch], turn[:a.batch], depth, **kw)  # warm-up
            torch.cuda.synchronize()
            ms, nodes, status = [], 0, {}
            t_start = time.perf_counter()
            for lo, hi in launches:
                t0 = time.perf_counter()
                r = ops.search(boards[lo:hi], turn[lo:hi], depth, **kw)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                nodes += int(r.nodes.cpu().numpy().view(np.uint32).astype(np.int64).sum())
                for s, c in zip(*np.unique(r.status.cpu().numpy(), return_counts=True)):
                    status[int(s)] = status.get(int(s), 0) + int(c)
                if time.perf_counter() - t_start > a.budget_s:
                    break
            if split == 0 and order == 0:
                base_nodes = (nodes, len(ms))
            line = {"depth": depth, "split": split, "order": order, "batch": a.batch, "launches": len(ms), "of": len(launches),
                    "ms_median": statistics.median(ms), "ms_max": max(ms), "ms_sum": sum(ms), "nodes": nodes,
                    "nodes_vs_split0": (nodes / base_nodes[0] if base_nodes and base_nodes[1] == len(ms)
                                        and base_nodes[0] else None),
                    "status_counts": status, "node_limit": a.node_limit,
                    "nodes_per_position": a.nodes_per_position if split else None,
                    "search_blocks": os.environ.get("OTH_SEARCH_BLOCKS"), "variant": a.tag, "library_sha16": sha}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
