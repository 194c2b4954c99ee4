#!/usr/bin/env python
"""Latency of the split solver (ops.solve(task_empties=T, order=o)) against the
one-lane solver (ops.solve) and the split search at full depth
(ops.search(depth=E, split=4, order=1)) in the same process, by empties.

Positions: the first --positions of tests/solve_cases.ladder(E, 64) for each E
of --empties, --batch per launch.  One JSON line per (E, method): median and
worst wall time of a launch (host clock around the call and a synchronise,
after one warm-up launch per method on the first position), the nodes of all
launches (under a split they depend on timing), the statuses, library_sha16.
Methods: "lane" (E <= 12), "search" (E <= 12), "T<t>o<o>" for every t of
--task-empties and o of --order, and with --hash-bits "T<t>o<o>h<bits>g<gate>f"
(ops.solve(..., table=) on a table emptied before every launch, outside the
timed region) and "...k" (one table kept across the launches of the line) for
every gate of --hash-min-empties.  Every launch carries --node-limit (per
position for "lane", per task otherwise); a method stops early once it has used
--budget-s seconds and says how many launches it timed.  Nothing raises a
limit silently: a position that ends as LIMIT or NOROOM is counted in
status_counts and named in "unsolved".

--window A,B / --wld / --around put every solve under a root window
(ops.solve(window=...)): a fixed one, (-1, 1), or (V - 1, V + 1)
per position with V from a full-window solve made before anything is timed.
The line says which ("window"); the "search" method has no window and is left
out.  --ladder K takes the first K ladder positions instead of 64 and --tile N
repeats the set up to N positions (the one-lane solver's 32,768-position
batches).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib  # noqa: E402


def hashed_method(ops, a, e, te, o, bits, gate, kept):
    """ops.solve with a table of its own; the caller clears it between launches unless it is kept."""
    table = ops.SolveTable(bits, "cuda")

    def fn(bb, tt, **kw):
        return ops.solve(bb, tt, max_empties=e, node_limit=a.node_limit, want_nodes=True, task_empties=te, order=o,
                         nodes_per_position=a.nodes_per_position, table=table, hash_min_empties=gate, **kw)

    fn.table, fn.kept = table, kept
    return fn


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--empties", type=int, nargs="+", default=[10, 12, 14, 16])
    p.add_argument("--task-empties", type=int, nargs="+", default=[8, 10, 12])
    p.add_argument("--order", type=int, nargs="+", choices=[0, 1], default=[0, 1])
    p.add_argument("--methods", nargs="+", default=["lane", "search", "split"])
    p.add_argument("--positions", type=int, default=64)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--node-limit", type=int, default=1 << 26)
    p.add_argument("--nodes-per-position", type=int, default=_lib.SOLVE_TREE_DEFAULT_NODES)
    p.add_argument("--budget-s", type=float, default=20.0)
    p.add_argument("--tag", default="", help="recorded on every line")
    p.add_argument("--hash-bits", type=int, nargs="*", default=[], help="also time the split solver with a table of 2**B entries")
    p.add_argument("--hash-min-empties", type=int, nargs="+", default=[_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES])
    p.add_argument("--no-plain", action="store_true", help="skip the split lines without a table")
    p.add_argument("--lib", default=None, help="another build of the library (the parent commit's), for the methods it has")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--window", default=None, metavar="A,B", help="solve under the root window (A, B)")
    g.add_argument("--wld", action="store_true", help="solve for win / draw / loss: the window (-1, 1)")
    g.add_argument("--around", action="store_true", help="solve under (V - 1, V + 1), V from a full-window solve")
    p.add_argument("--ladder", type=int, default=64, help="ladder positions per empties to draw --positions from")
    p.add_argument("--tile", type=int, default=0, help="repeat the position set up to this many positions")
    a = p.parse_args()
    windowed = "wld" if a.wld else "around" if a.around else a.window
    if a.node_limit <= 0:
        p.error("every launch carries a node limit")
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        import ctypes

        other = ctypes.CDLL(_lib.LIB_PATH)
        # (a build from before a set has nothing to bind it to)
        if not hasattr(other, "othh_solve_hashed"):
            _lib.SOLVE_HASH_SIGNATURES = {}
        if not hasattr(other, "othw_solve"):
            _lib.SOLVE_WINDOW_SIGNATURES = {}
        if (a.hash_bits and not _lib.SOLVE_HASH_SIGNATURES) or (windowed and not _lib.SOLVE_WINDOW_SIGNATURES):
            p.error("--lib measures the methods the other build has: it has no table / no window")
    import solve_cases
    from subproc_amd import ops

    sha = _lib.library_sha16(_lib.LIB_PATH)
    for e in sorted(a.empties):
        b, t = solve_cases.ladder(e, a.ladder)
        k = min(a.positions, len(t))
        b, t = np.array(b[:k]), np.array(t[:k])
        if a.tile > k:
            b, t = np.tile(b, (-(-a.tile // k), 1))[:a.tile], np.tile(t, -(-a.tile // k))[:a.tile]
            k = a.tile
        boards = ops.from_numpy_u64(b, "cuda")
        turn = torch.from_numpy(t).cuda()
        alpha = beta = None  # the windows, one per position
        if windowed == "around":
            exact = (ops.solve(boards, turn, max_empties=e, node_limit=a.node_limit) if e <= _lib.SOLVE_MAX_EMPTIES else
                     ops.solve(boards, turn, max_empties=e, node_limit=a.node_limit, task_empties=8, order=1,
                               table=ops.SolveTable(22, "cuda")))
            assert bool((exact.status == 1).all()), "the full-window solve that --around centres on did not finish"
            alpha, beta = (exact.value - 1).contiguous(), (exact.value + 1).contiguous()
        elif windowed:
            lo, hi = (-1, 1) if a.wld else (int(x) for x in a.window.split(","))
            alpha = torch.full((k,), lo, dtype=torch.int8, device="cuda")
            beta = torch.full((k,), hi, dtype=torch.int8, device="cuda")

        def win(lo, hi):
            return {} if alpha is None else {"window": (alpha[lo:hi], beta[lo:hi])}

        methods = []
        if "lane" in a.methods and e <= _lib.SOLVE_MAX_EMPTIES:
            methods.append(("lane", lambda bb, tt, **kw: ops.solve(bb, tt, max_empties=e, node_limit=a.node_limit,
                                                                   want_nodes=True, **kw)))
        if "search" in a.methods and 4 < e <= _lib.SEARCH_MAX_DEPTH + 4 and not windowed:
            methods.append(("search", lambda bb, tt: ops.search(bb, tt, e, node_limit=a.node_limit, want_nodes=True,
                                                                split=4, order=1)))
        if "split" in a.methods:
            for te in a.task_empties:
                for o in a.order:
                    if not a.no_plain:
                        methods.append(("T%do%d" % (te, o), lambda bb, tt, te=te, o=o, **kw: ops.solve(
                            bb, tt, max_empties=e, node_limit=a.node_limit, want_nodes=True, task_empties=te, order=o,
                            nodes_per_position=a.nodes_per_position, **kw)))
                    for bits in a.hash_bits:
                        for gate in a.hash_min_empties:
                            for kept in (False, True):
                                methods.append(("T%do%dh%dg%d%s" % (te, o, bits, gate, "k" if kept else "f"),
                                                hashed_method(ops, a, e, te, o, bits, gate, kept)))
        launches = [(i, i + a.batch) for i in range(0, k - a.batch + 1, a.batch)]
        for name, fn in methods:
            fn(boards[:1], turn[:1], **win(0, 1))  # warm-up
            torch.cuda.synchronize()
            if hasattr(fn, "table"):
                fn.table.clear()
            ms, nodes, status, unsolved = [], 0, {}, []
            t_start = time.perf_counter()
            for lo, hi in launches:
                if hasattr(fn, "table") and not fn.kept:
                    fn.table.clear()
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn(boards[lo:hi], turn[lo:hi], **win(lo, hi))
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                nodes += int(r.nodes.cpu().numpy().view(np.uint32).astype(np.int64).sum())
                st = r.status.cpu().numpy()
                for s, c in zip(*np.unique(st, return_counts=True)):
                    status[int(s)] = status.get(int(s), 0) + int(c)
                unsolved += [lo + int(i) for i in np.nonzero(st != 1)[0]]
                if time.perf_counter() - t_start > a.budget_s:
                    break
            line = {"empties": e, "method": name, "window": windowed, "batch": a.batch, "launches": len(ms), "of": len(launches),
                    "ms_median": statistics.median(ms), "ms_max": max(ms), "ms_sum": sum(ms), "nodes": nodes,
                    "status_counts": status, "unsolved": unsolved, "node_limit": a.node_limit,
                    "nodes_per_position": a.nodes_per_position if name.startswith("T") else None,
                    "solve_blocks": os.environ.get("OTH_SOLVE_BLOCKS"), "tag": a.tag, "library_sha16": sha}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
