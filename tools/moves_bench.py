#!/usr/bin/env python
"""What the per-move calls cost (ops.solve_moves / ops.search_moves, DESIGN.md
§21) against the calls that answer with one value and one move, on the same
positions in the same process.  One JSON line per measurement, each with the
library_sha16; medians over --reps launches after one warm-up, the worst beside.

  lane    32,768 positions of tests/solve_cases.pool() at --lane-empties:
          ops.solve, ops.solve_moves, and the host loop the call replaces
          (ops.legal + per move rank ops.step + ops.solve + a scatter); node
          sums, and the tail: max / mean nodes of a position (ops.solve), of a
          position's moves together (ops.solve_moves) and of a single root move
          (ops.solve of every child, outside the timing)
  split   tests/solve_cases.ladder(E, 64) at --split-empties, one position per
          launch and all 64 in one, task_empties 8, order 1
  search  ops.sample_midgame(32768, 0x5EED) at --depths: ops.search against
          ops.search_moves (there is no host loop that gives these numbers)
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

from subproc_amd import _lib, ops  # noqa: E402


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


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def counts(status):
    return {int(s): int(c) for s, c in zip(*np.unique(status.cpu().numpy(), return_counts=True))}


def host_loop(boards, turn, max_empties, node_limit):
    """The per-move rows from today's calls: one ops.step and one ops.solve per move rank, then a scatter."""
    n = boards.shape[0]
    rows = torch.full((n, 64), _lib.MOVES_NOT_A_MOVE, dtype=torch.int8, device=boards.device)
    left = ops.legal(boards, turn)
    idx = torch.arange(n, device=boards.device)
    while True:
        keep = left != 0
        if not bool(keep.any()):
            return rows
        idx, left = idx[keep], left[keep]
        low = left & -left
        # the square of the lowest set bit: popcount(low - 1) by a table of the 64 single-bit words
        sq = torch.searchsorted(_BITS_SORTED, low.contiguous())
        sq = _BITS_ORDER[sq].to(torch.uint8)
        side = turn[idx].contiguous()
        st = ops.step(boards[idx].contiguous(), side, sq, want_flips=False, want_legal=False)
        other = torch.where(side == 2, 1, 2).to(torch.uint8)  # (the child's mover, whatever the step made of a pass)
        r = ops.solve(st.boards, other, max_empties=max_empties, node_limit=node_limit)
        rows[idx, sq.long()] = -r.value
        left = left ^ low


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["lane", "split", "search"])
    p.add_argument("--lane-empties", type=int, nargs="+", default=[8, 10, 12])
    p.add_argument("--split-empties", type=int, nargs="+", default=[12, 14, 16])
    p.add_argument("--depths", type=int, nargs="+", default=[2, 3, 4, 5, 6])
    p.add_argument("--positions", type=int, default=32768)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--node-limit", type=int, default=1 << 26)
    p.add_argument("--nodes-per-position", type=int, default=_lib.SOLVE_TREE_DEFAULT_NODES)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    import moves_ref
    import solve_cases

    global _BITS_SORTED, _BITS_ORDER
    bits = torch.tensor([(1 << k) - (1 << 64 if k == 63 else 0) for k in range(64)], dtype=torch.int64, device="cuda")
    _BITS_SORTED, _BITS_ORDER = torch.sort(bits)
    base = {"library_sha16": _lib.library_sha16(), "reps": a.reps, "tag": a.tag, "node_limit": a.node_limit}

    def emit(**kw):
        print(json.dumps({**kw, **base}), flush=True)

    if "lane" in a.sections:
        for e in a.lane_empties:
            pool = solve_cases.pool()[e]
            k = len(pool["turn"])
            reps_ = -(-a.positions // k)
            b = np.tile(pool["boards"], (reps_, 1))[:a.positions]
            t = np.tile(pool["turn"], reps_)[:a.positions]
            bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t.copy()).cuda()
            kw = dict(max_empties=e, node_limit=a.node_limit)
            ms_s, mx_s, rs = timed(lambda: ops.solve(bt, tt, want_nodes=True, **kw), a.reps)
            ms_m, mx_m, rm = timed(lambda: ops.solve_moves(bt, tt, want_nodes=True, **kw), a.reps)
            ms_h, mx_h, rows = timed(lambda: host_loop(bt, tt, e, a.node_limit), a.reps)
            assert torch.equal(rows, rm.move_value), "the host loop and ops.solve_moves disagree"
            ns, nm = u32(rs.nodes), u32(rm.nodes)
            ci, csq, cb, ct, _, _ = moves_ref.children(b[:k], t[:k])  # the distinct positions' moves
            rc = ops.solve(ops.from_numpy_u64(cb, "cuda"), torch.from_numpy(ct.copy()).cuda(), want_nodes=True, **kw)
            nt = u32(rc.nodes) + 1
            emit(section="lane", empties=e, positions=a.positions, distinct=k,
                 solve_ms=ms_s, solve_ms_max=mx_s, moves_ms=ms_m, moves_ms_max=mx_m, loop_ms=ms_h, loop_ms_max=mx_h,
                 time_ratio=ms_m / ms_s, loop_over_moves=ms_h / ms_m, solve_nodes=int(ns.sum()),
                 moves_nodes=int(nm.sum()), node_ratio=float(nm.sum() / max(ns.sum(), 1)),
                 position_nodes_max=int(ns.max()), position_nodes_mean=float(ns.mean()),
                 moves_position_nodes_max=int(nm.max()), moves_position_nodes_mean=float(nm.mean()),
                 task_nodes_max=int(nt.max()), task_nodes_mean=float(nt.mean()), tasks=int(len(nt)),
                 solve_ns_per_node=ms_s * 1e6 / max(ns.sum(), 1), moves_ns_per_node=ms_m * 1e6 / max(nm.sum(), 1),
                 status=counts(rm.status))
    if "split" in a.sections:
        for e in a.split_empties:
            b, t = solve_cases.ladder(e, 64)
            bt, tt = ops.from_numpy_u64(np.array(b), "cuda"), torch.from_numpy(np.array(t)).cuda()
            kw = dict(max_empties=e, node_limit=a.node_limit, task_empties=8, order=1, want_nodes=True,
                      nodes_per_position=a.nodes_per_position)
            for batch in (1, 64):
                spans = [(i, i + batch) for i in range(0, len(t) - batch + 1, batch)][:16]
                ms = {"solve": [], "moves": []}
                nodes = {"solve": 0, "moves": 0}
                status = {}
                for name, fn in (("solve", ops.solve), ("moves", ops.solve_moves)):
                    fn(bt[:1], tt[:1], **kw)
                    for lo, hi in spans:
                        m, _, r = timed(lambda: fn(bt[lo:hi], tt[lo:hi], **kw), 1 if batch == 1 else a.reps)
                        ms[name].append(m)
                        nodes[name] += int(u32(r.nodes).sum())
                        if name == "moves":
                            for s, c in counts(r.status).items():
                                status[s] = status.get(s, 0) + c
                emit(section="split", empties=e, batch=batch, launches=len(spans), task_empties=8, order=1,
                     nodes_per_position=a.nodes_per_position, solve_ms=statistics.median(ms["solve"]),
                     solve_ms_max=max(ms["solve"]), moves_ms=statistics.median(ms["moves"]),
                     moves_ms_max=max(ms["moves"]), time_ratio=statistics.median(ms["moves"]) / statistics.median(ms["solve"]),
                     solve_nodes=nodes["solve"], moves_nodes=nodes["moves"],
                     node_ratio=nodes["moves"] / max(nodes["solve"], 1), status=status)
    if "search" in a.sections:
        pos = ops.sample_midgame(a.positions, 0x5EED)
        for d in a.depths:
            ms_s, mx_s, rs = timed(lambda: ops.search(pos.boards, pos.turn, d, node_limit=a.node_limit, want_nodes=True),
                                   a.reps)
            ms_m, mx_m, rm = timed(lambda: ops.search_moves(pos.boards, pos.turn, d, node_limit=a.node_limit,
                                                            want_nodes=True), a.reps)
            assert torch.equal(rs.value, rm.value) and torch.equal(rs.best_move, rm.best_move)
            ns, nm = u32(rs.nodes), u32(rm.nodes)
            emit(section="search", depth=d, positions=a.positions, search_ms=ms_s, search_ms_max=mx_s, moves_ms=ms_m,
                 moves_ms_max=mx_m, time_ratio=ms_m / ms_s, search_nodes=int(ns.sum()), moves_nodes=int(nm.sum()),
                 node_ratio=float(nm.sum() / max(ns.sum(), 1)), position_nodes_max=int(ns.max()),
                 position_nodes_mean=float(ns.mean()), moves_position_nodes_max=int(nm.max()),
                 moves_position_nodes_mean=float(nm.mean()), search_ns_per_node=ms_s * 1e6 / max(ns.sum(), 1),
                 moves_ns_per_node=ms_m * 1e6 / max(nm.sum(), 1), status=counts(rm.status))
    return 0


if __name__ == "__main__":
    sys.exit(main())
