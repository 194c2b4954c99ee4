#!/usr/bin/env python
"""What the principal-variation calls cost (ops.solve_line / ops.search_line,
DESIGN.md §24) against the calls that answer with one value and one move, on
the same positions in the same process.  One JSON line per measurement, each
with the library_sha16; medians over --reps launches after one warm-up, the
worst beside.

  exact   32,768 positions of tests/solve_cases.pool() at --empties (tiled):
          ops.solve, ops.solve_line, and the host loop the call replaces (per
          ply one ops.solve and one ops.step of the lines still running; its
          lines are compared equal first); node sums and the longest line
  search  ops.sample_midgame(32768, 0x5EED) at --depths: ops.search against
          ops.search_line, both orders (there is no host loop that gives these
          lines: ops.search on a child scores the leaves from the other side)
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
    """The exact lines from today's calls: per ply one ops.solve of the lines still running and one ops.step of
    their moves.  (line, length, launches)."""
    n = boards.shape[0]
    line = torch.full((n, _lib.LINE_STRIDE), 255, dtype=torch.uint8, device=boards.device)
    length = torch.zeros(n, dtype=torch.int64, device=boards.device)
    idx = torch.arange(n, device=boards.device)
    b, t = boards, turn
    launches = 0
    while idx.numel():
        r = ops.solve(b, t, max_empties=max_empties, node_limit=node_limit)
        launches += 2
        keep = r.best_move != 255
        idx, b, t, mv = idx[keep], b[keep].contiguous(), t[keep].contiguous(), r.best_move[keep].contiguous()
        line[idx, length[idx]] = mv
        length[idx] += 1
        st = ops.step(b, t, mv, want_flips=False, want_legal=False)
        b, t = st.boards, torch.where(t == 2, 1, 2).to(torch.uint8)  # (the other side, whatever the step made of a pass)
    return line, length, launches


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["exact", "search"])
    p.add_argument("--empties", type=int, nargs="+", default=[8, 10])
    p.add_argument("--depths", type=int, nargs="+", default=[4, 5])
    p.add_argument("--positions", type=int, default=32768)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--node-limit", type=int, default=1 << 26)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    import solve_cases

    base = {"library_sha16": _lib.library_sha16(), "reps": a.reps, "tag": a.tag, "node_limit": a.node_limit}

    def emit(**kw):
        print(json.dumps({**kw, **base}), flush=True)

    if "exact" in a.sections:
        for e in a.empties:
            pool = solve_cases.pool()[e]
            k = len(pool["turn"])
            reps_ = -(-a.positions // k)
            b = np.tile(pool["boards"], (reps_, 1))[:a.positions]
            t = np.tile(pool["turn"], reps_)[:a.positions]
            bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t.copy()).cuda()
            kw = dict(max_empties=e, node_limit=a.node_limit)
            ms_s, mx_s, rs = timed(lambda: ops.solve(bt, tt, want_nodes=True, **kw), a.reps)
            ms_l, mx_l, rl = timed(lambda: ops.solve_line(bt, tt, want_nodes=True, **kw), a.reps)
            ms_h, mx_h, (hl, hn, launches) = timed(lambda: host_loop(bt, tt, e, a.node_limit), a.reps)
            assert torch.equal(hl, rl.line) and torch.equal(hn, rl.length.long()), "the host loop and ops.solve_line disagree"
            assert torch.equal(rs.value, rl.value) and torch.equal(rs.best_move, rl.best_move)
            ns, nl = u32(rs.nodes), u32(rl.nodes)
            emit(section="exact", empties=e, positions=a.positions, distinct=k, solve_ms=ms_s, solve_ms_max=mx_s,
                 line_ms=ms_l, line_ms_max=mx_l, loop_ms=ms_h, loop_ms_max=mx_h, loop_launches=launches,
                 time_ratio=ms_l / ms_s, loop_over_line=ms_h / ms_l, solve_nodes=int(ns.sum()),
                 line_nodes=int(nl.sum()), node_ratio=float(nl.sum() / max(ns.sum(), 1)),
                 position_nodes_max=int(ns.max()), line_position_nodes_max=int(nl.max()),
                 length_max=int(rl.length.max()), length_mean=float(rl.length.float().mean()),
                 solve_ns_per_node=ms_s * 1e6 / max(ns.sum(), 1), line_ns_per_node=ms_l * 1e6 / max(nl.sum(), 1),
                 status=counts(rl.status))
    if "search" in a.sections:
        pos = ops.sample_midgame(a.positions, 0x5EED)
        for d in a.depths:
            for order in (0, 1):
                kw = dict(node_limit=a.node_limit, want_nodes=True, order=order)
                ms_s, mx_s, rs = timed(lambda: ops.search(pos.boards, pos.turn, d, **kw), a.reps)
                ms_l, mx_l, rl = timed(lambda: ops.search_line(pos.boards, pos.turn, d, **kw), a.reps)
                assert torch.equal(rs.value, rl.value) and torch.equal(rs.best_move, rl.best_move)
                ns, nl = u32(rs.nodes), u32(rl.nodes)
                emit(section="search", depth=d, order=order, positions=a.positions, search_ms=ms_s, search_ms_max=mx_s,
                     line_ms=ms_l, line_ms_max=mx_l, time_ratio=ms_l / ms_s, search_nodes=int(ns.sum()),
                     line_nodes=int(nl.sum()), node_ratio=float(nl.sum() / max(ns.sum(), 1)),
                     position_nodes_max=int(ns.max()), line_position_nodes_max=int(nl.max()),
                     length_max=int(rl.length.max()), length_mean=float(rl.length.float().mean()),
                     search_ns_per_node=ms_s * 1e6 / max(ns.sum(), 1), line_ns_per_node=ms_l * 1e6 / max(nl.sum(), 1),
                     status=counts(rl.status))
    return 0


if __name__ == "__main__":
    sys.exit(main())
