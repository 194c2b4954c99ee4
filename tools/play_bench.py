#!/usr/bin/env python
"""Throughput of search self-play (ops.play) against the host loop it replaces.

Games: --games of them (default 32,768: one per lane of 512 blocks) from
ops.sample_midgame(seed=0x5EED) starts with no random moves ("mid"), or from the
opening with random budgets (5, 5) ("open"); both players the default table, A
on Black; --depths pairs "a,b".  One JSON line per (source, depths):

  kernel    one ops.play launch (no move record): wall ms around a device
            synchronise, median of --reps; games/s, plies/s, nodes/s; per-game
            node sum mean / max / ratio (the launch lasts as long as its
            longest game); games stopped by the node limit
  host loop what the library offered before ops.play: per ply one ops.search
            per depth over the movers' positions and one ops.step over the
            batch, until every game is over.  It plays the kernel's games: the
            move stepped is the kernel's recorded one (so coin moves cost it
            nothing); `loop_moves_differing` counts the turns with two moves
            or more where the search's own move is another (0 without random
            budgets, at most the budgets' sum per game with them).  Timed in
            the same process, alternating with the kernel, --loop-reps times
  host      with tools/diag/play_host built: the same driver on 16 CPU threads
            over the first --host-games games (fewer once their nodes, known
            from the GPU run, pass --host-nodes), and whether its games agree

A launch or loop that took more than --slow-ms is not repeated.  OTH_PLAY_BLOCKS
in the environment caps the grid (recorded).
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools", "diag")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from subproc_amd import _lib, ops, params  # noqa: E402

HOST = os.path.join(ROOT, "tools", "diag", "play_host")
SEARCHED = _lib.SEARCH_SEARCHED


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def host_loop(b0, t0, moves, depths, limit):
    """(final boards, searched moves that differ from the recorded ones)."""
    n = moves.shape[0]
    if b0 is None:
        b, t, _ = ops.reset(n)
    else:
        b, t = b0.clone(), t0.clone()
    live = torch.ones(n, dtype=torch.bool, device=b.device)
    wrong = torch.zeros((), dtype=torch.int64, device=b.device)
    for ply in range(ops.MOVES_STRIDE):
        mv = moves[:, ply].contiguous()
        live = live & (mv != 255)
        if not bool(live.any()):
            break
        if depths[0] == depths[1]:
            best = ops.search(b, t, depths[0], node_limit=limit).best_move
        else:  # each mover's positions at its depth (A is Black)
            best = torch.empty_like(mv)
            for colour, d in ((1, depths[0]), (2, depths[1])):
                sel = t == colour
                best[sel] = ops.search(b[sel].contiguous(), t[sel].contiguous(), d, node_limit=limit).best_move
        own = ops.legal(b, t)
        searched = live & ((own & (own - 1)) != 0)  # a pass and a single move need no search
        wrong += (searched & (best != mv)).sum()
        st = ops.step(b, t, torch.where(live, mv, torch.full_like(mv, 64)), want_flips=False, want_legal=False)
        b = torch.where(live[:, None], st.boards, b)
        t = torch.where(live, st.turn, t)
    return b, wrong


def host_line(a, n, source, depths, start, turn, nodes, ref, order=0):
    if not os.path.exists(HOST) or a.host_games <= 0:
        return {}
    import play_host_check as phc

    k = min(n, a.host_games)
    while k > 16 and nodes[:k].sum() > a.host_nodes:
        k //= 2
    with tempfile.TemporaryDirectory() as d:
        args, out = os.path.join(d, "args"), os.path.join(d, "out")
        w = params.as_weights(params.DEFAULT_WEIGHTS)
        phc.write_args(args, k, a.seed, 0, depths, 0, a.budgets if source == "open" else (0, 0), False, a.node_limit,
                       w, w, None if start is None else ops.to_numpy_u64(start[:k]),
                       None if turn is None else turn[:k].cpu().numpy())
        r = subprocess.run([HOST, args, out, str(a.host_threads), str(order)], capture_output=True, text=True, check=True)
        h = json.loads(r.stderr.strip().splitlines()[-1])
        got = phc.read_out(out)
    same = ((got["final_boards"] == ref["final_boards"][:k]).all() and (got["plies"] == ref["plies"][:k]).all()
            and (got["nodes"] == ref["nodes"][:k]).all())
    return {"host_threads": a.host_threads, "host_games": k, "host_games_per_s": h["games_per_s"],
            "host_nodes_per_s": h["nodes"] / h["seconds"] if h["seconds"] > 0 else 0.0, "host_agrees": bool(same)}


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--depths", nargs="+", default=["1,1", "2,2", "3,3", "4,4", "5,5", "4,2"])
    p.add_argument("--sources", nargs="+", default=["mid", "open"], choices=["mid", "open"])
    p.add_argument("--games", type=int, default=32768)
    p.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    p.add_argument("--budgets", type=int, nargs=2, default=[5, 5])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--loop-reps", type=int, default=2)
    p.add_argument("--slow-ms", type=float, default=3000.0)
    p.add_argument("--node-limit", type=int, default=1 << 22)
    p.add_argument("--no-loop", action="store_true", help="skip the host-loop baseline")
    p.add_argument("--host-games", type=int, default=2048)
    p.add_argument("--host-nodes", type=float, default=4e8, help="host node budget per line")
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--order", type=int, nargs="+", choices=[0, 1], default=[0],
                   help="move ordering(s) of the kernel's searches, each a line (the host loop stays unordered)")
    a = p.parse_args()
    if a.node_limit <= 0:
        p.error("every launch carries a node limit")
    n = a.games
    warm = ops.play(64, a.seed, depth_a=2, node_limit=a.node_limit, record_moves=True)  # loads the code objects
    host_loop(None, None, warm.moves, (2, 1), a.node_limit)
    torch.cuda.synchronize()
    mid = ops.sample_midgame(n, seed=a.seed)
    for source in a.sources:
        start, turn = (mid.boards, mid.turn) if source == "mid" else (None, None)
        budgets = tuple(a.budgets) if source == "open" else (0, 0)
        for pair, order in [(p_, o) for p_ in a.depths for o in a.order]:
            depths = tuple(int(x) for x in pair.split(","))
            kw = dict(depth_a=depths[0], depth_b=depths[1], n_rand_a=budgets[0], n_rand_b=budgets[1], start=start,
                      start_turn=turn, node_limit=a.node_limit, order=order)
            rec = ops.play(n, a.seed, record_moves=True, want_nodes=True, **kw)  # the games, and a warm-up
            torch.cuda.synchronize()
            ms, loop_ms, wrong = [], [], None
            for rep in range(max(a.reps, a.loop_reps)):
                if rep < a.reps and not (ms and ms[-1] > a.slow_ms):
                    ms.append(timed(lambda: ops.play(n, a.seed, want_nodes=True, **kw))[1])
                if not a.no_loop and rep < a.loop_reps and not (loop_ms and loop_ms[-1] > a.slow_ms):
                    (fb, wrong), t_loop = timed(lambda: host_loop(start, turn, rec.moves, depths, a.node_limit))
                    loop_ms.append(t_loop)
            med = statistics.median(ms)
            nodes = rec.nodes.cpu().numpy().astype(np.int64)
            plies = rec.plies.cpu().numpy().astype(np.int64)
            status = rec.status.cpu().numpy()
            line = {"source": source, "depths": list(depths), "order": order, "budgets": list(budgets), "games": n,
                    "ms_per_launch": med, "ms_all": ms, "games_per_s": n / (med * 1e-3),
                    "plies_per_s": int(plies.sum()) / (med * 1e-3), "nodes_per_s": int(nodes.sum()) / (med * 1e-3),
                    "plies_mean": float(plies.mean()), "game_nodes_mean": float(nodes.mean()),
                    "game_nodes_max": int(nodes.max()), "game_tail_ratio": float(nodes.max() / max(nodes.mean(), 1e-9)),
                    "limit_hits": int((status != SEARCHED).sum()), "node_limit": a.node_limit,
                    "grid": _lib.load().otho_play_ordered_grid(n, order), "play_blocks": os.environ.get("OTH_PLAY_BLOCKS"),
                    "library_sha16": _lib.library_sha16()}
            if loop_ms:
                lmed = statistics.median(loop_ms)
                line.update({"loop_ms": lmed, "loop_ms_all": loop_ms, "loop_games_per_s": n / (lmed * 1e-3),
                             "kernel_over_loop": lmed / med, "loop_moves_differing": int(wrong),
                             "loop_finals_equal": bool(torch.equal(fb, rec.final_boards))})
            ref = {"final_boards": ops.to_numpy_u64(rec.final_boards).reshape(-1, 2), "plies": plies.astype(np.uint8),
                   "nodes": nodes.astype(np.uint64)}
            line.update(host_line(a, n, source, depths, start, turn, nodes, ref, order))
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
