#!/usr/bin/env python
"""Search self-play with the exact solver's endgame: one JSON
line per measurement, printed and appended to --out (default
profiles/play_solve_bench.jsonl).

The games: --games of them from ops.sample_midgame(., 0x5EED) ("midgame") and
from the opening with --n-rand random moves a side ("opening"), colours drawn;
players at fixed depth (--depth, --depth) ("fixed") or by budget (B, B) with cap
--cap, B = the mean nodes per ply of the depth --budget-depth games ("budget").

  twin   solve_empties = 8 against exact_empties = 8: the same moves (checked
         here on every field), so the ratio is the solver's machine and the
         null-window walk against the search's machine run to the end
  zone   solve_empties = 9..12 on the same games: time, nodes, nodes per game
         max / mean; the mean |diff(E) - diff(8)| over the same seeds (the label
         noise the longer zone removes); and, for scale, ops.solve alone on the
         positions where the games enter the zone (--floor), the floor no
         game's endgame can beat

Times are wall ms around a device synchronise, the median of --reps after one
warm-up call.  The share of a call spent in its second launch is not visible
from here: it is read from a kernel trace of one call (the tool then runs with
--reps 1 --only zone --zones E)."""
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

from subproc_amd import _lib, ops  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up
    ms, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), ms


def popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(1).reshape(x.shape)


def zone_entries(r, start, start_turn, e):
    """(boards, turn) on the device: each game's first recorded position with at most e empty squares."""
    rp = ops.replay(r.moves, r.plies, start, start_turn)
    pos = ops.to_numpy_u64(rp.boards).reshape(len(r.plies), -1, 2)
    inside = (64 - popcount(pos[:, :, 0] | pos[:, :, 1])) <= e
    inside &= np.arange(pos.shape[1])[None, :] <= r.plies.cpu().numpy().astype(np.int64)[:, None]
    has = inside.any(1)
    first = inside.argmax(1)
    g = np.nonzero(has)[0]
    turn = rp.turn.cpu().numpy().reshape(len(r.plies), -1)[g, first[g]]
    keep = (turn == 1) | (turn == 2)
    return ops.from_numpy_u64(pos[g[keep], first[g][keep]], "cuda"), torch.from_numpy(turn[keep]).cuda()


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--games", type=int, default=32768)
    p.add_argument("--depth", type=int, default=4)
    p.add_argument("--budget-depth", type=int, default=5)
    p.add_argument("--cap", type=int, default=8)
    p.add_argument("--n-rand", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--order", type=int, choices=[0, 1], default=0)
    p.add_argument("--zones", type=int, nargs="*", default=[9, 10, 11, 12])
    p.add_argument("--sources", nargs="*", default=["midgame", "opening"], choices=["midgame", "opening"])
    p.add_argument("--modes", nargs="*", default=["fixed", "budget"], choices=["fixed", "budget"])
    p.add_argument("--only", nargs="*", default=["twin", "zone"], choices=["twin", "zone"])
    p.add_argument("--floor", action="store_true", help="ops.solve alone on the zone-entry positions")
    p.add_argument("--node-limit", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "play_solve_bench.jsonl"))
    a = p.parse_args()
    n, sha = a.games, _lib.library_sha16()

    def emit(line):
        line.update({"games": n, "order": a.order, "library_sha16": sha})
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    def figures(r, ms, all_ms):
        nd = r.nodes.cpu().numpy().astype(np.float64)
        return {"ms": ms, "ms_all": all_ms, "nodes": int(nd.sum()), "game_nodes_mean": float(nd.mean()),
                "game_nodes_max": int(nd.max()), "tail_ratio": float(nd.max() / max(nd.mean(), 1.0)),
                "limit_hits": int((r.status != _lib.SEARCH_SEARCHED).sum())}

    mid = ops.sample_midgame(n, seed=0x5EED)
    for source in a.sources:
        start = dict(start=mid.boards, start_turn=mid.turn) if source == "midgame" else dict(
            n_rand_a=a.n_rand, n_rand_b=a.n_rand)
        base = dict(swap_colours=True, want_nodes=True, record_moves=True, order=a.order, node_limit=a.node_limit,
                    **start)
        for mode in a.modes:
            kw = dict(depth_a=a.depth, depth_b=a.depth, **base)
            tag = {"source": source, "mode": mode, "depth": a.depth}
            if mode == "budget":
                r = ops.play(n, 0x5EED, depth_a=a.budget_depth, depth_b=a.budget_depth, **base)
                budget = max(1, int(round(float(r.nodes.sum()) / float(r.plies.long().sum()))))
                kw = dict(depth_a=a.cap, depth_b=a.cap, budget=budget, **base)
                tag = {"source": source, "mode": mode, "budget": budget, "budget_of_depth": a.budget_depth, "cap": a.cap}
            x8, ms, all_ms = timed(lambda: ops.play(n, 0x5EED, solve_empties=8, **kw), a.reps)
            if "twin" in a.only:
                emit({"what": "solve_empties", "e": 8, **tag, **figures(x8, ms, all_ms)})
                s8, ms, all_ms = timed(lambda: ops.play(n, 0x5EED, exact_empties=8, **kw), a.reps)
                same = all(torch.equal(getattr(x8, k), getattr(s8, k)) for k in
                           ("final_boards", "diff", "plies", "moves", "a_black", "status", "hist"))
                emit({"what": "exact_empties", "e": 8, **tag, **figures(s8, ms, all_ms), "same_games": same})
            if "zone" not in a.only:
                continue
            d8 = x8.diff.cpu().numpy().astype(np.int64)
            for e in a.zones:
                r, ms, all_ms = timed(lambda: ops.play(n, 0x5EED, solve_empties=e, **kw), a.reps)
                line = {"what": "solve_empties", "e": e, **tag, **figures(r, ms, all_ms),
                        "mean_abs_diff_vs_e8": float(np.abs(r.diff.cpu().numpy().astype(np.int64) - d8).mean())}
                if a.floor:
                    zb, zt = zone_entries(r, base.get("start"), base.get("start_turn"), e)
                    sv, fms, fall = timed(lambda: ops.solve(zb, zt, max_empties=e, node_limit=a.node_limit,
                                                            want_nodes=True), a.reps)
                    sn = sv.nodes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                    # the same call from the zone-entry positions: every game parks at its start, so this is
                    # the second launch's work (random moves, spent long before, aside)
                    tail = {k: v for k, v in kw.items() if k not in ("start", "start_turn", "n_rand_a", "n_rand_b")}
                    en, ems, eall = timed(lambda: ops.play(len(zt), 0x5EED, start=zb, start_turn=zt, solve_empties=e,
                                                           **tail), a.reps)
                    line.update({"floor_positions": len(zt), "floor_ms": fms, "floor_ms_all": fall,
                                 "floor_nodes": int(sn.sum()), "floor_nodes_max": int(sn.max()),
                                 "endgame_ms": ems, "endgame_ms_all": eall, "endgame_nodes": int(en.nodes.sum()),
                                 "endgame_share": ems / ms})
                emit(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
