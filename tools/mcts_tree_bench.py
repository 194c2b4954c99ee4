#!/usr/bin/env python
"""What the Monte Carlo search trees that persist cost (ops.MctsTrees,
ops.mcts_play).  One JSON line per measurement, each with the
library_sha16: wall ms around a synchronise, the median of --reps calls after
one warm-up and the worst beside.

  search    MctsTrees.search(T) from freshly initialised trees against
            ops.mcts(T) on the same roots (the first n of
            ops.sample_midgame(.., 0x5EED)), same process, the two calls
            alternating, for n in --positions and T in --iterations: ms of
            each, the ratio of the medians, and each side's spread (worst /
            median) in that alternation.  The init is outside the clock.
  advance   on --advance-trees trees: search(T), then advance(best move,
            keep): ms of the advance, the nodes per tree before and after, and
            the advance's share of a ply (advance / (search + advance))
  play      ops.mcts_play on --games games from the opening at --play-iterations,
            with and without reuse, against the host loop it replaces (one
            ops.mcts and one ops.step per ply over all games, as
            tools/mcts_match.py plays; it runs on any commit that has ops.mcts):
            wall ms, playouts/s (searches made x T x 64), and with reuse the
            mean visits a root had when its move was chosen
  strength  reuse against no reuse at equal T over --strength-games games,
            colours alternating: won / drawn / lost by the side that reuses
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from subproc_amd import _lib, ops  # noqa: E402

SEED = 0xC0FFEE


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    return {"ms": statistics.median(ms), "ms_max": max(ms), "spread": max(ms) / statistics.median(ms)}


def emit(section, **kw):
    print(json.dumps({"section": section, **kw, "library_sha16": _lib.library_sha16()}), flush=True)


def search_section(a):
    for n in a.positions:
        pos = ops.sample_midgame(n, seed=0x5EED)
        for T in a.iterations:
            M = min(1 + 16 * T, _lib.MCTS_MAX_NODES)
            trees = ops.MctsTrees(n, M)

            def fresh():
                trees.init(pos.boards, pos.turn, game_id0=0, stride=T * 64)

            def one():
                return ops.mcts(pos.boards, pos.turn, T, seed=SEED, max_nodes=M, want_nodes=True)

            def mine():
                return trees.search(T, seed=SEED)

            fresh(), mine(), one()  # warm-up
            old, new = [], []
            for _ in range(a.reps):
                ms, r0 = clocked(one)
                old.append(ms)
                fresh()
                ms, r1 = clocked(mine)
                new.append(ms)
            same = all(torch.equal(getattr(r0, k), getattr(r1, k)) for k in r0._fields)
            emit("search", positions=n, iterations=T, max_nodes=M, grid=_lib.load().othr_trees_grid(n),
                 mcts=stats(old), trees=stats(new), ratio=statistics.median(new) / statistics.median(old),
                 same_answers=same, playouts_per_s=n * T * 64 / statistics.median(new) * 1e3)
            del trees


def advance_section(a):
    n = a.advance_trees
    pos = ops.sample_midgame(n, seed=0x5EED)
    for T in a.advance_iterations:
        M = min(1 + 16 * T, _lib.MCTS_MAX_NODES)
        trees = ops.MctsTrees(n, M)
        search, adv, before, after = [], [], 0.0, 0.0
        for rep in range(a.reps + 1):
            trees.init(pos.boards, pos.turn, game_id0=0, stride=T * 64)
            ms_s, r = clocked(lambda: trees.search(T, seed=SEED))
            move, nodes = r.best_move.clone(), r.nodes.float().mean().item()
            ms_a, _ = clocked(lambda: trees.advance(move, keep=True))
            if rep:  # (the first is the warm-up)
                search.append(ms_s), adv.append(ms_a)
                before, after = nodes, trees.rows().nodes.float().mean().item()
        emit("advance", trees=n, iterations=T, max_nodes=M, nodes_before=before, nodes_kept=after, advance=stats(adv),
             search=stats(search), share_of_ply=statistics.median(adv) / (statistics.median(adv) +
                                                                         statistics.median(search)))
        del trees


def host_loop(n, T, seed):
    """tools/mcts_match.py's way: one ops.mcts and one ops.step per ply over all games, one host read per ply."""
    boards, turn, _ = ops.reset(n)
    searches = 0
    for ply in range(130):
        legal = ops.legal(boards, turn)
        if bool(ops.result(boards).terminal.bool().all()):
            break
        m = ops.mcts(boards, turn, T, seed=seed, game_id0=ply * n * T * 64)
        move = torch.where(legal == 0, torch.full_like(m.best_move, _lib.PASS), m.best_move)
        ops.step(boards, turn, move, inplace=True, want_flips=False, want_legal=False)
        searches += n
    return searches


def play_section(a):
    n, T = a.games, a.play_iterations
    runs = {"host loop": lambda: host_loop(n, T, 7),
            "mcts_play reuse=0": lambda: ops.mcts_play(n, 7, iterations=T, reuse=False),
            "mcts_play reuse=1": lambda: ops.mcts_play(n, 7, iterations=T, reuse=True)}
    ms = {k: [] for k in runs}
    last = {}
    for rep in range(a.reps + 1):
        for k, fn in runs.items():  # alternating
            t, last[k] = clocked(fn)
            if rep:
                ms[k].append(t)
    for k in runs:
        r = last[k]
        extra = {}
        if isinstance(r, int):
            searches = r  # (every game at every ply, finished or not)
        else:
            searches = int(r.plies.sum()) + n  # (and each game's last search, which finds it over)
            extra = {"plies_mean": float(r.plies.float().mean()),
                     "root_visits_mean": float(r.root_visits.sum()) / float(r.plies.sum()),
                     "a_wins": int(((r.diff > 0) == (r.a_black != 0))[r.diff != 0].sum()),
                     "draws": int((r.diff == 0).sum())}
        emit("play", how=k, games=n, iterations=T, **stats(ms[k]), searches=searches,
             playouts_per_s=searches * T * 64 / statistics.median(ms[k]) * 1e3, **extra)


def strength_section(a):
    for T in a.strength_iterations:
        r = ops.mcts_play(a.strength_games, 7, iterations=T, reuse=(True, False))
        torch.cuda.synchronize()
        mine = torch.where(r.a_black != 0, r.diff.int(), -r.diff.int())
        emit("strength", games=a.strength_games, iterations=T, a="reuse", b="no reuse", won=int((mine > 0).sum()),
             drawn=int((mine == 0).sum()), lost=int((mine < 0).sum()), mean_disc_difference=float(mine.float().mean()),
             a_root_visits_mean=float(r.root_visits.sum()) / float(r.plies.sum()))


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["search", "advance", "play", "strength"])
    p.add_argument("--positions", type=int, nargs="+", default=[1, 64, 4096, 32768])
    p.add_argument("--iterations", type=int, nargs="+", default=[64, 256])
    p.add_argument("--advance-trees", type=int, default=4096)
    p.add_argument("--advance-iterations", type=int, nargs="+", default=[16, 64, 256, 1024])
    p.add_argument("--games", type=int, default=32768)
    p.add_argument("--play-iterations", type=int, default=64)
    p.add_argument("--strength-games", type=int, default=256)
    p.add_argument("--strength-iterations", type=int, nargs="+", default=[64, 256])
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mcts_tree_bench needs a ROCm GPU")
    for name in a.sections:
        {"search": search_section, "advance": advance_section, "play": play_section,
         "strength": strength_section}[name](a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
