#!/usr/bin/env python
"""What the wide Monte Carlo tree search costs and how it plays
(ops.mcts(..., leaves=L)).  One JSON line per measurement, each
with the library_sha16; tools/mcts_bench.py's method: wall ms around a
synchronise, the median of --reps calls after one warm-up and the worst beside.

  rate      n roots for n in --positions (the first n of ops.sample_midgame(..,
            0x5EED)), N leaf visits for N in --visits, L in --leaves, R = N / L
            rounds: us per leaf visit; beside it ops.mcts(T = N) without
            `leaves` in the same process, the yardstick, and the ratio
  batch     the same at --batch-positions roots, --batch-visits leaf visits and
            --batch-leaves: what a wide block costs where one wave a tree
            already fills the device
  round     one root, from the rate lines of the largest N: the least-squares
            line us per round = a + b L over --leaves.  b is what one more
            walker adds to a round (wave 0's selection, expansion and marking,
            serial), a what a round costs whatever L (the playout, the back-up
            and the two barriers, parallel over the waves).  A fit over timing
            variants, not a counter
  strength  --games games in lockstep, colours alternating, c = --explore:
            the wide search of --match-rounds x --match-leaves against ops.mcts
            of as many iterations as rounds, against ops.mcts of as many
            iterations as leaf visits, and against the sum over --match-leaves
            ops.mcts trees of --match-rounds iterations each (root parallelism
            from the host: rows of one batch, their visits and wins summed)
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


def measure(emit, section, pos, n, N, leaves, explore, reps):
    """The yardstick and every L at n roots and N leaf visits; returns {L: us per round} of the wide calls."""
    b, t = pos.boards[:n].contiguous(), pos.turn[:n].contiguous()
    lib = _lib.load()
    yms, ymx, r = timed(lambda: ops.mcts(b, t, N, explore=explore, seed=SEED, want_nodes=True), reps)
    assert bool((r.status == _lib.MCTS_SEARCHED).all())
    y_us = yms * 1e3 / N
    emit(section=section, positions=n, visits=N, leaves=None, call="ops.mcts", grid=lib.othu_mcts_grid(n), ms=yms,
         ms_max=ymx, us_per_leaf_visit=y_us, nodes_mean=float(r.nodes.float().mean()))
    per_round = {}
    for L in leaves:
        R = N // L
        ms, mx, r = timed(lambda: ops.mcts(b, t, R, explore=explore, seed=SEED, want_nodes=True, leaves=L), reps)
        assert bool((r.status == _lib.MCTS_SEARCHED).all())
        per_round[L] = ms * 1e3 / R
        emit(section=section, positions=n, visits=R * L, leaves=L, rounds=R, call="ops.mcts leaves",
             grid=lib.othv_mcts_wide_grid(n, L), ms=ms, ms_max=mx, us_per_leaf_visit=ms * 1e3 / (R * L),
             us_per_round=per_round[L], ratio_to_yardstick=(ms * 1e3 / (R * L)) / y_us,
             nodes_mean=float(r.nodes.float().mean()))
    return per_round


def summed_move(r, legal, copies):
    """The move of the sum of `copies` consecutive rows: most visits, then more wins, then the lowest square."""
    n = r.visits.shape[0] // copies
    visits = r.visits.view(n, copies, 64).sum(1).long()
    wins = r.wins.view(n, copies, 64).sum(1).long()
    sq = torch.arange(64, device=visits.device)
    key = ((visits << 24) | wins) * 64 + (63 - sq)
    is_move = ((legal.unsqueeze(1) >> sq) & 1) != 0
    key = torch.where(is_move, key, torch.full_like(key, -1))
    return (63 - key.max(1).values % 64).to(torch.uint8)


def play(n, a_move, b_move):
    """n games in lockstep, A Black in the even games: (won, drawn, lost, mean disc difference) for A."""
    boards, turn, _ = ops.reset(n)
    a_black = torch.arange(n, device=boards.device) % 2 == 0
    for ply in range(130):  # (60 placements and the passes between them)
        legal = ops.legal(boards, turn)
        if bool(ops.result(boards).terminal.bool().all()):
            break
        move = torch.where((turn == 1) == a_black, a_move(boards, turn, legal, ply), b_move(boards, turn, legal, ply))
        move = torch.where(legal == 0, torch.full_like(move, _lib.PASS), move)  # (a finished game passes on)
        ops.step(boards, turn, move, inplace=True, want_flips=False, want_legal=False)
    diff = ops.result(boards).diff.to(torch.int32)
    mine = torch.where(a_black, diff, -diff)
    return int((mine > 0).sum()), int((mine == 0).sum()), int((mine < 0).sum()), float(mine.float().mean())


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--sections", nargs="+", default=["rate", "batch", "round", "strength"])
    p.add_argument("--positions", type=int, nargs="+", default=[1, 64])
    p.add_argument("--visits", type=int, nargs="+", default=[1024, 4096, 16384])
    p.add_argument("--leaves", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    p.add_argument("--batch-positions", type=int, nargs="+", default=[4096, 32768])
    p.add_argument("--batch-visits", type=int, default=256)
    p.add_argument("--batch-leaves", type=int, nargs="+", default=[4, 16])
    p.add_argument("--games", type=int, default=256)
    p.add_argument("--match-rounds", type=int, default=64)
    p.add_argument("--match-leaves", type=int, default=16)
    p.add_argument("--explore", type=float, default=0.5)
    p.add_argument("--match-seed", type=int, default=7)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    base = {"library_sha16": _lib.library_sha16(), "reps": a.reps, "tag": a.tag, "explore": a.explore}

    def emit(**kw):
        print(json.dumps({**kw, **base}), flush=True)

    pos = ops.sample_midgame(max(a.positions + a.batch_positions), seed=0x5EED)
    one_root = {}
    if "rate" in a.sections or "round" in a.sections:
        for n in a.positions:
            for N in a.visits:
                per_round = measure(emit, "rate", pos, n, N, a.leaves, a.explore, a.reps)
                if n == 1:
                    one_root[N] = per_round
    if "batch" in a.sections:
        for n in a.batch_positions:
            measure(emit, "batch", pos, n, a.batch_visits, a.batch_leaves, a.explore, a.reps)
    if "round" in a.sections and one_root and len(a.leaves) > 1:
        N = max(one_root)
        xs, ys = list(one_root[N]), list(one_root[N].values())
        mx, my = statistics.mean(xs), statistics.mean(ys)
        slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
        inter = my - slope * mx
        top = max(xs)
        emit(section="round", positions=1, visits=N, us_per_round=one_root[N], us_per_walker_serial=slope,
             us_per_round_parallel=inter, serial_share_at_most_leaves=slope * top / (inter + slope * top), leaves=top,
             us_per_leaf_visit_ceiling=slope, method="least squares over L of us per round = a + b L")
    if "strength" in a.sections:
        R, L, c, seed, n = a.match_rounds, a.match_leaves, a.explore, a.match_seed, a.games

        def wide(boards, turn, legal, ply):
            return ops.mcts(boards, turn, R, explore=c, seed=seed, game_id0=ply * n * R * L * 64, leaves=L).best_move

        def one_wave(T, salt):
            def move(boards, turn, legal, ply):
                return ops.mcts(boards, turn, T, explore=c, seed=seed + salt, game_id0=ply * n * T * 64).best_move
            return move

        def root_parallel(boards, turn, legal, ply):
            b = boards.repeat_interleave(L, dim=0).contiguous()
            t = turn.repeat_interleave(L).contiguous()
            r = ops.mcts(b, t, R, explore=c, seed=seed + 2, game_id0=ply * n * L * R * 64)
            return summed_move(r, legal, L)

        for name, other in (("ops.mcts T = %d (equal rounds)" % R, one_wave(R, 1)),
                            ("ops.mcts T = %d (equal playouts)" % (R * L), one_wave(R * L, 1)),
                            ("sum of %d ops.mcts trees of T = %d (root parallel)" % (L, R), root_parallel)):
            won, drawn, lost, mean = play(n, wide, other)
            emit(section="strength", games=n, rounds=R, leaves=L, opponent=name, won=won, drawn=drawn, lost=lost,
                 win_rate=(won + 0.5 * drawn) / n, mean_disc_difference=mean)
    return 0


if __name__ == "__main__":
    sys.exit(main())
