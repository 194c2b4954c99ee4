#!/usr/bin/env python
"""How the Monte Carlo tree search plays (context for DESIGN.md §28, not a test):
--games games in lockstep, one ops.mcts and one ops.search call per ply over
all games, then ops.step with each game's mover's move.  The search side plays
ops.search at each of --depths with the default eval table (depth 1 is the
1-ply eval policy's move); colours alternate game by game.  One JSON line per
pairing with the numbers of games won, drawn and lost by the tree search.
--reuse 1 gives the tree search one tree per game that persists
(ops.MctsTrees): T more iterations where it is to move, and a re-root on every
move played, its own and the opponent's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from subproc_amd import _lib, ops  # noqa: E402


def play(n, T, depth, explore, seed, reuse=False):
    boards, turn, _ = ops.reset(n)
    mcts_black = torch.arange(n, device=boards.device) % 2 == 0
    trees = None
    if reuse:
        trees = ops.MctsTrees(n, min(1 + 32 * T, _lib.MCTS_MAX_NODES), boards.device)
        trees.init(boards, turn, game_id0=0, stride=1 << 32)
    for ply in range(130):  # (60 placements and the passes between them)
        legal = ops.legal(boards, turn)
        if bool(ops.result(boards).terminal.bool().all()):
            break
        if reuse:
            mine = (turn == 1) == mcts_black
            m = trees.search(torch.where(mine, T, 0).to(torch.int32), explore=explore, seed=seed)
        else:
            m = ops.mcts(boards, turn, T, explore=explore, seed=seed, game_id0=ply * n * T * 64)
        s = ops.search(boards, turn, depth)
        move = torch.where((turn == 1) == mcts_black, m.best_move, s.best_move)
        move = torch.where(legal == 0, torch.full_like(move, _lib.PASS), move)  # (a finished game passes on)
        if reuse:
            trees.advance(move)  # (a finished game's pass is refused: its tree stays)
        ops.step(boards, turn, move, inplace=True, want_flips=False, want_legal=False)
    diff = ops.result(boards).diff.to(torch.int32)
    mine = torch.where(mcts_black, diff, -diff)
    return int((mine > 0).sum()), int((mine == 0).sum()), int((mine < 0).sum()), float(mine.float().mean())


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--games", type=int, default=256)
    p.add_argument("--iterations", type=int, nargs="+", default=[64, 256])
    p.add_argument("--depths", type=int, nargs="+", default=[1, 4])
    p.add_argument("--explore", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--reuse", type=int, default=0, choices=[0, 1], help="1: trees that persist (ops.MctsTrees)")
    a = p.parse_args()
    for T in a.iterations:
        for depth in a.depths:
            won, drawn, lost, mean = play(a.games, T, depth, a.explore, a.seed, bool(a.reuse))
            print(json.dumps({"section": "match", "games": a.games, "iterations": T, "explore": a.explore,
                              "reuse": a.reuse, "opponent": "search depth %d" % depth, "won": won, "drawn": drawn, "lost": lost,
                              "win_rate": (won + 0.5 * drawn) / a.games, "mean_disc_difference": mean,
                              "library_sha16": _lib.library_sha16()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
