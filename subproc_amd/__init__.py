"""subproc_amd — MI355X-native batched Othello environment (the board.py step
path of ysnrkdm/subproc, re-designed for gfx950).

Modules:
  ops     tensor-level batched kernels (reset / legal / step / result / rollout / solve / search / play)
  env     VecEnv: reset / legal_moves / step / result over N games in HBM
  board   drop-in ``board`` module: the reference Board class API
  codec   Edax move strings and book text (host side)
  dist    one-process-per-GPU sharded rollouts + histogram all-reduce
The compute lives in lib/libsubproc_amd_hip.so (C-ABI: include/othello.h and,
for the endgame solver, the depth-limited search and search self-play,
include/othello_solve.h, include/othello_search.h and include/othello_play.h).
``solve`` / ``SolveResult``, ``search`` / ``SearchResult`` and ``play`` /
``PlayResult`` are ops.solve, ops.search, ops.play and their result types.
"""
__version__ = "0.1.0"

from ._lib import (BLACK, HIST_BINS, PASS, WHITE, OthelloCallError, OthelloLibraryError, load as load_library,
                   version as library_version)

__all__ = ["BLACK", "WHITE", "PASS", "HIST_BINS", "OthelloLibraryError", "OthelloCallError", "load_library",
           "library_version", "solve", "SolveResult", "search", "SearchResult", "play", "PlayResult",
           "__version__"]


def __getattr__(name):
    # ops imports torch: bound on first use, so that `import subproc_amd` stays light
    if name in ("solve", "SolveResult", "search", "SearchResult", "play", "PlayResult"):
        from . import ops

        return getattr(ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
