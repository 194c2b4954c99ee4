"""Batched env API of the reference's env driver — reset / legal_moves / step /
result — over N games resident in HBM.

The reference drives one game per process (game_runner.py:154-201: Board(),
puttables, put_s, is_game_over, n_black/n_white); VecEnv keeps the same
per-game semantics for N games at once, each call one HIP launch on torch's
current stream.  State layout: boards (N,2) int64 bit
patterns [black, white], turn (N,) uint8, nturn (N,) uint8.
"""
import torch

from . import _lib, codec, ops


class VecEnv:
    def __init__(self, n, device="cuda"):
        if n <= 0:
            raise ValueError("n must be positive")
        self.n = n
        self.device = torch.device(device)
        self.boards, self.turn, self.nturn = ops.reset(n, self.device)

    # reference: Board() per game (game_runner.py:169)
    def reset(self, mask=None):
        """Reset every game, or only those where the bool tensor `mask` is set."""
        b, t, nt = ops.reset(self.n, self.device)
        if mask is None:
            self.boards, self.turn, self.nturn = b, t, nt
        else:
            self.boards = torch.where(mask[:, None], b, self.boards)
            self.turn = torch.where(mask, t, self.turn)
            self.nturn = torch.where(mask, nt, self.nturn)
        return self.boards, self.turn

    # reference: puttables(turn) (game_runner.py:137)
    def legal_moves(self):
        return ops.legal(self.boards, self.turn)

    # reference: put_s(hand) (game_runner.py:157)
    def step(self, moves):
        """Apply one move code per game (uint8: 0..63, 64 = pass) in place.
        Returns (ret int8, flips int64, legal_next int64) where ret follows
        board.put_s: -1 illegal/unchanged, 0 pass, n >= 1 discs flipped."""
        if moves.dtype != torch.uint8:
            moves = moves.to(torch.uint8)
        r = ops.step(self.boards, self.turn, moves.contiguous(), nturn=self.nturn, inplace=True)
        return r.ret, r.flips, r.legal_next

    def step_strings(self, hands):
        """Edax move strings per game ('d3', 'PS', ...), parsed on the host as put_s does."""
        codes = torch.tensor([codec.move_code(h) for h in hands], dtype=torch.uint8)
        return self.step(codes.to(self.device))

    # reference: is_game_over + n_black/n_white result rule (game_runner.py:162, 194-199)
    def result(self):
        """dict(n_black, n_white, diff, terminal, winner) with winner 1 Black, 2 White, 0 draw."""
        r = ops.result(self.boards)
        d = r.diff
        winner = torch.where(d > 0, 1, torch.where(d < 0, 2, 0)).to(torch.uint8)
        return dict(n_black=r.n_black, n_white=r.n_white, diff=d, terminal=r.terminal.bool(), winner=winner)

    def is_game_over(self):
        return ops.result(self.boards).terminal.bool()

    def solve(self, max_empties=12, node_limit=0, task_empties=None, order=0,
              nodes_per_position=_lib.SOLVE_TREE_DEFAULT_NODES, table=None,
              hash_min_empties=_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES, window=None, wld=False):
        """Exact endgame solve of the current state (ops.solve): per game the
        disc difference under perfect play from the mover's side and the move
        that achieves it, for the games with at most `max_empties` empties.
        `task_empties` = T: the split solver, for a few games at a time and up
        to 16 empties; `order` = 1 orders the moves inside its tasks; `table`
        (an ops.SolveTable, kept by the caller) gives them a transposition
        table, `hash_min_empties` its gate: the same answers.  `window` =
        (alpha, beta), ints or int8 per-game tensors, asks for the value
        clamped into the window only; `wld=True` is the window (-1, 1): who
        wins, and a winning (or drawing) move."""
        return ops.solve(self.boards, self.turn, max_empties=max_empties, node_limit=node_limit,
                         task_empties=task_empties, order=order, nodes_per_position=nodes_per_position, table=table,
                         hash_min_empties=hash_min_empties, window=window, wld=wld)

    def search(self, depth, weights=None, node_limit=0, split=0, order=0):
        """Depth-limited search of the current state (ops.search): per game the
        `depth`-ply alpha-beta value under the eval table `weights` from the
        mover's side and the move that achieves it.  `split` >= 1: the split
        search, for a few games at a time and depths up to 8 + split; `order` = 1 the
        ordered search (the same results from a smaller tree)."""
        return ops.search(self.boards, self.turn, depth, weights=weights, node_limit=node_limit, split=split,
                          order=order)

    def search_budget(self, budget, max_depth=8, weights=None, order=0, want_nodes=False):
        """Search of the current state by node budget (ops.search_budget): per
        game the value and move of the deepest iteration of an iterative
        deepening that fitted `budget` nodes (an int, or one per game), with the
        depth it reached; `max_depth` caps the depth."""
        return ops.search_budget(self.boards, self.turn, budget, max_depth=max_depth, weights=weights, order=order,
                                 want_nodes=want_nodes)

    def solve_moves(self, max_empties=12, node_limit=0, want_nodes=False, task_empties=None, order=0,
                    nodes_per_position=_lib.SOLVE_TREE_DEFAULT_NODES, table=None,
                    hash_min_empties=_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES):
        """The exact value of every legal move of the current state
        (ops.solve_moves): per game a row of 64 values from the mover's side
        (-128 where the square is no move) beside solve()'s value and move.
        With `task_empties` every move slot costs a slab of
        `nodes_per_position` nodes: pass a small one for many games."""
        return ops.solve_moves(self.boards, self.turn, max_empties=max_empties, node_limit=node_limit,
                               want_nodes=want_nodes, task_empties=task_empties, order=order,
                               nodes_per_position=nodes_per_position, table=table, hash_min_empties=hash_min_empties)

    def search_moves(self, depth, weights=None, node_limit=0, want_nodes=False):
        """The `depth`-ply value of every legal move of the current state
        (ops.search_moves), the leaves scored from the mover's side: per game a
        row of 64 int32 values (-2**31 where the square is no move) beside
        search()'s value and move."""
        return ops.search_moves(self.boards, self.turn, depth, weights=weights, node_limit=node_limit,
                                want_nodes=want_nodes)

    def solve_line(self, max_empties=12, node_limit=0, want_nodes=False):
        """The line of perfect play from the current state (ops.solve_line):
        per game up to 32 move codes (64 = pass, 255 = padding) beside solve()'s
        value and move, and the position where the line ends."""
        return ops.solve_line(self.boards, self.turn, max_empties=max_empties, node_limit=node_limit,
                              want_nodes=want_nodes)

    def search_line(self, depth, weights=None, order=0, node_limit=0, want_nodes=False):
        """The line of the `depth`-ply search from the current state
        (ops.search_line), every leaf scored from the mover's side: per game the
        moves down to the horizon beside search()'s value and move.  `depth` is
        an int or one uint8 per game (search_budget's `depth` output fits)."""
        return ops.search_line(self.boards, self.turn, depth, weights=weights, order=order, node_limit=node_limit,
                               want_nodes=want_nodes)

    def perft(self, depth, split=0, want_divide=False, want_nodes=False, node_limit=0, max_tasks=1 << 20):
        """Perft of the current state (ops.perft): per game the number of move
        paths of length `depth` (a pass is a ply, a finished game one path), with
        `want_divide` the count below every legal move.  `split` >= 1 spreads
        each game's tree over the device, for a few games at a time."""
        return ops.perft(self.boards, self.turn, depth, split=split, want_divide=want_divide, want_nodes=want_nodes,
                         node_limit=node_limit, max_tasks=max_tasks)

    def mcts(self, iterations, explore=0.5, seed=0, game_id0=0, max_nodes=None, log_table=None, want_nodes=False,
             leaves=None):
        """Monte Carlo tree search from the current state (ops.mcts): per game
        `iterations` iterations of 64 random playouts, the visits, half-points
        and disc sums of every root move and the most visited move.  `leaves`
        = L: the wide search, `iterations` rounds of L leaves each."""
        return ops.mcts(self.boards, self.turn, iterations, explore=explore, seed=seed, game_id0=game_id0,
                        max_nodes=max_nodes, log_table=log_table, want_nodes=want_nodes, leaves=leaves)

    def mcts_trees(self, max_nodes, id_base=None, game_id0=0, stride=0):
        """Search trees that persist, one per game, rooted at the current state
        (ops.MctsTrees, initialised): `.search(T)` resumes them, `.advance(moves)`
        re-roots them on the moves played and keeps the playouts below.  The
        trees do not follow `step`: advance them by the same moves."""
        trees = ops.MctsTrees(self.n, max_nodes, self.boards.device)
        trees.init(self.boards, self.turn, id_base=id_base, game_id0=game_id0, stride=stride)
        return trees

    def books(self):
        """Book text (serialize_str, board.py:214-221) of every game: oth_book_text
        on the device, one 67-byte line per game, decoded on the host."""
        raw = ops.book_text(self.boards, self.turn).cpu().numpy().tobytes()
        return raw.decode("ascii").splitlines()
