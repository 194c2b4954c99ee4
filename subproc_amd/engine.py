"""Edax-protocol engine backed by the GPU env.

The reference drives external engines through pipes with the Player class
(game_runner.py:9-102).  This module answers exactly the commands Player sends,
so ``proc_a_path = python -m subproc_amd.engine --policy greedy`` plugs a GPU
policy into GameRunner unchanged:

  init          -> 1 line                                   (game_runner.py:35-39)
  go            -> 3 lines; joined they match
                   ">(.+) plays [WB]?([a-zA-Z][0-9]|PS)"     (game_runner.py:19-33)
                   and the engine plays that move on its board
  <move>        -> 3 lines matching "(.+) play ([a-zA-Z][0-9]|PS|ps)"  (game_runner.py:41-54);
                   the move ('d3', 'ps', ...) is applied for the side to move
                   (go_for also sends the engine its OWN randomised moves, 149)
  verbose p     -> 1 line (parameter description)           (game_runner.py:66-73)
  verbose 1     -> 13 lines: the board display, the last line "Black won" /
                   "White won" once the game is over with a winner
                   (Player.show parses "(Black|White) won", game_runner.py:75-91)
  verbose 0     -> after a "verbose 1": 1 line, "Game Over" once the game is
                   over (Player.show reads one line and looks for it, 92-95);
                   otherwise nothing (show_hamlet_param sends it unread, 70)
  quit          -> 1 line, exit                              (game_runner.py:56-64)
  hint          -> Edax's name for it: one line "<move> <value>" per legal move of
                   the side to move, best first (lowest square first among
                   equals), or the one line "hint unavailable" (policies random
                   and greedy outside --solve-empties); then an empty line.
                   Nothing is played.  Player never sends it.
  pv            -> one line "<value> <move> <move> ...": the line of best play
                   from the side to move (PS for a pass) and its value, from
                   ops.solve_line within --solve-empties (at most 12 empties),
                   else from ops.search_line for policy search (at --depth, or
                   the depth the last budget search reached) and policy eval
                   (depth 1); or the one line "pv unavailable" (policies random
                   and greedy, --split, more than 12 empties in the exact
                   range).  Nothing is played.  Player never sends it.
  perft D       -> ops.perft of the position at depth D (0..14; a pass is a ply,
                   a finished game one path): one line "<move> <count>" per legal
                   move of the side to move in a1..h8 order, then one line with
                   the total; or the one line "perft unavailable" (D out of
                   range, a task past its node limit).  Whatever the policy.
                   Nothing is played.  Player never sends it.

Rules and move generation run on the GPU through the drop-in Board
(subproc_amd.board); the move choice is the env's policy: "random" (uniform
over legal moves, seeded), "greedy" (minimise the opponent's mobility, ties
to the first move in puttables order) or "eval" (maximise the mover's linear
eval of the child under an eval table, ties likewise -- the kernels' eval
policy).  ``--params FILE`` loads the table from the file paramgen.py writes
(paramgen.py:12-19), the file the reference's own engines read.
``--solve-empties K`` (K = 1..12) plays the endgame perfectly, as the engines
this one stands in for do: with at most K empty squares and a legal move, the
move is the exact solver's (ops.solve: best final disc difference, ties to the
lowest square), whatever the policy.  ``--solve-task-empties T`` (T = 1..12)
makes that solve the split solver (ops.solve(task_empties=T), the position's
tree spread over the whole device) and lets K go to 16; ``--solve-order 1``
orders the moves inside its tasks (default: ``--order``'s value);
``--solve-hash-bits B`` (B = 4..26, needs ``--solve-task-empties``) gives the
tasks a transposition table of 2**B entries (ops.SolveTable) that the engine
keeps for its life, so successive ``go``s of one endgame reuse what the earlier
ones solved: the same moves.
``--solve-wld-empties W`` (W above ``--solve-empties``; at most 12, or 16 with
``--solve-task-empties``) asks the solver who wins before the exact score is
within reach: while more than K and at most W squares are empty, a ``go`` makes
one win/draw/loss solve (ops.solve(wld=True)) with the exact solve's node
limit, task settings and table.  On a proved win or draw the engine plays the
solver's move (the lowest winning, resp. drawing, square); on a proved loss, a
node limit or a tree that did not fit, the policy's move, as without the option.
``--policy search --depth D`` (D = 1..8) looks D plies ahead: the move is
ops.search's, a fixed-depth alpha-beta with the eval table at the horizon (one
launch per ``go``; depth 1 is the "eval" policy's move).  ``--solve-empties``
still takes precedence where it applies.  ``--split S`` (S = 1..4) makes that
search the split search (ops.search(split=S)): the position's tree is spread
over the whole device, and D may go to 8 + S.  ``--order 1`` searches with move
ordering (ops.search(order=1), include/othello_order.h): the same moves from a
smaller tree.  ``--nodes B`` (with ``--policy search``, without ``--split``)
gives every ``go`` a budget of B nodes instead of a fixed depth: the move is
ops.search_budget's, an iterative deepening whose deepest completed iteration
answers, ``--depth`` (at most 8) being its cap; "verbose 1" then shows the depth
the last search reached at the end of the board display's last line.
``--policy mcts --iterations T`` (T = 1..65536; ``--explore C``, default 0.5)
needs no eval table: every ``go`` is one ops.mcts call on the position, a Monte
Carlo tree search of T iterations of 64 random playouts, and plays its most
visited move.  The playouts are ``--seed``'s games; the k-th ``go`` (from 0)
takes the ids from k * T * 64, so no two ``go``s share a playout.
``--reuse 1`` (with ``--policy mcts``; default 0) keeps the search tree between
moves (ops.MctsTrees): every move played, the engine's own or the opponent's,
re-roots the tree on that move and keeps the playouts below it, and every ``go``
runs T more iterations on what is left.  A new game, or a position the tree
does not stand at, starts a tree from one node; the k-th such start (from 0)
takes the ids from k * 2**40.  The tree has room for 1 + 32 T nodes.
``--leaves L`` (with ``--policy mcts``, 1..16; not with ``--reuse 1``) makes
every ``go`` the wide search, ops.mcts(..., leaves=L): ``--iterations`` is then
the number R of rounds of L leaves each, R L at most 65536, one block of L waves
on the position, and the k-th ``go`` takes the ids from k * R * L * 64.
"""
import argparse
import random
import sys

import numpy as np
import torch

from . import board as gboard
from . import _lib, codec, ops, params
from .codec import handstr_from_coord


class Engine:
    def __init__(self, name="GPU", policy="greedy", seed=0, weights=None, solve_empties=0, depth=1, split=0, order=0,
                 solve_task_empties=None, solve_order=None, solve_hash_bits=None, solve_wld_empties=0, nodes=None,
                 iterations=None, explore=0.5, reuse=0, leaves=None):
        top = _lib.SOLVE_MAX_EMPTIES if solve_task_empties is None else _lib.SOLVE_TREE_MAX_EMPTIES
        if not 0 <= solve_empties <= top:
            raise ValueError(f"solve_empties must lie in 0..{top}" + (
                "" if solve_task_empties is not None else
                f" (up to {_lib.SOLVE_TREE_MAX_EMPTIES} with solve_task_empties)"))
        if solve_task_empties is not None and not 1 <= solve_task_empties <= _lib.SOLVE_MAX_EMPTIES:
            raise ValueError(f"solve_task_empties must lie in 1..{_lib.SOLVE_MAX_EMPTIES}")
        if solve_order is not None and solve_order not in (0, 1):
            raise ValueError("solve_order must be 0 or 1")
        if solve_hash_bits is not None:
            if solve_task_empties is None:
                raise ValueError("solve_hash_bits needs solve_task_empties: the table serves the split solver's tasks")
            if not _lib.SOLVE_HASH_MIN_BITS <= solve_hash_bits <= _lib.SOLVE_HASH_MAX_BITS:
                raise ValueError(f"solve_hash_bits must lie in {_lib.SOLVE_HASH_MIN_BITS}..{_lib.SOLVE_HASH_MAX_BITS}")
        if solve_wld_empties != 0:
            if not 1 <= solve_wld_empties <= top:
                raise ValueError(f"solve_wld_empties must lie in 1..{top}" + (
                    "" if solve_task_empties is not None else
                    f" (up to {_lib.SOLVE_TREE_MAX_EMPTIES} with solve_task_empties)"))
            if solve_wld_empties <= solve_empties:
                raise ValueError("solve_wld_empties must exceed solve_empties: below it the exact solve answers")
        if not 0 <= split <= _lib.TREE_MAX_SPLIT:
            raise ValueError(f"split must lie in 0..{_lib.TREE_MAX_SPLIT}")
        if not 1 <= depth <= _lib.SEARCH_MAX_DEPTH + split:
            raise ValueError(f"depth must lie in 1..{_lib.SEARCH_MAX_DEPTH + split}")
        if not 0 <= order <= _lib.ORDER_MAX:
            raise ValueError(f"order must lie in 0..{_lib.ORDER_MAX}")
        if nodes is not None:
            if policy != "search" or split != 0:
                raise ValueError("nodes applies to policy search without a split")
            if not 1 <= nodes < 2**32:
                raise ValueError("nodes must lie in 1..2**32 - 1")
            if depth > _lib.SEARCH_MAX_DEPTH:
                raise ValueError(f"with nodes, depth is the cap and must lie in 1..{_lib.SEARCH_MAX_DEPTH}")
        if policy == "mcts":
            if iterations is None or not 1 <= iterations <= _lib.MCTS_MAX_ITERATIONS:
                raise ValueError(f"policy mcts needs iterations in 1..{_lib.MCTS_MAX_ITERATIONS}")
        elif iterations is not None:
            raise ValueError("iterations applies to policy mcts")
        if leaves is not None:
            if policy != "mcts":
                raise ValueError("leaves applies to policy mcts")
            if reuse:
                raise ValueError("leaves applies to a search from one node: not with reuse")
            if not 1 <= leaves <= _lib.MCTS_WIDE_MAX_LEAVES or iterations * leaves > _lib.MCTS_MAX_ITERATIONS:
                raise ValueError(f"leaves must lie in 1..{_lib.MCTS_WIDE_MAX_LEAVES}, iterations x leaves in "
                                 f"1..{_lib.MCTS_MAX_ITERATIONS}")
        self.leaves = leaves
        if reuse not in (0, 1):
            raise ValueError("reuse must be 0 or 1")
        if reuse and policy != "mcts":
            raise ValueError("reuse applies to policy mcts")
        self.reuse = reuse
        self._trees = None    # reuse: the tree (ops.MctsTrees of one), made on the first go
        self._tree_at = None  # the position its root stands at, as _tree_key(); None: nowhere
        self._tree_inits = 0
        self.iterations = iterations
        self.explore = float(explore)
        self.seed = seed
        self.go_index = 0  # the searches made so far: each takes its own playout ids
        self.nodes = nodes
        self.reached = None  # the depth the last budget search reached
        self.solve_empties = solve_empties
        self.solve_wld_empties = solve_wld_empties
        self.solve_task_empties = solve_task_empties
        # (the solver's tasks take the search's --order unless --solve-order says otherwise)
        self.solve_order = (order if solve_order is None else solve_order) if solve_task_empties is not None else 0
        self.solve_hash_bits = solve_hash_bits
        self._solve_table = None  # made on the first solve, kept for the engine's life, never cleared
        self.order = order
        self.depth = depth
        # (a depth the split leaves no plies below is searched unsplit)
        self.split = split if depth > split else 0
        self.name = name
        self.policy = policy
        self.rng = random.Random(seed)
        self.weights = params.as_weights(params.DEFAULT_WEIGHTS if weights is None else weights)
        self.board = gboard.Board()
        self._shown = False  # a "verbose 1" awaits its "verbose 0" line

    def _children(self, puts, want_legal):
        """Every child of the side to move in ONE oth_step launch (board
        repeated per legal square): the StepResult on the device."""
        b = self.board
        bl, wh = b.bitboards()
        n = len(puts)
        dev = torch.device("cuda", torch.cuda.current_device())
        boards = ops.from_numpy_u64(np.array([[bl, wh]] * n, np.uint64), dev)
        side = torch.full((n,), b.turn, dtype=torch.uint8, device=dev)
        sq = torch.tensor([x + 8 * y for (x, y) in puts], dtype=torch.uint8, device=dev)
        return ops.step(boards, side, sq, want_flips=False, want_legal=want_legal), side

    def _choose_eval(self, puts):
        """The children's evals in one more oth_eval launch."""
        r, side = self._children(puts, want_legal=False)
        ev = ops.evaluate(r.boards, side, self.weights).cpu().tolist()
        k = max(range(len(puts)), key=lambda i: (ev[i], -i))  # puts is LSB-first: ties -> lowest square
        return handstr_from_coord(*puts[k])

    def _choose_greedy(self, puts):
        """A legal move hands the turn over, so each child's legal_next is the
        opponent's puttables: its popcount is n_puttable_for(hostile)."""
        r, _ = self._children(puts, want_legal=True)
        mob = [bin(v & (2**64 - 1)).count("1") for v in r.legal_next.cpu().tolist()]
        k = min(range(len(puts)), key=lambda i: (mob[i], i))  # ties -> lowest square
        return handstr_from_coord(*puts[k])

    def _choose_solved(self):
        """The solver's move for the side to move (one oths_solve launch, or
        othe_solve's with solve_task_empties), or None when it gives none (more
        than solve_empties empties; a node limit; a tree that did not fit).
        With more than solve_empties and at most solve_wld_empties empties the
        one solve is for win / draw / loss: its move, or None on a proved loss."""
        b = self.board
        bl, wh = b.bitboards()
        empties = 64 - bin(bl | wh).count("1")
        wld = empties > self.solve_empties
        if empties > (self.solve_wld_empties if wld else self.solve_empties):
            return None
        dev = torch.device("cuda", torch.cuda.current_device())
        boards = ops.from_numpy_u64(np.array([[bl, wh]], np.uint64), dev)
        side = torch.full((1,), b.turn, dtype=torch.uint8, device=dev)
        # (a position that would need more than 2**24 nodes -- none at <= 12
        # empties in DESIGN.md §12's samples -- falls back to the policy)
        if self.solve_hash_bits is not None and self._solve_table is None:
            self._solve_table = ops.SolveTable(self.solve_hash_bits, dev)
        r = ops.solve(boards, side, max_empties=self.solve_wld_empties if wld else self.solve_empties,
                      node_limit=1 << 24, task_empties=self.solve_task_empties, order=self.solve_order,
                      table=self._solve_table, wld=wld)
        sq = int(r.best_move.cpu()[0])
        if int(r.status.cpu()[0]) != _lib.SOLVE_SOLVED or sq > 63:
            return None
        return handstr_from_coord(sq & 7, sq >> 3)

    def _choose_searched(self):
        """The depth-limited search's move for the side to move (one
        othm_search launch, or otht_search's with a split), or None when it
        gives none (node limit; with a split, a tree that did not fit)."""
        b = self.board
        bl, wh = b.bitboards()
        dev = torch.device("cuda", torch.cuda.current_device())
        boards = ops.from_numpy_u64(np.array([[bl, wh]], np.uint64), dev)
        side = torch.full((1,), b.turn, dtype=torch.uint8, device=dev)
        if self.nodes is not None:  # by budget: the deepest completed iteration's move
            r = ops.search_budget(boards, side, self.nodes, max_depth=self.depth, weights=self.weights,
                                  order=self.order)
            self.reached = int(r.depth.cpu()[0])
        else:
            r = ops.search(boards, side, self.depth, weights=self.weights, node_limit=1 << 24, split=self.split,
                           order=self.order)
        sq = int(r.best_move.cpu()[0])
        if int(r.status.cpu()[0]) != _lib.SEARCH_SEARCHED or sq > 63:
            return None
        return handstr_from_coord(sq & 7, sq >> 3)

    def _choose_mcts(self):
        """The Monte Carlo tree search's move for the side to move (one
        othu_mcts launch), or None when it gives none."""
        boards, side, _ = self._position()
        if self.reuse:
            if self._tree_at != self._tree_key():
                if self._trees is None:
                    self._trees = ops.MctsTrees(1, min(1 + 32 * self.iterations, _lib.MCTS_MAX_NODES), boards.device)
                self._trees.init(boards, side, game_id0=self._tree_inits << 40)
                self._tree_inits += 1
                self._tree_at = self._tree_key()
            r = self._trees.search(self.iterations, explore=self.explore, seed=self.seed)
        else:
            r = ops.mcts(boards, side, self.iterations, explore=self.explore, seed=self.seed,
                         game_id0=self.go_index * self.iterations * (self.leaves or 1) * 64, leaves=self.leaves)
            self.go_index += 1
        sq = int(r.best_move.cpu()[0])
        if int(r.status.cpu()[0]) != _lib.MCTS_SEARCHED or sq > 63:
            return None
        return handstr_from_coord(sq & 7, sq >> 3)

    def _tree_key(self):
        return (*self.board.bitboards(), self.board.turn)

    def _put(self, mv):
        """board.put_s(mv), and with reuse the same move on the tree where it stands at the board's position."""
        before = self._tree_key() if self.reuse else None
        self.board.put_s(mv)
        if self._tree_at is None or self._tree_at != before:
            self._tree_at = None
            return
        try:
            code = codec.move_code(mv)
        except IndexError:
            code = codec.INVALID
        move = torch.full((1,), code, dtype=torch.uint8, device=self._trees.device)
        ok = code != codec.INVALID and int(self._trees.advance(move, keep=True).cpu()[0]) == _lib.MCTS_TREE_READY
        self._tree_at = self._tree_key() if ok else None

    def _position(self):
        """The board as a batch of one on the current device: (boards, side, empties)."""
        bl, wh = self.board.bitboards()
        dev = torch.device("cuda", torch.cuda.current_device())
        boards = ops.from_numpy_u64(np.array([[bl, wh]], np.uint64), dev)
        side = torch.full((1,), self.board.turn, dtype=torch.uint8, device=dev)
        return boards, side, 64 - bin(bl | wh).count("1")

    def hint(self):
        """The `hint` command's lines: "<move> <value>" for every legal move of
        the side to move, best first and lowest square first among equals, or
        ["hint unavailable"].  The values are ops.solve_moves' within
        solve_empties (the engine's task, order and table settings; final disc
        differences), else ops.search_moves' at the engine's depth (at most 8:
        there is no split here) for policy search, else at depth 1 for policies
        search and eval (the eval's units, 2**17 per disc where the game ends
        inside the horizon); a row with an unknown move falls through to the
        next source.  Policies random and greedy have no values of their own."""
        b = self.board
        if not b.puttables(b.turn) or b.turn not in (gboard.Black, gboard.White):
            return []
        boards, side, empties = self._position()
        rows = []  # (row, the value that marks a square that is no move), lazily
        if 0 < self.solve_empties and empties <= self.solve_empties:
            if self.solve_hash_bits is not None and self._solve_table is None:
                self._solve_table = ops.SolveTable(self.solve_hash_bits, boards.device)
            rows.append(lambda: (ops.solve_moves(boards, side, max_empties=self.solve_empties, node_limit=1 << 24,
                                                 task_empties=self.solve_task_empties, order=self.solve_order,
                                                 table=self._solve_table), _lib.MOVES_NOT_A_MOVE, _lib.MOVES_UNKNOWN))
        if self.policy in ("search", "eval"):
            depths = [min(self.depth, _lib.SEARCH_MAX_DEPTH), 1] if self.policy == "search" else [1]
            for d in dict.fromkeys(depths):
                rows.append(lambda d=d: (ops.search_moves(boards, side, d, weights=self.weights, node_limit=1 << 24),
                                         _lib.MOVES_NOT_A_MOVE32, _lib.MOVES_UNKNOWN32))
        for source in rows:
            r, no_move, unknown = source()
            row = r.move_value[0].cpu().tolist()
            if unknown in row:
                continue
            best = sorted((sq for sq in range(64) if row[sq] != no_move), key=lambda sq: (-row[sq], sq))
            return ["%s %d" % (handstr_from_coord(sq & 7, sq >> 3).upper(), row[sq]) for sq in best]
        return ["hint unavailable"]

    def pv(self):
        """The `pv` command's line: "<value> <move> <move> ..." (Edax move
        strings, PS for a pass), the line of best play from the side to move
        and the value it stands for, or "pv unavailable".  Within solve_empties
        it is ops.solve_line's (at most 12 empties: there is no line through
        the split solver; the final disc difference), whatever the policy; else
        ops.search_line's for policy search at the engine's depth (with nodes:
        the depth the last go reached) and for policy eval at depth 1 (the
        eval's units).  Policies random and greedy have no line of their own,
        and there is none through the split search."""
        if self.board.turn not in (gboard.Black, gboard.White):
            return "pv unavailable"
        boards, side, empties = self._position()
        r = None
        if 0 < self.solve_empties and empties <= self.solve_empties:
            if empties > _lib.SOLVE_MAX_EMPTIES:
                return "pv unavailable"
            r = ops.solve_line(boards, side, max_empties=min(self.solve_empties, _lib.SOLVE_MAX_EMPTIES),
                               node_limit=1 << 24)
        elif self.policy in ("search", "eval") and self.split == 0:
            depth = 1 if self.policy == "eval" else self.depth if self.nodes is None else (self.reached or 0)
            if 1 <= depth <= _lib.SEARCH_MAX_DEPTH:
                r = ops.search_line(boards, side, depth, weights=self.weights, order=self.order, node_limit=1 << 24)
        if r is None or int(r.status.cpu()[0]) != _lib.SOLVE_SOLVED:  # (== SEARCH_SEARCHED)
            return "pv unavailable"
        line = r.line[0, :int(r.length.cpu()[0])].cpu().tolist()
        return " ".join(["%d" % int(r.value.cpu()[0])] + [
            "PS" if sq == _lib.PASS else handstr_from_coord(sq & 7, sq >> 3).upper() for sq in line])

    def perft(self, depth):
        """The `perft D` command's lines: "<move> <count>" for every legal move
        of the side to move, lowest square first, then the total; or ["perft
        unavailable"].  The tree's top plies become tasks for the whole device
        (ops.perft's split: the fastest measured)."""
        if self.board.turn not in (gboard.Black, gboard.White) or not 0 <= depth <= _lib.PERFT_MAX_DEPTH:
            return ["perft unavailable"]
        boards, side, _ = self._position()
        split = _lib.PERFT_MAX_SPLIT if depth >= 12 else min(max(depth - 3, 1), 7)
        r = ops.perft(boards, side, depth, split=split, want_divide=True)
        if int(r.status.cpu()[0]) != _lib.PERFT_COUNTED:
            return ["perft unavailable"]
        row = r.divide[0].cpu().tolist()
        return ["%s %d" % (handstr_from_coord(sq & 7, sq >> 3).upper(), row[sq]) for sq in range(64) if row[sq]] + [
            "%d" % int(r.leaves.cpu()[0])]

    def choose(self):
        b = self.board
        puts = b.puttables(b.turn)
        if not puts:
            return "PS"
        if (self.solve_empties > 0 or self.solve_wld_empties > 0) and b.turn in (gboard.Black, gboard.White):
            mv = self._choose_solved()
            if mv is not None:
                return mv
        if self.policy == "random":
            x, y = puts[self.rng.randrange(len(puts))]
            return handstr_from_coord(x, y)
        if self.policy == "search" and b.turn in (gboard.Black, gboard.White):
            mv = self._choose_searched()
            if mv is not None:
                return mv
        if self.policy == "mcts" and b.turn in (gboard.Black, gboard.White):
            mv = self._choose_mcts()
            if mv is not None:
                return mv
        if self.policy in ("eval", "search"):  # (search: its LIMIT / NOROOM fall-back)
            return self._choose_eval(puts)
        return self._choose_greedy(puts)

    def handle(self, line, out):
        cmd = line.strip()
        if cmd == "init":
            self.board = gboard.Board()
            self._tree_at = None
            out("init done")
        elif cmd == "go":
            mv = self.choose()
            color = "B" if self.board.turn == gboard.Black else "W"
            self._put(mv.lower() if mv != "PS" else "PS")
            out("")
            out(">%s plays %s%s" % (self.name, color, mv.upper() if mv != "PS" else "PS"))
            out("")
        elif cmd == "hint":
            for t in self.hint():
                out(t)
            out("")
        elif cmd == "pv":
            out(self.pv())
        elif cmd.split()[:1] == ["perft"]:
            arg = cmd.split()[1:]
            ok = len(arg) == 1 and arg[0].isdigit()
            for t in (self.perft(int(arg[0])) if ok else ["perft unavailable"]):
                out(t)
        elif cmd == "verbose p":
            extra = " weights=%s" % self.weights.reshape(-1).tolist() if self.policy in ("eval", "search") else ""
            if self.policy == "mcts":
                extra = " iterations=%d explore=%g" % (self.iterations, self.explore) + (
                    " reuse=1" if self.reuse else "") + (" leaves=%d" % self.leaves if self.leaves else "")
            if self.policy == "search":
                extra = " depth=%d" % self.depth + (" nodes=%d" % self.nodes if self.nodes is not None else "") + (
                    " split=%d" % self.split if self.split > 0 else "") + (
                    " order=%d" % self.order if self.order > 0 else "") + extra
            if self.solve_empties > 0 or self.solve_wld_empties > 0:
                if self.solve_empties > 0:
                    extra += " solve_empties=%d" % self.solve_empties
                if self.solve_wld_empties > 0:
                    extra += " solve_wld_empties=%d" % self.solve_wld_empties
                if self.solve_task_empties is not None:
                    extra += " solve_task_empties=%d" % self.solve_task_empties + (
                        " solve_order=%d" % self.solve_order if self.solve_order > 0 else "") + (
                        " solve_hash_bits=%d" % self.solve_hash_bits if self.solve_hash_bits is not None else "")
            out("%s policy=%s%s" % (self.name, self.policy, extra))
        elif cmd == "verbose 1":
            b = self.board
            text = str(b).rstrip("\n").split("\n")[:12]
            text += [""] * (12 - len(text))
            if self.nodes is not None and self.reached is not None:
                text[11] = (text[11] + " " if text[11] else "") + "depth=%d" % self.reached
            won = ""
            if b.is_game_over() and b.n_black() != b.n_white():
                won = "Black won" if b.n_black() > b.n_white() else "White won"
            for t in text + [won]:
                out(t)
            self._shown = True
        elif cmd == "verbose 0":
            if self._shown:
                out("Game Over" if self.board.is_game_over() else "")
            self._shown = False
        elif cmd.startswith("verbose"):
            self._shown = False
        elif cmd == "quit":
            out("bye")
            return False
        elif cmd:
            mv = cmd.split()[-1]
            self._put(mv)
            out("")
            out("%s play %s" % (self.name, mv))
            out("")
        return True


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--name", default="GPU")
    p.add_argument("--policy", choices=["random", "greedy", "eval", "search", "mcts"], default="greedy")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--params", default=None, help="eval table in the paramgen.py file format (policies eval and search)")
    p.add_argument("--depth", type=int, default=1, metavar="D", help="plies policy search looks ahead (1..8, with --split S 1..8+S)")
    p.add_argument("--nodes", type=int, default=None, metavar="B",
                   help="policy search by node budget: every go deepens until B nodes are spent, --depth is the cap")
    p.add_argument("--split", type=int, default=0, metavar="S",
                   help="spread policy search's tree over the device: its top S plies become tasks (0 = off, max 4)")
    p.add_argument("--order", type=int, choices=[0, 1], default=0,
                   help="policy search's move ordering: 0 lowest square first, 1 ordered (same moves, smaller tree)")
    p.add_argument("--solve-empties", type=int, default=0, metavar="K",
                   help="play the exact solver's move once at most K squares are empty (0 = never, max 12; "
                        "max 16 with --solve-task-empties)")
    p.add_argument("--solve-task-empties", type=int, default=None, metavar="T",
                   help="spread the exact solver's tree over the device: nodes of at most T empties become tasks (1..12)")
    p.add_argument("--solve-order", type=int, choices=[0, 1], default=None,
                   help="move ordering inside the split solver's tasks (default: --order's value)")
    p.add_argument("--solve-hash-bits", type=int, default=None, metavar="B",
                   help="give the split solver's tasks a transposition table of 2**B entries, kept between moves "
                        "(4..26; needs --solve-task-empties)")
    p.add_argument("--solve-wld-empties", type=int, default=0, metavar="W",
                   help="with more than K and at most W empty squares, solve for win / draw / loss and play the proved "
                        "winning or drawing move (0 = never; W > K, max 12, max 16 with --solve-task-empties)")
    p.add_argument("--iterations", type=int, default=None, metavar="T",
                   help="policy mcts: iterations of 64 random playouts per go (1..65536)")
    p.add_argument("--explore", type=float, default=0.5, metavar="C", help="policy mcts: UCT's exploration constant")
    p.add_argument("--reuse", type=int, default=0, choices=[0, 1],
                   help="policy mcts: 1 keeps the search tree between moves, re-rooted on every move played")
    p.add_argument("--leaves", type=int, default=None, metavar="L",
                   help="policy mcts: the wide search, --iterations rounds of L leaves each, a block of L waves (1..16)")
    a = p.parse_args(argv)
    if a.policy != "mcts" and a.reuse:
        p.error("--reuse applies to --policy mcts")
    if a.policy != "mcts" and a.leaves is not None:
        p.error("--leaves applies to --policy mcts")
    if a.leaves is not None and a.reuse:
        p.error("--leaves is not for --reuse 1: the trees that persist have one leaf an iteration")
    if a.policy == "mcts" and a.iterations is None:
        p.error("--policy mcts needs --iterations")
    if a.policy != "mcts" and a.iterations is not None:
        p.error("--iterations applies to --policy mcts")
    if a.solve_hash_bits is not None and a.solve_task_empties is None:
        p.error("--solve-hash-bits needs --solve-task-empties")
    weights = params.read_paramgen(a.params)[1] if a.params else None
    eng = Engine(a.name, a.policy, a.seed, weights, a.solve_empties, a.depth, a.split, a.order,
                 a.solve_task_empties, a.solve_order, a.solve_hash_bits, a.solve_wld_empties, a.nodes, a.iterations,
                 a.explore, a.reuse, a.leaves)

    def out(s):
        sys.stdout.write(s + "\n")
        sys.stdout.flush()

    for line in sys.stdin:
        if not eng.handle(line, out):
            break
    return 0


if __name__ == "__main__":
    sys.exit(main())
