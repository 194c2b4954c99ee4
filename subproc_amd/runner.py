"""GameRunner matches in batches: the job an ElJemTask performs
(eljem_task.py:9-20 -> subproc.do_match, subproc.py:15-39 -> GameRunner,
game_runner.py:104-201), for n games at once on the GPU.

``do_matches(conf, params, n, seed)`` plays n games between player A -- the
eval policy with ``params`` (the table paramgen writes for the engine,
eljem_task.py:13-16) -- and player B, with the conf keys do_match reads:

  proc_n_rand_hands_for_a / _b   GameRunner's random-move budgets (each capped
                                 at N_RAND_HAND_UNTIL = 10, game_runner.py:115-119)
  proc_randomize_black_white     per game, A plays White with probability 1/2

and returns what the reference's recorder and learner see: the books of every
game (GameBooks: flat-file text and per-ply records), the meta GameRunner
stores with them (``{'proc_a': Black's name, 'proc_b': White's name,
'hamletparam': ...}``, game_runner.py:182-183), the winner tuple play_a_game
returns (194-199), and the batch statistics LearnBasePlus.store_batch_stats
derives from the books (learn_base.py:58-110).

The schedule runs inside the rollout kernel (oth_rollout_runner,
include/othello.h) for the 1-ply policies and inside the self-play kernel
(othp_play, include/othello_play.h) for policy "search", where both players
look ahead; its draws come from each game's counter RNG stream
(DESIGN.md §4), so a batch is reproducible from (seed, game ids) and any
split of the ids over launches or GPUs plays the same games.
"""
from collections import namedtuple

import numpy as np

from . import codec, ops, params, stats
from .books import GameBooks

MatchBatch = namedtuple("MatchBatch", "games books meta won stats a_black")

N_RAND_HAND_UNTIL = 10  # game_runner.py:6


def hamlet_param_line(name, policy, weights, depth=None, solve_empties=0, nodes=None):
    """The 'verbose p' line of the GPU engine (subproc_amd.engine): what
    GameRunner.extract_hamlet_param stores as 'hamletparam' (game_runner.py:124-130).
    For policy "search": the engine's depth before the weights and, if set,
    its solve_empties after them; ``nodes``, the engine's --nodes budget, after
    the depth (None: no budget, the text as it always was)."""
    extra = " weights=%s" % params.as_weights(weights).reshape(-1).tolist() if policy in ("eval", "search") else ""
    if policy == "search":
        extra = " depth=%d" % depth + (" nodes=%d" % nodes if nodes is not None else "") + extra
        if solve_empties > 0:
            extra += " solve_empties=%d" % solve_empties
    return "%s policy=%s%s" % (name, policy, extra)


def do_matches(conf, weights_a=None, n=1, seed=0, game_id0=0, weights_b=None, policy="eval", name_a="Hamlet",
               name_b="GPU", device="cuda", record=True, win_rule="reference", store=None, depth=None,
               exact_empties=0, order=0, budget=None, solve_empties=0, iterations=None, explore=0.5, reuse=True):
    """n GameRunner games between A (``weights_a``) and B (``weights_b``,
    default params.DEFAULT_WEIGHTS), both playing ``policy``: "greedy", "eval",
    or "search" -- every policy move searched ``depth`` plies deep (an int, or
    (A's, B's); 1..8) over the mover's table, exactly from ``exact_empties``
    empty squares on (ops.play: the whole games in one launch; ``order`` = 1: with
    move ordering, the same games from smaller trees).  A "search"
    game that a search's node limit stopped (ops.play's status) raises.
    ``budget`` = B or (A's, B's): the moves are searched by node budget, ``depth``
    being the cap (ops.play(budget=...)); None: fixed depth.
    ``solve_empties`` = E (1..12) in place of ``exact_empties``: from E empty
    squares on the moves are the exact solver's (ops.play(solve_empties=...)),
    as the engine's --solve-empties plays them; the parameter line names it.
    ``policy`` = "mcts": both players are Monte Carlo tree searchers of
    ``iterations`` = T or (A's, B's) iterations per move with ``explore`` = c or
    (A's, B's), each keeping its tree between moves where ``reuse``
    (ops.mcts_play: a launch per step, no eval table; colours alternate, A
    Black in game 0).  The weights and every keyword of the eval searches are
    refused, and so are the conf's random-move budgets and colour draw: random
    opening plies are not part of these games.

    Game i is global id ``game_id0 + i`` (its book id).  ``record=True``
    replays every game into books (the recorder's view); the batch stats are
    computed from the terminal records as learn_books hands them to
    store_batch_stats (``win_rule`` as subproc_amd.stats), and written to
    ``store`` if given.  The reference's engine named 'Hamlet' provides
    'hamletparam'; here player A is that engine."""
    n_rand_a = int(conf.get("proc_n_rand_hands_for_a", 0))
    n_rand_b = int(conf.get("proc_n_rand_hands_for_b", 0))
    swap = int(conf.get("proc_randomize_black_white", 0)) == 1
    wa = params.DEFAULT_WEIGHTS if weights_a is None else weights_a
    wb = params.DEFAULT_WEIGHTS if weights_b is None else weights_b
    if policy != "mcts" and iterations is not None:
        raise ValueError("iterations, explore and reuse apply to policy 'mcts' only")
    if policy == "mcts":
        if iterations is None:
            raise ValueError("policy 'mcts' needs iterations=T or iterations=(Ta, Tb)")
        if (weights_a is not None or weights_b is not None or depth is not None or exact_empties or order
                or budget is not None or solve_empties):
            raise ValueError("weights, depth, exact_empties, order, budget and solve_empties belong to the eval "
                             "searches, not to policy 'mcts'")
        if n_rand_a or n_rand_b or swap:
            raise ValueError("policy 'mcts' plays no random plies and draws no colours: start games through "
                             "ops.mcts_play(start=...)")
        r = ops.mcts_play(n, seed, game_id0, iterations=iterations, explore=explore, reuse=reuse, record_moves=record,
                          device=device)
        (ta, tb), (ca, cb) = ops._mcts_pair("iterations", iterations, 1, 1 << 16, int), ops._mcts_pair(
            "explore", explore, -3.0e38, 3.0e38, float)
        tail = " reuse=1" if reuse else ""
        line = {"a": "%s policy=mcts iterations=%d explore=%g%s" % (name_a, ta, ca, tail),
                "b": "%s policy=mcts iterations=%d explore=%g%s" % (name_b, tb, cb, tail)}
    elif policy == "search":
        if depth is None:
            raise ValueError("policy 'search' needs depth=D or depth=(Da, Db)")
        depth_a, depth_b = (depth, depth) if isinstance(depth, int) else depth
        budget_a, budget_b = (budget, budget) if budget is None or isinstance(budget, int) else budget
        r = ops.play(n, seed, game_id0, wa, wb, depth_a, depth_b, exact_empties, n_rand_a, n_rand_b, swap,
                     record_moves=record, device=device, order=order,
                     budget=None if budget is None else (budget_a, budget_b), solve_empties=solve_empties)
        if not bool((r.status == ops._lib.SEARCH_SEARCHED).all()):
            raise RuntimeError("do_matches: a game's search reached the node limit")
        zone = solve_empties or exact_empties  # (ops.play has refused both)
        line = {"a": hamlet_param_line(name_a, policy, wa, depth_a, zone, budget_a),
                "b": hamlet_param_line(name_b, policy, wb, depth_b, zone, budget_b)}
    else:
        if depth is not None or exact_empties or budget is not None or solve_empties:
            raise ValueError("depth, exact_empties, solve_empties and budget apply to policy 'search' only")
        if order:
            raise ValueError("order applies to policy 'search' only")
        r = ops.rollout_runner(n, seed, game_id0, policy, wa, wb, n_rand_a, n_rand_b, swap, record_moves=record,
                               device=device)
        line = {"a": hamlet_param_line(name_a, policy, wa), "b": hamlet_param_line(name_b, policy, wb)}
    a_black = r.a_black.cpu().numpy().astype(bool)
    # extract_hamlet_param (game_runner.py:124-130): Black's engine first, then
    # White's, per game (the colours follow the swap draw)

    def hamlet(black, white):
        for who, name in (black, white):
            if name == "Hamlet":
                return line[who]
        return "No Hamlet"

    meta = []
    for ab in a_black:
        black, white = (("a", name_a), ("b", name_b)) if ab else (("b", name_b), ("a", name_a))
        meta.append({"proc_a": black[1], "proc_b": white[1], "hamletparam": hamlet(black, white)})
    diff = r.diff.cpu().numpy().astype(int)
    won = [("Black", m["proc_a"]) if d > 0 else (("White", m["proc_b"]) if d < 0 else ("None", ""))
           for d, m in zip(diff, meta)]
    books = GameBooks.from_rollout(r) if record else None
    # the terminal record of each book (book[0] after learn_books' reverse sort,
    # replearn.py:34-39) with its meta: store_batch_stats' input
    fin = ops.to_numpy_u64(r.final_boards).reshape(-1, 2)
    texts = codec.serialize_boards(fin)
    pl = r.plies.cpu().numpy().astype(int)
    side = ["-"] * n
    if books is not None:  # the side to move the recorder wrote with the terminal board
        last = books.pos.row_off + r.plies.long().clamp(max=ops.MOVES_STRIDE)
        side = ["O" if t == 1 else ("X" if t == 2 else "-") for t in books.pos.turn[last].cpu().tolist()]
    terminal = [(game_id0 + i, [{"book": t, "whosturn": side[i], "turn": int(pl[i]), "end": True}], meta[i])
                for i, t in enumerate(texts)]
    st = stats.store_batch_stats(terminal, store=store, win_rule=win_rule, device=device)
    return MatchBatch(r, books, meta, won, st, a_black)


def wins_of_a(batch):
    """Player A's wins / losses / draws over a MatchBatch (by colour and swap)."""
    d = batch.games.diff.cpu().numpy().astype(int)
    sign = np.where(batch.a_black, 1, -1) * np.sign(d)
    return int((sign > 0).sum()), int((sign < 0).sum()), int((sign == 0).sum())
