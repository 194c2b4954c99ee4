"""The search self-play's checker: include/othello_play.h's game rule as a
plain Python loop over the C oracle's game_key / rng_draw / legal / step, with a
pluggable chooser for the policy moves and no knowledge of the code under test.

Per game, on its counter RNG stream (pick(n) = (draw * n) >> 32):
  * start boards that overlap: INVALID, nothing played, no draw made;
  * with swap, the first draw pick(2) == 1 puts player A on White;
  * budgets min(n_rand, 10) by player; on each turn of a player with budget
    r > 0 -- a pass too, but not once the game is over -- a draw pick(r); 0 with
    a legal move plays puttables[pick(#legal)] and spends one;
  * otherwise: neither side can move: over; no move: pass (a ply); one legal
    move: played; else the chooser's move.

All live games advance one ply per round, so the chooser sees every game's
position of that round in one call: chooser(boards (k, 2) uint64, turn (k,)
uint8, player (k,) 0 = A / 1 = B) -> (k,) move codes.
"""
import numpy as np

import oracle
import search_ref
from solve_ref import empties

PASS = 64
SEARCHED, INVALID, LIMIT = 1, 2, 3
MAX_BUDGET = 10
OPENING = (0x0000000810000000, 0x0000001008000000)


class _Rng:
    def __init__(self, key):
        self.key, self.i = key, 0

    def pick(self, n):
        self.i += 1
        return (int(oracle.rng_draw(self.key, self.i)) * int(n)) >> 32


def _squares(mask):
    mask = int(mask)
    return [s for s in range(64) if mask >> s & 1]


def play(n, seed, chooser, game_id0=0, n_rand_a=0, n_rand_b=0, swap=False, start=None, start_turn=None):
    """dict(a_black, final_boards, diff, plies, moves (n, 128) 255-padded,
    status, hist) of the n games."""
    if start is None:
        boards = np.tile(np.array(OPENING, np.uint64), (n, 1))
        turn = np.ones(n, np.uint8)
    else:
        boards = np.array(start, np.uint64).reshape(n, 2)
        turn = (np.ones(n, np.uint8) if start_turn is None
                else np.where(np.asarray(start_turn, np.uint8) == 2, 2, 1).astype(np.uint8))
    rng = [_Rng(oracle.game_key(seed, game_id0 + i)) for i in range(n)]
    a_black = np.ones(n, np.uint8)
    status = np.full(n, SEARCHED, np.uint8)
    plies = np.zeros(n, np.int64)
    moves = np.full((n, oracle.MOVES_STRIDE), 255, np.uint8)
    rem = np.zeros((n, 3), np.int64)  # by colour: [.., Black, White]
    live = np.ones(n, bool)
    for i in range(n):
        if int(boards[i, 0]) & int(boards[i, 1]):
            status[i], live[i] = INVALID, False
            continue
        if swap and rng[i].pick(2) == 1:
            a_black[i] = 0
        ra, rb = min(n_rand_a, MAX_BUDGET), min(n_rand_b, MAX_BUDGET)
        rem[i, 1], rem[i, 2] = (ra, rb) if a_black[i] else (rb, ra)
    while live.any():
        idx = np.nonzero(live)[0]
        own = oracle.legal(boards[idx], turn[idx])
        opp = oracle.legal(boards[idx], (3 - turn[idx]).astype(np.uint8))
        move = np.full(len(idx), 255, np.int64)
        ask = []
        for k, i in enumerate(idx):
            if own[k] == 0 and opp[k] == 0:
                live[i] = False
                continue
            t = int(turn[i])
            coin = False
            if rem[i, t] > 0 and rng[i].pick(rem[i, t]) == 0 and own[k] != 0:
                coin = True
                rem[i, t] -= 1
            sq = _squares(own[k])
            if not sq:
                move[k] = PASS
            elif coin:
                move[k] = sq[rng[i].pick(len(sq))]
            elif len(sq) == 1:
                move[k] = sq[0]
            else:
                ask.append(k)
        if ask:
            g = idx[ask]
            player = np.where((turn[g] == 1) == (a_black[g] == 1), 0, 1)
            chosen = np.asarray(chooser(boards[g], turn[g], player))
            assert all(int(own[k]) >> int(m) & 1 for k, m in zip(ask, chosen)), "the chooser's move is not legal"
            move[ask] = chosen
        go = move != 255
        g = idx[go]
        if len(g) == 0:
            continue
        st = oracle.step(boards[g], turn[g], move[go].astype(np.uint8))
        assert (st["ret"] >= 0).all()
        boards[g], turn[g] = st["boards"], st["turn"]
        rec = plies[g] < oracle.MOVES_STRIDE
        moves[g[rec], plies[g][rec]] = move[go][rec]
        plies[g] += 1
    played = status == SEARCHED
    nb = np.array([bin(int(v)).count("1") for v in boards[:, 0]], np.int64)
    nw = np.array([bin(int(v)).count("1") for v in boards[:, 1]], np.int64)
    diff = np.where(played, nb - nw, 0)
    return dict(a_black=a_black, final_boards=boards, diff=diff.astype(np.int8), plies=plies.astype(np.uint8),
                moves=moves, status=status, hist=histogram(diff[played], plies[played]))


def histogram(diff, plies):
    """oth_rollout's bins of finished games: [0..128] diff + 64, 129 Black wins,
    130 White wins, 131 draws, 132 total plies."""
    diff = np.asarray(diff, np.int64)
    h = np.zeros(oracle.HIST_BINS, np.int64)
    np.add.at(h, diff + 64, 1)
    h[129], h[130], h[131] = (diff > 0).sum(), (diff < 0).sum(), (diff == 0).sum()
    h[132] = np.asarray(plies, np.int64).sum()
    return h


def search_chooser(weights_a, weights_b, depth_a, depth_b, exact_empties=0):
    """The rule's policy move: search_ref.search's best move with the mover's
    table at the mover's depth, or max(depth, empties) plies once empties <=
    exact_empties; one search call per (player, depth) group."""
    def choose(boards, turn, player):
        emp = empties(boards)
        d = np.where(player == 0, depth_a, depth_b)
        d = np.where(emp <= exact_empties, np.maximum(d, emp), d)
        out = np.full(len(boards), 255, np.uint8)
        for p, w in ((0, weights_a), (1, weights_b)):
            for dd in np.unique(d[player == p]):
                sel = np.nonzero((player == p) & (d == dd))[0]
                out[sel] = search_ref.search(boards[sel], turn[sel], int(dd), w)[1]
        return out
    return choose


def one_ply_chooser(weights_a, weights_b):
    """The 1-ply eval policy: the move whose child maximises the mover's
    oracle.evaluate, the lowest square among equals."""
    def choose(boards, turn, player):
        out = np.empty(len(boards), np.uint8)
        own = oracle.legal(boards, turn)
        for k in range(len(boards)):
            sq = np.array(_squares(own[k]), np.uint8)
            b, t = np.tile(boards[k], (len(sq), 1)), np.full(len(sq), turn[k], np.uint8)
            child = oracle.step(b, t, sq)["boards"]
            ev = oracle.evaluate(child, t, weights_a if player[k] == 0 else weights_b)
            out[k] = sq[int(np.argmax(ev))]  # argmax keeps the first maximiser: the lowest square
        return out
    return choose
