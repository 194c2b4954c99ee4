"""The checker of the Monte Carlo search trees that persist:
include/othello_mcts_tree.h's rule in Python, over tests/mcts_ref.py's pieces
(its tree of Python lists, its float32 score, oracle.legal, oracle.step and
oracle.rollout).  It knows nothing of the code under test: a tree is a Python
object, a re-root builds a new one by walking the kept subtree, and the
canonical form (:func:`bfs`) is what any layout of the same tree gives.  Test
infrastructure only: one tree at a time, a few ms per iteration."""
import numpy as np

import mcts_ref
import oracle
from mcts_ref import F32, INVALID, MASK64, NO_MOVE, PASS, _legal, _squares

READY, BADMOVE, KEEP = 1, 8, 255
MAX_ITERATIONS = 65536
FIELDS = ("visits", "wins", "diffs", "root_wins", "root_diffs", "best_move", "status", "nodes", "ran", "root_boards",
          "root_turn")


def log_table(last=MAX_ITERATIONS):
    """ln(max(k, 1)) for k = 0..last in float32: the library's table is last = 65,536."""
    return mcts_ref.log_table(last)


class Tree:
    def __init__(self, board, turn, id_base):
        black, white = (int(x) for x in board)
        self.turn = 2 if int(turn) == 2 else 1
        self.id_base, self.played = int(id_base) & MASK64, 0
        self.status = INVALID if black & white else READY
        self.t = mcts_ref._Tree((black, white), self.turn)

    @property
    def nodes(self):
        return len(self.t.n) if self.status == READY else 0


def search(tree, T, c, seed, M, table):
    """``ran`` more iterations of steps 1 to 4 (mcts_ref.search_one's, with this tree's ids); returns ran."""
    if tree.status != READY:
        return 0
    t = tree.t
    ran = min(int(T), MAX_ITERATIONS - t.n[0])
    c = F32(c)
    for _ in range(ran):
        v, path = 0, [0]
        while t.cnt[v]:
            kids = range(t.first[v], t.first[v] + t.cnt[v])
            fresh = [k for k in kids if t.n[k] == 0]
            if fresh:
                v = fresh[0]
            else:
                n_c = np.array([t.n[k] for k in kids], np.float32)
                mean = np.array([t.s[k] for k in kids], np.float32) / (F32(128) * n_c)
                score = mean + c * np.sqrt(table[t.n[v]] / n_c)
                assert score.dtype == np.float32
                v = kids[int(np.argmax(score))]
            path.append(v)
        b, m = t.board[v], t.mover[v]
        legal = _legal(b, m)
        terminal = legal == 0 and _legal(b, 3 - m) == 0
        cnt = bin(legal).count("1") if legal else (0 if terminal else 1)
        if not terminal and (v == 0 or t.n[v] > 0) and len(t.n) + cnt <= M:
            t.first[v], t.cnt[v] = len(t.n), cnt
            for kid in _children(b, m, legal):
                t.add(kid, 3 - m)
            v = t.first[v]
            path.append(v)
        b, m = t.board[v], t.mover[v]
        gid = (tree.id_base + tree.played * 64) & MASK64
        g = oracle.rollout(64, seed, game_id0=gid, start=np.array([b] * 64, np.uint64),
                           start_turn=np.full(64, m, np.uint8))
        dp = g["diff"].astype(np.int64) * (-1 if m == 1 else 1)
        W, D = int(2 * (dp > 0).sum() + (dp == 0).sum()), int(dp.sum())
        for k in reversed(path):
            t.n[k] += 1
            t.s[k] += W
            t.d[k] += D
            W, D = 128 - W, -D
        tree.played += 1
    return ran


def _children(b, m, legal):
    """The children's boards of (b, mover m) in ascending square order; the pass child where legal == 0."""
    if not legal:
        return [b]
    sq = _squares(legal)
    r = oracle.step(np.array([b] * len(sq), np.uint64), np.full(len(sq), m, np.uint8), np.array(sq, np.uint8))
    assert (r["ret"] > 0).all()
    return [(int(row[0]), int(row[1])) for row in r["boards"]]


def rows(tree, ran=0):
    """The outputs of a search / of rows for one tree, as a dict of ints and int64 arrays."""
    out = dict(visits=np.zeros(64, np.int64), wins=np.zeros(64, np.int64), diffs=np.zeros(64, np.int64), root_wins=0,
               root_diffs=0, best_move=NO_MOVE, status=tree.status, nodes=tree.nodes, ran=ran,
               root_boards=np.zeros(2, np.uint64), root_turn=tree.turn)
    if tree.status != READY:
        return out
    t = tree.t
    b, m = t.board[0], t.mover[0]
    assert m == tree.turn
    out["root_boards"] = np.array(b, np.uint64)
    legal = _legal(b, m)
    if t.cnt[0] and legal:
        for k, sq in enumerate(_squares(legal)):
            kid = t.first[0] + k
            out["visits"][sq], out["wins"][sq], out["diffs"][sq] = t.n[kid], t.s[kid], t.d[kid]
    out["root_wins"], out["root_diffs"] = 128 * t.n[0] - t.s[0], -t.d[0]
    if legal:
        out["best_move"] = max(_squares(legal), key=lambda sq: (out["visits"][sq], out["wins"][sq], -sq))
    elif _legal(b, 3 - m):
        out["best_move"] = PASS
    return out


def last_move(tree):
    """The root mover's last legal square; PASS where it must pass, 255 where the game is over."""
    b, m = tree.t.board[0], tree.t.mover[0]
    legal = _legal(b, m)
    if legal:
        return _squares(legal)[-1]
    return PASS if _legal(b, 3 - m) else NO_MOVE


def advance(tree, move, keep):
    """The status; the tree re-rooted (a new object tree: the kept nodes walked breadth first)."""
    if tree.status != READY:
        return INVALID
    move = int(move)
    if move == KEEP:
        return READY
    t = tree.t
    b, m = t.board[0], t.mover[0]
    legal = _legal(b, m)
    if move < 64:
        if not legal >> move & 1:
            return BADMOVE
        k = _squares(legal).index(move)
    elif move == PASS and legal == 0 and _legal(b, 3 - m):
        k = 0
    else:
        return BADMOVE
    new = mcts_ref._Tree((0, 0), 3 - m)
    if keep and t.cnt[0]:
        order = [t.first[0] + k]
        q = 0
        while q < len(order):
            v = order[q]
            order.extend(range(t.first[v], t.first[v] + t.cnt[v]))
            q += 1
        place = {v: j for j, v in enumerate(order)}
        for j, v in enumerate(order):
            if j:
                new.add(None, None)
            new.board[j], new.mover[j] = t.board[v], t.mover[v]
            new.n[j], new.s[j], new.d[j], new.cnt[j] = t.n[v], t.s[v], t.d[v], t.cnt[v]
            new.first[j] = place[t.first[v]] if t.cnt[v] else 0
    else:
        new.board[0] = _children(b, m, legal)[k]
    tree.t = new
    tree.turn = 3 - tree.turn
    return READY


def bfs(tree):
    """The canonical form: [(P, O, n, s, d, children count)] breadth first from the root."""
    if tree.status != READY:
        return []
    t = tree.t
    order, q, out = [0], 0, []
    while q < len(order):
        v = order[q]
        black, white = t.board[v]
        P, O = (white, black) if t.mover[v] == 2 else (black, white)
        out.append((P, O, t.n[v], t.s[v], t.d[v], t.cnt[v]))
        order.extend(range(t.first[v], t.first[v] + t.cnt[v]))
        q += 1
    assert len(out) == len(t.n)  # every node is reachable
    return out


def play(starts, start_turn, a_black, Ts, cs, seed, game_id0, M, table, reuse):
    """The checker's game loop of ops.mcts_play: per game (moves, final board, diff, plies)."""
    games = []
    for i, (board, turn) in enumerate(zip(starts, start_turn)):
        trees = [Tree(board, turn, game_id0 + ((2 * i + p) << 32)) for p in (0, 1)]
        moves = []
        while True:
            mover = trees[0].turn
            p = 0 if (mover == 1) == bool(a_black[i]) else 1
            search(trees[p], Ts[p], cs[p], seed, M, table)
            mv = rows(trees[p])["best_move"]
            if mv == NO_MOVE:
                break
            moves.append(mv)
            for t in trees:
                assert advance(t, mv, reuse) == READY
        b = trees[0].t.board[0]
        games.append((moves, b, bin(b[0]).count("1") - bin(b[1]).count("1"), len(moves)))
    return games
