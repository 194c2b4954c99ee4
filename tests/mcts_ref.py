"""The checker of the Monte Carlo tree search: include/othello_mcts.h's rule in
Python over oracle.legal, oracle.step and oracle.rollout, with numpy float32 for
the selection score (every operation rounded on its own; numpy's float32
division and square root are IEEE).  Test infrastructure only: one root at a
time, a few ms per iteration."""
import numpy as np

import oracle

SEARCHED, INVALID = 1, 2
NO_MOVE, PASS = 255, 64
F32 = np.float32
MASK64 = (1 << 64) - 1


def log_table(T):
    """The table the library is given: ln(max(k, 1)) for k = 0..T, computed in float64 and rounded once."""
    return np.log(np.arange(T + 1, dtype=np.float64).clip(1)).astype(np.float32)


def default_nodes(T):
    return 1 + 16 * T


def _legal(board, mover):
    return int(oracle.legal(np.array([board], np.uint64), np.array([mover], np.uint8))[0])


def _squares(mask):
    return [sq for sq in range(64) if mask >> sq & 1]


class _Tree:
    def __init__(self, board, mover):
        self.board = [tuple(int(x) for x in board)]  # (black, white)
        self.mover = [mover]
        self.n, self.s, self.d = [0], [0], [0]
        self.first, self.cnt = [0], [0]

    def add(self, board, mover):
        self.board.append(board), self.mover.append(mover)
        self.n.append(0), self.s.append(0), self.d.append(0), self.first.append(0), self.cnt.append(0)


def search_one(board, mover, i, T, c, seed, game_id0, M, table):
    """One valid root: (tree, legal mask of the root)."""
    tree = _Tree(board, mover)
    c = F32(c)
    for t in range(T):
        # 1. select
        v, path = 0, [0]
        while tree.cnt[v]:
            kids = range(tree.first[v], tree.first[v] + tree.cnt[v])
            fresh = [k for k in kids if tree.n[k] == 0]
            if fresh:
                v = fresh[0]
            else:
                n_c = np.array([tree.n[k] for k in kids], np.float32)
                mean = np.array([tree.s[k] for k in kids], np.float32) / (F32(128) * n_c)
                score = mean + c * np.sqrt(table[tree.n[v]] / n_c)
                assert score.dtype == np.float32
                v = kids[int(np.argmax(score))]  # the first maximum: a strict >
            path.append(v)
        # 2. expand
        b, m = tree.board[v], tree.mover[v]
        legal = _legal(b, m)
        terminal = legal == 0 and _legal(b, 3 - m) == 0
        cnt = bin(legal).count("1") if legal else (0 if terminal else 1)
        if not terminal and (v == 0 or tree.n[v] > 0) and len(tree.n) + cnt <= M:
            tree.first[v], tree.cnt[v] = len(tree.n), cnt
            if legal:
                sq = _squares(legal)
                r = oracle.step(np.array([b] * cnt, np.uint64), np.full(cnt, m, np.uint8), np.array(sq, np.uint8))
                assert (r["ret"] > 0).all()
                for row in r["boards"]:
                    tree.add((int(row[0]), int(row[1])), 3 - m)
            else:
                tree.add(b, 3 - m)
            v = tree.first[v]
            path.append(v)
        # 3. play out
        b, m = tree.board[v], tree.mover[v]
        gid = (game_id0 + (i * T + t) * 64) & MASK64
        g = oracle.rollout(64, seed, game_id0=gid, start=np.array([b] * 64, np.uint64),
                           start_turn=np.full(64, m, np.uint8))
        dp = g["diff"].astype(np.int64) * (-1 if m == 1 else 1)  # from the opponent of the leaf's mover
        W = int(2 * (dp > 0).sum() + (dp == 0).sum())
        D = int(dp.sum())
        # 4. back up
        for k in reversed(path):
            tree.n[k] += 1
            tree.s[k] += W
            tree.d[k] += D
            W, D = 128 - W, -D
    return tree


def mcts(boards, turn, T, c=0.5, seed=0, game_id0=0, max_nodes=None, table=None):
    """dict(visits, wins, diffs (n, 64); root_wins, root_diffs, best_move, status, nodes (n,)) as int64."""
    boards = np.asarray(boards, np.uint64).reshape(-1, 2)
    n = len(boards)
    M = default_nodes(T) if max_nodes is None else max_nodes
    table = log_table(T) if table is None else table
    out = dict(visits=np.zeros((n, 64), np.int64), wins=np.zeros((n, 64), np.int64), diffs=np.zeros((n, 64), np.int64),
               root_wins=np.zeros(n, np.int64), root_diffs=np.zeros(n, np.int64),
               best_move=np.full(n, NO_MOVE, np.int64), status=np.full(n, SEARCHED, np.int64),
               nodes=np.zeros(n, np.int64))
    for i in range(n):
        black, white = int(boards[i, 0]), int(boards[i, 1])
        if black & white:
            out["status"][i] = INVALID
            continue
        mover = 2 if int(turn[i]) == 2 else 1
        tree = search_one((black, white), mover, i, T, c, seed, game_id0, M, table)
        legal = _legal((black, white), mover)
        if tree.cnt[0] and legal:
            for k, sq in enumerate(_squares(legal)):
                kid = tree.first[0] + k
                out["visits"][i, sq], out["wins"][i, sq], out["diffs"][i, sq] = tree.n[kid], tree.s[kid], tree.d[kid]
        out["root_wins"][i] = 128 * tree.n[0] - tree.s[0]
        out["root_diffs"][i] = -tree.d[0]
        out["nodes"][i] = len(tree.n)
        if legal:
            out["best_move"][i] = max(_squares(legal), key=lambda sq: (out["visits"][i, sq], out["wins"][i, sq], -sq))
        elif _legal((black, white), 3 - mover):
            out["best_move"][i] = PASS
    return out
