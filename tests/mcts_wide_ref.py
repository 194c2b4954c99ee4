"""The checker of the wide Monte Carlo tree search:
include/othello_mcts_wide.h's rule in Python over oracle.legal, oracle.step and
oracle.rollout, with numpy float32 for the selection score, as tests/mcts_ref.py
is othello_mcts.h's.  The walkers of a round run strictly one after another:
select, expand, mark; then every walker's 64 games; then every back-up.  Test
infrastructure only; it knows nothing of the code under test."""
import numpy as np

import oracle
from mcts_ref import F32, INVALID, MASK64, NO_MOVE, PASS, SEARCHED, _legal, _squares, _Tree, default_nodes, log_table

MAX_LEAVES = 16


def search_one(board, mover, i, R, L, c, seed, game_id0, M, table):
    """One valid root: the tree after R rounds of L walkers."""
    tree = _Tree(board, mover)
    c = F32(c)
    for r in range(R):
        paths = []
        # A. the walkers, in order
        for w in range(L):
            # 1. select, on the words as they stand now
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
            if not tree.cnt[v] and not terminal and (v == 0 or tree.n[v] > 0) and len(tree.n) + cnt <= M:
                tree.first[v], tree.cnt[v] = len(tree.n), cnt
                if legal:
                    sq = _squares(legal)
                    s = oracle.step(np.array([b] * cnt, np.uint64), np.full(cnt, m, np.uint8), np.array(sq, np.uint8))
                    assert (s["ret"] > 0).all()
                    for row in s["boards"]:
                        tree.add((int(row[0]), int(row[1])), 3 - m)
                else:
                    tree.add(b, 3 - m)
                v = tree.first[v]
                path.append(v)
            # 3. mark
            for k in path:
                tree.n[k] += 1
            paths.append(path)
        # B. play out
        sums = []
        for w, path in enumerate(paths):
            b, m = tree.board[path[-1]], tree.mover[path[-1]]
            gid = (game_id0 + ((i * R + r) * L + w) * 64) & MASK64
            g = oracle.rollout(64, seed, game_id0=gid, start=np.array([b] * 64, np.uint64),
                               start_turn=np.full(64, m, np.uint8))
            dp = g["diff"].astype(np.int64) * (-1 if m == 1 else 1)  # from the opponent of the leaf's mover
            sums.append((int(2 * (dp > 0).sum() + (dp == 0).sum()), int(dp.sum())))
        # C. back up
        for path, (W, D) in zip(paths, sums):
            for k in reversed(path):
                tree.s[k] += W
                tree.d[k] += D
                W, D = 128 - W, -D
    return tree


def mcts_wide(boards, turn, R, L, c=0.5, seed=0, game_id0=0, max_nodes=None, table=None):
    """dict(visits, wins, diffs (n, 64); root_wins, root_diffs, best_move, status, nodes (n,)) as int64."""
    assert 1 <= L <= MAX_LEAVES and R >= 1
    boards = np.asarray(boards, np.uint64).reshape(-1, 2)
    n = len(boards)
    M = default_nodes(R * L) if max_nodes is None else max_nodes
    table = log_table(R * L) if table is None else table
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
        tree = search_one((black, white), mover, i, R, L, c, seed, game_id0, M, table)
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
