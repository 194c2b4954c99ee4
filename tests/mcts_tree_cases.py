"""The checker's answers that the tests of the Monte Carlo search trees that
persist share (tests/test_mcts_tree_host.py, tests/test_gpu_mcts_tree.py), over
tests/mcts_cases.py's sets: each is computed once per process by
tests/mcts_tree_ref.py and handed out as it is (do not modify).

    session(M, how)   on `small`: init, search 17, advance(keep) by `how`
                      ("best": the tree's best move; "last": the root mover's
                      last legal square), search 23; the rows and the canonical
                      tree after each of the three
    reroot(how)       on the 4 wide roots: init, search 20, advance(keep) by
                      "best", "second" (the visited move with the fewest visits
                      that is not the best) or "unvisited" (a legal move with 0
                      visits), search 24
"""
import copy
import functools

import numpy as np

import mcts_cases
import mcts_ref
import mcts_tree_ref as ref

SEED, C = mcts_cases.SEED, 0.5
T1, T2 = 17, 23
WIDE_T1, WIDE_T2 = 20, 24
TABLE = ref.log_table()
TABLE.setflags(write=False)


def id_base(i, T=T1 + T2):
    """The ids that make searches summing to T equal othu_mcts at T on mcts_cases' batch."""
    return mcts_cases.GAME_ID0 + i * T * 64


def snapshot(trees, ran=None):
    return ([ref.rows(t, 0 if ran is None else ran[i]) for i, t in enumerate(trees)], [ref.bfs(t) for t in trees])


@functools.lru_cache(maxsize=None)
def _searched(name, lo, hi, T, M):
    b, t = mcts_cases.inputs(name)
    trees = [ref.Tree(b[i], t[i], id_base(i)) for i in range(lo, hi if hi else len(t))]
    ran = [ref.search(tr, T, C, SEED, M, TABLE) for tr in trees]
    return trees, ran


def _moves(trees, how):
    out = []
    for tr in trees:
        if tr.status != ref.READY:
            out.append(ref.KEEP)
            continue
        r = ref.rows(tr)
        legal = [sq for sq in range(64) if mcts_ref._legal(tr.t.board[0], tr.turn) >> sq & 1]
        if how == "best":
            out.append(r["best_move"])
        elif how == "last":
            out.append(ref.last_move(tr))
        elif how == "second":
            seen = [sq for sq in legal if r["visits"][sq] > 0 and sq != r["best_move"]]
            out.append(min(seen, key=lambda sq: (r["visits"][sq], sq)))
        else:
            out.append([sq for sq in legal if r["visits"][sq] == 0][0])
    return out


def _session(name, lo, hi, Ta, Tb, M, how):
    trees, ran = _searched(name, lo, hi, Ta, M)
    first = snapshot(trees, ran)
    trees = copy.deepcopy(trees)
    moves = _moves(trees, how)
    status = [ref.advance(tr, mv, True) for tr, mv in zip(trees, moves)]
    second = snapshot(trees)
    ran = [ref.search(tr, Tb, C, SEED, M, TABLE) for tr in trees]
    return dict(moves=moves, status=status, stages=(first, second, snapshot(trees, ran)))


@functools.lru_cache(maxsize=None)
def session(M, how):
    return _session("small", 0, 0, T1, T2, M, how)


WIDE = (32, 36)  # mcts_cases' `small`: 12 midgame roots, 20 edge roots, then the 4 wide ones


@functools.lru_cache(maxsize=None)
def reroot(how):
    return _session("small", *WIDE, WIDE_T1, WIDE_T2, mcts_ref.default_nodes(40), how)


def same_rows(got, want, what):
    """got: field -> array over the trees; want: the checker's list of rows."""
    for k in ref.FIELDS:
        w = np.array([np.asarray(r[k]).astype(np.int64) for r in want])
        g = np.asarray(got[k]).astype(np.int64).reshape(w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
