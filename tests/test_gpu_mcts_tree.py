"""ops.MctsTrees / othr_* and ops.mcts_play on the GPU
(include/othello_mcts_tree.h): a search that is resumed equals
ops.mcts; a re-rooted tree equals tests/mcts_tree_ref.py's checker, rows and
whole tree; a tree advanced without keeping equals ops.mcts on the child; the
refused moves leave every byte; and the self-play loop above them plays the
games of a host loop over ops.mcts (no reuse) and of the checker (reuse).  All
comparisons are exact."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcts_cases
import mcts_ref
import mcts_tree_cases as cases
import mcts_tree_ref as ref
import oracle

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402
from subproc_amd.books import GameBooks  # noqa: E402
from subproc_amd.codec import handstr_from_coord, move_str  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

SEED, ID0 = mcts_cases.SEED, mcts_cases.GAME_ID0
READY, INVALID, BADMOVE, KEEP = _lib.MCTS_TREE_READY, _lib.MCTS_TREE_INVALID, _lib.MCTS_TREE_BADMOVE, 255
M40 = mcts_ref.default_nodes(40)


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def u8(x):
    return torch.tensor([int(v) for v in x], dtype=torch.uint8, device="cuda")


def ids_of(ids):
    return torch.from_numpy(np.array([int(i) & (2**64 - 1) for i in ids], np.uint64).view(np.int64)).cuda()


def make(boards, turn, M, ids):
    """Trees on the positions, every byte of theirs defined (so that whole slabs can be compared)."""
    trees = ops.MctsTrees(len(turn), M)
    trees.slabs.zero_()
    trees.init(*dev(boards, turn), id_base=ids_of(ids))
    return trees


def unpack(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.int64) for k, v in r._asdict().items()}


def state(trees):
    torch.cuda.synchronize()
    return trees.slabs.clone(), trees.records.clone()


def same_state(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def small_ids(n, T=40):
    return [ID0 + i * T * 64 for i in range(n)]


# ---- 1. resume ----
@pytest.mark.parametrize("name,M", [("small", None), ("long", 24)])
def test_a_search_in_parts_is_ops_mcts_on_every_field(name, M):
    b, t = mcts_cases.inputs(name)
    T, c = 40, 0.5
    M = M40 if M is None else M
    want = unpack(ops.mcts(*dev(b, t), T, explore=c, seed=SEED, game_id0=ID0, max_nodes=M, want_nodes=True))
    if name == "small":  # (and ops.mcts is what the checker says)
        mcts_cases.same(want, mcts_cases.reference("small", T, c, M), "ops.mcts")
    for parts in ((40,), (1, 39), (17, 23)):
        trees = make(b, t, M, small_ids(len(t)))
        ran = []
        for p in parts:
            r = unpack(trees.search(p, explore=c, seed=SEED))
            ran.append(r["ran"])
        for k in mcts_cases.FIELDS:
            assert (r[k] == want[k]).all(), (name, parts, k)
        ok = want["status"] == _lib.MCTS_SEARCHED
        assert (np.sum(ran, 0)[ok] == T).all() and (np.sum(ran, 0)[~ok] == 0).all()
        assert (r["root_boards"][ok].astype(np.uint64) == b[ok]).all()
        assert (r["root_turn"][ok] == np.where(t[ok] == 2, 2, 1)).all()
        rows = unpack(trees.rows())
        for k in mcts_cases.FIELDS:
            assert (rows[k] == want[k]).all(), (name, parts, "rows", k)
        assert not rows["ran"].any()
    if name == "long":  # trees that ran out of room: the no-expansion branch
        roomy = unpack(ops.mcts(*dev(b, t), T, explore=c, seed=SEED, game_id0=ID0, want_nodes=True))
        assert (want["nodes"] <= 24).all() and (roomy["nodes"] > 24).all()


# ---- 2. re-root ----
def exported(trees):
    return [trees.export(i)["tree"] for i in range(trees.n)]


def same_trees(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, i, len(g), len(w))
        for j, (x, y) in enumerate(zip(g, w)):
            assert x == y, (what, i, j, x, y)


def run_session(b, t, ids, M, Ta, Tb, want, what):
    """init, search Ta, advance by the checker's moves (keeping), search Tb: rows and whole trees at every stage."""
    (r1, t1), (r2, t2), (r3, t3) = want["stages"]
    trees = make(b, t, M, ids)
    cases.same_rows(unpack(trees.search(Ta, explore=cases.C, seed=SEED)), r1, (what, "first search"))
    same_trees(exported(trees), t1, (what, "first search"))
    st = trees.advance(u8(want["moves"]), keep=True)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == want["status"], what
    got = unpack(trees.rows())
    cases.same_rows(got, r2, (what, "advance"))
    same_trees(exported(trees), t2, (what, "advance"))
    assert got["nodes"].tolist() == [len(x) for x in t2]  # the subtree's size: the room is free again
    assert [trees.export(i)["nodes"] for i in range(trees.n)] == [len(x) for x in t2]
    cases.same_rows(unpack(trees.search(Tb, explore=cases.C, seed=SEED)), r3, (what, "second search"))
    same_trees(exported(trees), t3, (what, "second search"))
    return trees


@pytest.mark.parametrize("how", ["best", "second", "unvisited"])
def test_a_re_rooted_wide_tree_is_the_checkers(how):
    b, t = mcts_cases.inputs("small")
    lo, hi = cases.WIDE
    want = cases.reroot(how)
    first = want["stages"][0][0]
    assert all((r["visits"] > 0).sum() == cases.WIDE_T1 and (r["visits"] <= 1).all() for r in first)  # wide: 32+ moves
    if how == "unvisited":
        assert all(r["visits"][m] == 0 for r, m in zip(first, want["moves"]))
    elif how == "second":
        assert all(r["visits"][m] > 0 and m != r["best_move"] for r, m in zip(first, want["moves"]))
    run_session(b[lo:hi], t[lo:hi], [cases.id_base(i) for i in range(lo, hi)], M40, cases.WIDE_T1, cases.WIDE_T2, want,
                ("wide", how))


@pytest.mark.parametrize("M", [M40, 24])
@pytest.mark.parametrize("how", ["best", "last"])
def test_the_host_tests_session_on_the_gpu(M, how):
    """tests/test_mcts_tree_host.py's session (deep subtrees; with M = 24 trees that are full before the re-root)."""
    b, t = mcts_cases.inputs("small")
    trees = run_session(b, t, [cases.id_base(i) for i in range(len(t))], M, cases.T1, cases.T2, cases.session(M, how),
                        ("session", M, how))
    played = [trees.export(i)["played"] for i in range(trees.n)]
    assert played == [cases.T1 + cases.T2] * (trees.n - 1) + [0]  # (the overlap ran nothing)


# ---- 3. a fresh tree ----
def test_advance_without_keeping_then_search_is_ops_mcts_on_the_child():
    b, t = mcts_cases.inputs("small")
    n, T1, T2, X = len(t), 17, 23, 1 << 33
    trees = make(b, t, M40, [X + i * T2 * 64 for i in range(n)])  # (so that the children are one ops.mcts batch)
    first = unpack(trees.search(T1, explore=0.5, seed=SEED))
    st = trees.advance(u8(first["best_move"]), keep=False)
    child = unpack(trees.rows())
    moved = (first["best_move"] != KEEP) & (first["status"] == READY)
    assert moved.sum() >= 25 and (st.cpu().numpy()[moved] == READY).all()
    assert (child["nodes"][moved] == 1).all() and not child["visits"][moved].any()
    assert (child["root_turn"][moved] == 3 - first["root_turn"][moved]).all()
    cb = torch.from_numpy(child["root_boards"]).cuda()
    ct = torch.from_numpy(child["root_turn"].astype(np.uint8)).cuda()
    got = unpack(trees.search(T2, explore=0.5, seed=SEED))
    want = unpack(ops.mcts(cb, ct, T2, explore=0.5, seed=SEED, game_id0=X + T1 * 64, max_nodes=M40, want_nodes=True))
    for k in mcts_cases.FIELDS:
        assert (got[k][moved] == want[k][moved]).all(), k
    for i in np.flatnonzero(moved)[[0, 10, -1]].tolist():  # and row by row, with the tree's own id: id_base + played * 64
        e = trees.export(i)
        assert e["played"] == T1 + T2 and e["id_base"] == X + i * T2 * 64
        one = unpack(ops.mcts(cb[i:i + 1], ct[i:i + 1], T2, explore=0.5, seed=SEED,
                              game_id0=e["id_base"] + T1 * 64, max_nodes=M40, want_nodes=True))
        for k in mcts_cases.FIELDS:
            assert (got[k][i] == one[k][0]).all(), (i, k)
    # the steps through the oracle: the child is the position after the move
    o = oracle.step(b[moved], t[moved], first["best_move"][moved].astype(np.uint8))
    assert (o["boards"] == child["root_boards"][moved].astype(np.uint64)).all()


# ---- 4. edges ----
def test_refused_moves_leave_every_byte_and_the_other_edges():
    b, t = mcts_cases.inputs("small")
    n = len(t)
    (T, c, M), = mcts_cases.runs("small")
    base = mcts_cases.reference("small", T, c, M)
    must_pass = np.flatnonzero(base["best_move"] == 64)
    over = np.flatnonzero((base["best_move"] == 255) & (base["status"] == 1))
    playing = np.flatnonzero(base["best_move"] < 64)
    assert len(must_pass) and len(over) and len(playing) > 15 and base["status"][-1] == INVALID
    legal = oracle.legal(b, t)
    occupied = b[:, 0] | b[:, 1]
    trees = make(b, t, M, small_ids(n))
    trees.search(9, seed=SEED)
    before = state(trees)
    rows = unpack(trees.rows())

    def refused(moves, who):
        st = trees.advance(u8(moves), keep=True).cpu().numpy()
        assert (st[who] == BADMOVE).all() and st[-1] == INVALID
        assert same_state(state(trees), before)
        st = trees.advance(u8(moves), keep=False).cpu().numpy()
        assert (st[who] == BADMOVE).all() and same_state(state(trees), before)

    first_bit = [next((s for s in range(64) if int(m) >> s & 1), KEEP) for m in occupied]
    refused(first_bit, np.concatenate([playing, must_pass, over[occupied[over] != 0]]))  # an occupied square
    dead = [next((s for s in range(64) if not int(o | m) >> s & 1), KEEP) for o, m in zip(occupied, legal)]
    who = np.array([i for i in range(n - 1) if dead[i] != KEEP])
    assert len(who) > 15
    refused(dead, who)  # an empty square that flips nothing
    refused([64 if i in playing or i in over else KEEP for i in range(n)], np.concatenate([playing, over]))
    refused([65 if i < n - 1 else KEEP for i in range(n)], np.arange(n - 1))  # no move code at all
    refused([int(base["best_move"][playing[0]]) if i in over else KEEP for i in range(n)], over)  # a finished game
    st = trees.advance(u8([KEEP] * n)).cpu().numpy()
    assert (st[:-1] == READY).all() and st[-1] == INVALID and same_state(state(trees), before)
    # the pass: the same discs, the other mover, a kept subtree
    st = trees.advance(u8([64 if i in must_pass else KEEP for i in range(n)])).cpu().numpy()
    assert (st[:-1] == READY).all()
    after = unpack(trees.rows())
    assert (after["root_boards"][must_pass] == rows["root_boards"][must_pass]).all()
    assert (after["root_turn"][must_pass] == 3 - rows["root_turn"][must_pass]).all()
    assert (after["root_wins"][must_pass] == 128 * 9 - rows["root_wins"][must_pass]).all()  # the child's 9 visits
    assert (after["nodes"][must_pass] == rows["nodes"][must_pass] - 1).all()
    others = np.setdiff1d(np.arange(n), must_pass)
    assert all((after[k][others] == rows[k][others]).all() for k in mcts_cases.FIELDS)
    # the overlap stays INVALID through everything, all rows 0
    for r in (rows, after, unpack(trees.search(5, seed=SEED))):
        assert r["status"][-1] == INVALID and r["best_move"][-1] == 255 and r["ran"][-1] == 0
        assert not any(r[k][-1].any() for k in ("visits", "wins", "diffs", "root_wins", "root_diffs", "nodes"))
    # a root that cannot expand (max_nodes = 1) advances to a fresh root
    one = make(b, t, 1, small_ids(n))
    r = unpack(one.search(6, seed=SEED))
    assert (r["nodes"][:-1] == 1).all() and not r["visits"].any() and (r["best_move"][playing] < 64).all()
    assert (r["root_wins"][playing] > 0).any()
    st = one.advance(u8(r["best_move"]), keep=True).cpu().numpy()
    a = unpack(one.rows())
    assert (st[playing] == READY).all() and (a["nodes"][playing] == 1).all() and not a["root_wins"][playing].any()
    o = oracle.step(b[playing], t[playing], r["best_move"][playing].astype(np.uint8))
    assert (o["boards"] == a["root_boards"][playing].astype(np.uint64)).all()


# ---- 5. per-tree iterations ----
def test_an_iteration_count_per_tree_is_the_single_calls():
    b, t = mcts_cases.inputs("small")
    n = len(t)
    counts = np.array([0, 1, 7, 40] * n)[:n]
    ids = small_ids(n)
    alone = {}
    for T in (1, 7, 40):
        tr = make(b, t, M40, ids)
        alone[T] = (unpack(tr.search(T, seed=SEED)), state(tr))
    trees = make(b, t, M40, ids)
    fresh = state(trees)
    r = unpack(trees.search(torch.from_numpy(counts.astype(np.int32)).cuda(), seed=SEED))
    mine = state(trees)
    ok = r["status"] == READY
    assert (r["ran"][ok] == counts[ok]).all() and not r["ran"][~ok].any()
    for i in range(n):
        T = int(counts[i])
        if T == 0:  # untouched, byte for byte
            assert torch.equal(mine[0][i], fresh[0][i]) and torch.equal(mine[1][i], fresh[1][i])
            assert r["ran"][i] == 0 and not r["visits"][i].any()
            continue
        want, (slabs, records) = alone[T]
        for k in want:
            assert (r[k][i] == want[k][i]).all(), (i, k)
        assert torch.equal(mine[0][i], slabs[i]) and torch.equal(mine[1][i], records[i])


# ---- 6. the visit cap ----
def test_a_root_never_passes_65536_visits():
    import solve_cases

    cs = solve_cases.cases()[2]  # two empties: short playouts
    i = int(np.flatnonzero(oracle.legal(cs["boards"], cs["turn"]))[0])  # (a root with a move of its own)
    b, t = cs["boards"][i:i + 1], cs["turn"][i:i + 1]
    trees = make(b, t, 64, [ID0])
    r = unpack(trees.search(65530, seed=SEED))
    assert r["ran"][0] == 65530
    r = unpack(trees.search(10, seed=SEED))
    assert r["ran"][0] == 6
    full = state(trees)
    want = unpack(ops.mcts(*dev(b, t), 65536, seed=SEED, game_id0=ID0, max_nodes=64, want_nodes=True))
    for k in mcts_cases.FIELDS:
        assert (r[k] == want[k]).all(), k
    assert r["visits"].sum() == 65536 and trees.export(0)["played"] == 65536
    r = unpack(trees.search(10, seed=SEED))
    assert r["ran"][0] == 0 and same_state(state(trees), full)


# ---- 7. determinism ----
def session_bytes(b, t, ids, M):
    trees = make(b, t, M, ids)
    r = trees.search(17, seed=SEED)
    trees.advance(r.best_move, keep=True)
    out = unpack(trees.search(23, seed=SEED))
    return trees, out, state(trees)


def test_the_grid_the_run_and_a_captured_graph_give_the_same_bytes(monkeypatch):
    b, t = mcts_cases.inputs("small")
    n = len(t)
    ids = [cases.id_base(i) for i in range(n)]
    _, out, eager = session_bytes(b, t, ids, M40)
    cases.same_rows(out, cases.session(M40, "best")["stages"][2][0], "eager")
    _, out2, again = session_bytes(b, t, ids, M40)
    assert same_state(again, eager)
    monkeypatch.setenv("OTH_MCTS_BLOCKS", "3")
    assert _lib.load().othr_trees_grid(n) == 3  # each wave walks about 14 trees
    _, out3, three = session_bytes(b, t, ids, M40)
    monkeypatch.delenv("OTH_MCTS_BLOCKS")
    assert _lib.load().othr_trees_grid(n) == n
    assert same_state(three, eager) and all((out3[k] == out[k]).all() for k in out)
    # search + advance + search as one graph: a replay from the initialised trees gives the eager bytes
    trees = make(b, t, M40, ids)
    bt, tt = dev(b, t)
    idt = ids_of(ids)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        r = trees.search(17, seed=SEED)
        trees.advance(r.best_move, keep=True)
        r = trees.search(23, seed=SEED)
    for _ in range(2):
        trees.slabs.zero_()
        trees.init(bt, tt, id_base=idt)
        g.replay()
        assert same_state(state(trees), eager)
        got = unpack(r)
        assert all((got[k] == out[k]).all() for k in out)


# ---- 8. self-play ----
def replayed(start, start_turn, moves):
    """The oracle's game from the recorded moves: (final board, diff, plies), every move legal."""
    board, turn = np.array(start, np.uint64).reshape(1, 2), np.array([start_turn], np.uint8)
    for mv in moves:
        r = oracle.step(board, turn, np.array([mv], np.uint8))
        assert r["ret"][0] >= 0, (mv, board)
        board, turn = r["boards"], r["turn"]
    assert oracle.legal(board, turn)[0] == 0 and oracle.legal(board, (3 - turn).astype(np.uint8))[0] == 0
    bl, wh = int(board[0, 0]), int(board[0, 1])
    return (bl, wh), bin(bl).count("1") - bin(wh).count("1"), len(moves)


def endgame_starts(k=6):
    """k starts with 10 empty squares.  oracle.sample_midgame's positions are 10 to 49 plies from the opening, so
    none has fewer than 11 empties: the k with the fewest are played on, the lowest legal square each ply, until
    10 are left."""
    g = oracle.sample_midgame(512, 0x5EED)
    empties = np.array([64 - bin(int(x[0] | x[1])).count("1") for x in g["boards"]])
    boards, turns = [], []
    for i in np.argsort(empties, kind="stable"):
        board, turn = g["boards"][i:i + 1].copy(), g["turn"][i:i + 1].copy()
        while 64 - bin(int(board[0, 0] | board[0, 1])).count("1") > 10:
            legal = int(oracle.legal(board, turn)[0])
            if not legal and not int(oracle.legal(board, (3 - turn).astype(np.uint8))[0]):
                break
            r = oracle.step(board, turn, np.array([(legal & -legal).bit_length() - 1 if legal else 64], np.uint8))
            board, turn = r["boards"], r["turn"]
        else:
            boards.append(board[0]), turns.append(turn[0])
        if len(boards) == k:
            break
    assert len(boards) == k
    return np.array(boards, np.uint64), np.array(turns, np.uint8)


PLAY = dict(iterations=(12, 20), explore=(0.5, 1.0))
A_BLACK = [1, 1, 0, 0, 1, 0]


def check_games(r, sb, st, games):
    torch.cuda.synchronize()
    moves, plies = r.moves.cpu().numpy(), r.plies.cpu().numpy()
    fb, diff = ops.to_numpy_u64(r.final_boards), r.diff.cpu().numpy()
    for i, (mv, board, d, p) in enumerate(games):
        assert moves[i, :p].tolist() == list(mv) and (moves[i, p:] == 255).all() and plies[i] == p, (i, mv, moves[i])
        final, od, op = replayed(sb[i], st[i], mv)
        assert (int(fb[i, 0]), int(fb[i, 1])) == final == tuple(board) and diff[i] == od == d and op == p
    assert (r.status.cpu().numpy() == READY).all() and r.a_black.cpu().tolist() == A_BLACK
    h = r.hist.cpu().numpy()
    assert h[:129].sum() == len(games) and h[129:132].sum() == len(games) and h[132] == plies.sum()
    books = GameBooks.from_rollout(r, *dev(sb, st))
    assert books.n == len(games) and len(books.lines(0)) == plies[0] + 1


def test_self_play_without_reuse_is_the_host_loop_over_ops_mcts():
    sb, st = endgame_starts()
    (Ta, Tb), (ca, cb) = PLAY["iterations"], PLAY["explore"]
    M = 1 + 16 * 20
    r = ops.mcts_play(6, SEED, game_id0=ID0, reuse=False, a_black=u8(A_BLACK), start=dev(sb, st)[0],
                      start_turn=dev(sb, st)[1], record_moves=True, **PLAY)
    games, visits = [], []
    for i in range(6):
        board, turn = dev(sb[i:i + 1], st[i:i + 1])
        played, moves, seen = [0, 0], [], 0
        while True:
            p = 0 if (int(turn[0]) == 1) == bool(A_BLACK[i]) else 1
            T, c = ((Ta, ca), (Tb, cb))[p]
            m = ops.mcts(board, turn, T, explore=c, seed=SEED, max_nodes=M,
                         game_id0=ID0 + ((2 * i + p) << 32) + played[p] * 64)
            played[p] += T
            seen += int(m.visits.sum())
            mv = int(m.best_move.cpu()[0])
            if mv == 255:
                break
            moves.append(mv)
            s = ops.step(board, turn, m.best_move)
            assert int(s.ret.cpu()[0]) >= 0
            board, turn = s.boards, s.turn
        bl, wh = (int(x) for x in ops.to_numpy_u64(board)[0])
        games.append((moves, (bl, wh), bin(bl).count("1") - bin(wh).count("1"), len(moves)))
        visits.append(seen)
    check_games(r, sb, st, games)
    assert r.root_visits.cpu().tolist() == visits  # a fresh root has its own search's visits, no more


def test_self_play_with_reuse_is_the_checkers_game_loop():
    sb, st = endgame_starts()
    r = ops.mcts_play(6, SEED, game_id0=ID0, reuse=True, a_black=u8(A_BLACK), start=dev(sb, st)[0],
                      start_turn=dev(sb, st)[1], record_moves=True, **PLAY)
    games = ref.play([tuple(int(x) for x in row) for row in sb], st.tolist(), A_BLACK, PLAY["iterations"],
                     PLAY["explore"], SEED, ID0, 1 + 16 * 20, cases.TABLE, True)
    check_games(r, sb, st, games)
    plain = ops.mcts_play(6, SEED, game_id0=ID0, reuse=False, a_black=u8(A_BLACK), start=dev(sb, st)[0],
                          start_turn=dev(sb, st)[1], **PLAY)
    torch.cuda.synchronize()
    assert plain.moves is None
    # the kept playouts: the roots had more visits when they chose than the iterations of their own searches
    assert int(r.root_visits.sum()) > int(plain.root_visits.sum()) > 0
    # polling the end every 4 plies plays the same games
    rare = ops.mcts_play(6, SEED, game_id0=ID0, reuse=True, a_black=u8(A_BLACK), start=dev(sb, st)[0],
                         start_turn=dev(sb, st)[1], record_moves=True, poll=4, **PLAY)
    torch.cuda.synchronize()
    for x, y in zip(rare, r):
        assert torch.equal(x, y)


def test_256_games_from_the_opening_end_with_legal_moves():
    hist = torch.zeros(_lib.HIST_BINS, dtype=torch.int64, device="cuda")
    r = ops.mcts_play(256, 7, iterations=8, record_moves=True, hist=hist)
    torch.cuda.synchronize()
    assert r.hist is hist and int(hist[:129].sum()) == 256 and int(hist[129:132].sum()) == 256
    assert r.a_black.cpu().tolist() == [1, 0] * 128  # colours alternate, A Black in game 0
    assert (r.status.cpu().numpy() == READY).all()
    moves, plies = r.moves.cpu().numpy(), r.plies.cpu().numpy().astype(np.int64)
    assert (plies >= 9).all() and int(hist[132]) == plies.sum()
    board = np.tile(ops.to_numpy_u64(ops.reset(1)[0]), (256, 1))
    turn = np.ones(256, np.uint8)
    for p in range(int(plies.max())):
        live = np.flatnonzero(plies > p)
        assert (moves[live, p] <= 64).all() and (moves[plies <= p, p] == 255).all()
        s = oracle.step(board[live], turn[live], moves[live, p])
        assert (s["ret"] >= 0).all(), p  # every recorded move is legal
        board[live], turn[live] = s["boards"], s["turn"]
    assert not oracle.legal(board, turn).any() and not oracle.legal(board, (3 - turn).astype(np.uint8)).any()
    assert (board == ops.to_numpy_u64(r.final_boards)).all()
    diff = np.array([bin(int(x)).count("1") - bin(int(y)).count("1") for x, y in board])
    assert (diff == r.diff.cpu().numpy()).all()
    assert (np.bincount(diff + 64, minlength=129) == hist[:129].cpu().numpy()).all()
    # the thin wrapper: runner.do_matches(policy="mcts") is these games with their books
    from subproc_amd import runner

    m = runner.do_matches({}, n=8, seed=7, policy="mcts", iterations=8)
    assert torch.equal(m.games.moves, r.moves[:8]) and m.books.n == 8
    assert m.meta[0]["hamletparam"] == "Hamlet policy=mcts iterations=8 explore=0.5 reuse=1"
    assert m.meta[0]["proc_a"] == "Hamlet" and m.meta[1]["proc_a"] == "GPU"


def test_vecenv_mcts_trees():
    env = VecEnv(3)
    trees = env.mcts_trees(64, game_id0=5, stride=1 << 20)
    r = trees.search(16, seed=3)
    torch.cuda.synchronize()
    assert (r.visits.sum(dim=1) == 16).all() and (r.status == READY).all() and (r.ran == 16).all()
    assert [trees.export(i)["id_base"] for i in range(3)] == [5, 5 + (1 << 20), 5 + (2 << 20)]
    moves = r.best_move.clone()
    env.step(moves)
    assert (trees.advance(moves) == READY).all()
    r = trees.rows()
    assert torch.equal(r.root_boards, env.boards) and torch.equal(r.root_turn, env.turn)


# ---- 9. the engine ----
def engine_moves(args, script):
    p = subprocess.run([sys.executable, "-m", "subproc_amd.engine", "--policy", "mcts", *args], input=script,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return [ln.split()[-1] for ln in p.stdout.splitlines() if " plays " in ln], p.stdout


def named(sq, turn):
    return ("B" if turn == 1 else "W") + handstr_from_coord(sq & 7, sq >> 3).upper()


def test_the_engine_with_reuse_plays_a_mcts_trees_session_and_without_it_what_it_played():
    T, seed = 24, 11
    # go, go, the opponent's move, go: the session the engine's tree goes through
    env = VecEnv(1)
    trees = env.mcts_trees(1 + 32 * T, game_id0=0)
    want, opp = [], None
    for k in range(4):
        if k == 2:  # the opponent: the lowest legal square
            legal = int(ops.legal(env.boards, env.turn).cpu()[0])
            opp = (legal & -legal).bit_length() - 1
            mv = u8([opp])
        else:
            mv = trees.search(T, seed=seed).best_move.clone()
            want.append(named(int(mv.cpu()[0]), int(env.turn.cpu()[0])))
        assert int(trees.advance(mv).cpu()[0]) == READY
        env.step(mv)
    script = "go\ngo\n%s\ngo\nverbose p\nquit\n" % move_str(opp)
    played, text = engine_moves(["--iterations", str(T), "--seed", str(seed), "--reuse", "1"], script)
    assert played == want
    assert "GPU policy=mcts iterations=24 explore=0.5 reuse=1" in text
    # --reuse 0, and no --reuse at all: one fresh ops.mcts per go with the go's own ids, as ever
    env = VecEnv(1)
    fresh, k = [], 0
    for step in range(4):
        if step == 2:
            mv = u8([opp])
        else:
            mv = ops.mcts(env.boards, env.turn, T, seed=seed, game_id0=k * T * 64).best_move
            fresh.append(named(int(mv.cpu()[0]), int(env.turn.cpu()[0])))
            k += 1
        env.step(mv)
    zero, text0 = engine_moves(["--iterations", str(T), "--seed", str(seed), "--reuse", "0"], script)
    none, text1 = engine_moves(["--iterations", str(T), "--seed", str(seed)], script)
    assert zero == none == fresh and text0 == text1
    assert "GPU policy=mcts iterations=24 explore=0.5\n" in text0
