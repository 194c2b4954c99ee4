"""ops.search(split=...) / otht_search on the GPU: every value and move against
the exhaustive checker (tests/search_ref.py) on the cases of tests/tree_cases.py
(midgame roots, depths 9 and 10 beyond the one-lane search, forced passes and
game-overs inside the split plies); value, move and status bit for bit against
the existing kernels (othm_search, oths_solve) on the 4,096 midgame roots and on
full-depth endgames; the tie rule; independence of the grid, the batch and the
slab; the node limit, the work word and the argument checks; the engine."""
import functools
import io
import sys

import numpy as np
import pytest
import torch

import oracle
import search_ref
import solve_cases
import solve_ref
import tree_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, codec, engine, ops  # noqa: E402

SEARCHED, INVALID, LIMIT, NOROOM = _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT, _lib.TREE_NOROOM
T = search_ref.T
FULL = (1 << 64) - 1
NODE_LIMIT = 1 << 22  # per task; the deepest task here (8 plies at 8 empties) stays far below: a defect ends as LIMIT
TABLES = tree_cases.TABLES


def dev(boards, turn):
    return (ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda"),
            torch.from_numpy(np.array(turn, np.uint8)).cuda())


def tree_search(boards, turn, depth, split, weights, node_limit=NODE_LIMIT, **kw):
    b, t = dev(boards, turn)
    r = ops.search(b, t, depth, weights=weights, node_limit=node_limit, split=split, **kw)
    torch.cuda.synchronize()
    return r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy()


def lane_search(boards, turn, depth, weights):
    b, t = dev(boards, turn)
    r = ops.search(b, t, depth, weights=weights, node_limit=1 << 26)
    torch.cuda.synchronize()
    return r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy()


def splits_of(depth):
    return range(1, min(4, depth - 1) + 1)


# ---------------------------------------------------------------- 1. the checker
CHECKER = [(name, table, split) for name, (_, splits, tables) in tree_cases.CASES.items() for table in tables
           for split in splits]


@pytest.mark.parametrize("name,table,split", CHECKER)
def test_matches_the_checker(name, table, split):
    depth = tree_cases.CASES[name][0]
    b, t = tree_cases.inputs(name)
    rv, rm, _ = tree_cases.reference(name, table)
    v, m, s = tree_search(b, t, depth, split, TABLES[table])
    assert (s == SEARCHED).all()
    bad = np.nonzero((v != rv) | (m != rm))[0]
    assert len(bad) == 0, (bad[:8], v[bad[:8]], rv[bad[:8]], m[bad[:8]], rm[bad[:8]])
    assert ops.work_word("cuda").item() == 0


def test_the_checker_cases_are_what_they_claim():
    assert {k: len(tree_cases.inputs(k)[1]) for k in ("mid3", "mid4", "mid5", "deep9a", "deep9b", "deep10")} == {
        "mid3": 64, "mid4": 32, "mid5": 8, "deep9a": 8, "deep9b": 4, "deep10": 2}
    for name, e in (("deep9a", 10), ("deep9b", 11), ("deep10", 11)):
        assert (solve_ref.empties(tree_cases.inputs(name)[0]) == e).all()
        # the horizon is inside the game: small evals, not multiples of T
        rv = tree_cases.reference(name, "default")[0].astype(np.int64)
        assert (np.abs(rv) < T).all() and (rv % T != 0).any()
    b, t = tree_cases.inputs("special3")
    own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
    # (the pool has no game-over root with three or more empties: these are all forced passes; games that end
    # inside the split plies are below them, at depth 9 with 3..9 empties)
    assert (own == 0).all() and (opp != 0).any()
    emp = solve_ref.empties(b)
    assert emp.min() >= 3 and emp.max() <= 9
    rm = tree_cases.reference("special9", "default")[1]
    assert 64 in rm.tolist() and set(rm.tolist()) <= {64, 255}
    rv = tree_cases.reference("special9", "default")[0].astype(np.int64)
    assert (rv % T == 0).all()  # depth 9 reaches the end of every one of them


# ---------------------------------------------------------------- 2. the existing kernels
@pytest.mark.parametrize("table", tree_cases.BOTH)
@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_equals_the_one_lane_search_on_4096_midgame_roots(depth, table):
    g = tree_cases.midgame()
    b, t = g["boards"], g["turn"]
    assert len(t) == 4096
    rv, rm, rs = lane_search(b, t, depth, TABLES[table])
    assert (rs == SEARCHED).all()
    for split in splits_of(depth):
        # (8,192 nodes a root: 1.7 GB of slabs; the deepest level of some roots then does not fit and their tasks
        # start a level higher, which is part of what is compared)
        v, m, s = tree_search(b, t, depth, split, TABLES[table], nodes_per_position=8192)
        assert (s == SEARCHED).all(), split
        assert (v == rv).all() and (m == rm).all(), (split, np.nonzero((v != rv) | (m != rm))[0][:8])


@pytest.mark.parametrize("e,k", [(11, 64), (12, 16)])  # test_gpu_solve.py's counts at these empties
def test_full_depth_is_t_times_the_solver(e, k):
    b, t = solve_cases.ladder(e, k)
    assert len(t) == k and (solve_ref.empties(b) == e).all()
    bt, tt = dev(b, t)
    r = ops.solve(bt, tt, max_empties=e, node_limit=1 << 26)
    assert (r.status.cpu().numpy() == _lib.SOLVE_SOLVED).all()
    sv, sm = r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy()
    for split in (3, 4):
        if e > split + _lib.SEARCH_MAX_DEPTH:  # depth 12 needs split 4: 12 > 3 + 8 is an argument error
            with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
                ops.search(bt, tt, e, split=split)
            continue
        v, m, s = tree_search(b, t, e, split, TABLES["default"])
        assert (s == SEARCHED).all()
        assert (v == T * sv).all() and (m == sm).all(), split


# ---------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("depth,value", [(4, 560), (5, 900), (6, 660)])
def test_the_openings_four_way_tie_keeps_the_lowest_square(depth, value):
    ob, ot = tree_cases.opening_ties()
    assert len(ot) == 16
    rv, rm, rs = lane_search(ob, ot, depth, TABLES["default"])
    assert (rs == SEARCHED).all() and (rv == value).all() and rm[0] == 19
    # the image of a tied root has its own lowest maximiser: more than one move occurs
    assert len(set(rm.tolist())) > 1
    b, t = np.repeat(ob, 64, axis=0), np.repeat(ot, 64)
    for split in (1, 2, 3):
        v, m, s = tree_search(b, t, depth, split, TABLES["default"])
        assert (s == SEARCHED).all() and (v == value).all(), split
        assert (m == np.repeat(rm, 64)).all(), (split, np.nonzero(m != np.repeat(rm, 64))[0][:8])


def test_two_empties_ties_keep_the_lower_square():
    p = solve_cases.pool()[2]
    b, t = p["boards"][:64], p["turn"][:64]
    rv, rm, _ = search_ref.search(b, t, 2, TABLES["default"])
    v, m, s = tree_search(b, t, 2, 1, TABLES["default"])
    assert (s == SEARCHED).all() and (v == rv).all() and (m == rm).all()


# ---------------------------------------------------------------- 4. order independence
MIX_DEPTH, MIX_SPLIT = 4, 2


@functools.lru_cache(maxsize=None)
def mixed():
    """256 roots: the first 128 midgame roots and 128 forced-pass / game-over
    roots, shuffled once, with the one-lane search's depth-4 answers."""
    g = tree_cases.midgame()
    sb, st = tree_cases.inputs("special3")
    some = np.sort(np.random.default_rng(4).permutation(len(st))[:128])
    b = np.concatenate([g["boards"][:128], sb[some]])
    t = np.concatenate([g["turn"][:128], st[some]])
    order = np.random.default_rng(3).permutation(256)
    b, t = np.ascontiguousarray(b[order]), np.ascontiguousarray(t[order])
    v, m, s = lane_search(b, t, MIX_DEPTH, TABLES["default"])
    assert (s == SEARCHED).all()
    return b, t, v, m


def test_one_wave_runs_every_task(monkeypatch):
    b, t, rv, rm = mixed()
    full = tree_search(b, t, MIX_DEPTH, MIX_SPLIT, TABLES["default"])
    lib = _lib.load()
    assert lib.otht_search_grid(1000) == 16
    monkeypatch.setenv("OTH_SEARCH_BLOCKS", "1")
    assert lib.otht_search_grid(1000) == 1
    one = tree_search(b, t, MIX_DEPTH, MIX_SPLIT, TABLES["default"])
    assert ops.work_word("cuda").item() == 0
    for v, m, s in (full, one):
        assert (s == SEARCHED).all() and (v == rv).all() and (m == rm).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n):
    b, t, rv, rm = mixed()
    v, m, s = tree_search(b[:n], t[:n], MIX_DEPTH, MIX_SPLIT, TABLES["default"])
    assert (s == SEARCHED).all() and (v == rv[:n]).all() and (m == rm[:n]).all()
    assert ops.work_word("cuda").item() == 0


def test_the_batch_reversed():
    b, t, rv, rm = mixed()
    v, m, s = tree_search(b[::-1], t[::-1], MIX_DEPTH, MIX_SPLIT, TABLES["default"])
    assert (s == SEARCHED).all() and (v == rv[::-1]).all() and (m == rm[::-1]).all()


def test_the_smallest_slab_on_the_mixed_roots():
    """64 nodes hold two levels of few roots: the tasks start higher, the
    answers are the same (depth 4 leaves at most 3 plies below level 1)."""
    b, t, rv, rm = mixed()
    v, m, s = tree_search(b, t, MIX_DEPTH, 3, TABLES["default"], nodes_per_position=64)
    assert (s == SEARCHED).all() and (v == rv).all() and (m == rm).all()


@pytest.mark.parametrize("split", [2, 3])
def test_no_room_exactly_where_the_frontier_is_deeper_than_eight(split):
    """Depth 10 at 11 empties in 64 nodes: the first level always fits and
    leaves 9 plies, the second fits for some roots only."""
    b, t = solve_cases.ladder(11, 16)
    want = tree_cases.expected_noroom(b, t, 10, split, 64)
    assert 0 < want.sum() < len(t), want.sum()
    assert not tree_cases.expected_noroom(b, t, 10, split, 32768).any()
    big = tree_search(b, t, 10, split, TABLES["default"])
    assert (big[2] == SEARCHED).all()
    v, m, s = tree_search(b, t, 10, split, TABLES["default"], nodes_per_position=64)
    assert (s == np.where(want, NOROOM, SEARCHED)).all(), (s, want)
    assert (v[want] == 0).all() and (m[want] == 255).all()
    assert (v[~want] == big[0][~want]).all() and (m[~want] == big[1][~want]).all()
    # the two roots of the checker's depth-10 case are the first two of these
    rv, rm, _ = tree_cases.reference("deep10", "default")
    assert (big[0][:2] == rv).all() and (big[1][:2] == rm).all()


# ---------------------------------------------------------------- 5. node limit
def test_node_limit_one_ends_every_midgame_root_as_limit():
    """Depth 3, split 1: every task is a root child with two plies to search
    and no lower bound (its alpha comes from nodes an even number of edges up:
    none), so it searches, and its first move and that move's first reply are
    two nodes."""
    b, t = tree_cases.inputs("mid3")
    v, m, s = tree_search(b, t, 3, 1, TABLES["default"], node_limit=1)
    assert (s == LIMIT).all() and (v == 0).all() and (m == 255).all()
    assert ops.work_word("cuda").item() == 0


def test_a_large_limit_searches_the_whole_midgame_set_at_depth_5():
    g = tree_cases.midgame()
    v, m, s = tree_search(g["boards"], g["turn"], 5, 2, TABLES["default"], node_limit=1 << 22,
                          nodes_per_position=8192)
    assert (s == SEARCHED).all()


# ---------------------------------------------------------------- 6. plumbing
def test_work_word_is_shared_with_the_other_launches_and_left_zero():
    b, t, rv, rm = mixed()
    bt, tt = dev(b, t)
    c = solve_cases.cases()[6]
    cb, ct = dev(c["boards"], c["turn"])
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.search(bt, tt, MIX_DEPTH, node_limit=NODE_LIMIT, split=MIX_SPLIT, work=w)
    r2 = ops.search(bt, tt, MIX_DEPTH, node_limit=NODE_LIMIT, split=1, work=w)
    torch.cuda.synchronize()
    assert w.item() == 0
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r3 = ops.search(bt, tt, MIX_DEPTH, node_limit=NODE_LIMIT, split=MIX_SPLIT, want_nodes=True)
    sv = ops.solve(cb, ct, max_empties=6, node_limit=NODE_LIMIT)
    r4 = ops.search(bt, tt, MIX_DEPTH, node_limit=NODE_LIMIT)
    p1 = ops.play(64, seed=5, depth_a=2, depth_b=1, node_limit=NODE_LIMIT)
    r5 = ops.search(bt, tt, MIX_DEPTH, node_limit=NODE_LIMIT, split=3)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    for r in (r1, r2, r3, r4, r5):
        assert (r.status.cpu().numpy() == SEARCHED).all()
        assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()
    assert r1.nodes is None and r3.nodes.dtype == torch.int32 and (r3.nodes.cpu().numpy().view(np.uint32) > 0).any()
    assert (sv.value.cpu().numpy() == c["value"]).all() and (sv.best_move.cpu().numpy() == c["best_move"]).all()
    assert (p1.status.cpu().numpy() == SEARCHED).all()
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)


def raw(lib, bt, tt, depth, split, w8, val, mv, st, nd, scratch, scratch_bytes, npp, work, n):
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    return lib.otht_search(ptr(bt), ptr(tt), depth, split, w8, NODE_LIMIT, ptr(val), ptr(mv), ptr(st), ptr(nd),
                           ptr(scratch), scratch_bytes, npp, ptr(work), n, torch.cuda.current_stream().cuda_stream)


def test_null_outputs_bad_arguments_and_overlap():
    b, t, rv, rm = mixed()
    b, t, rv, rm = b[:40], t[:40], rv[:40], rm[:40]
    bt, tt = dev(b, t)
    n, npp = len(t), 4096
    lib, w8, w = _lib.load(), ops._weights_ptr(None), ops.work_word("cuda")
    size = lib.otht_scratch_bytes(n, npp)
    assert size > 0
    sc = torch.empty(size // 8 + 1, dtype=torch.int64, device="cuda")
    val = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    mv = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    ok = lambda *a, **k: raw(lib, bt, tt, MIX_DEPTH, MIX_SPLIT, w8, *a, **k)  # noqa: E731
    assert ok(None, None, None, None, sc, size, npp, w, n) == 0
    assert ok(val, None, None, None, sc, size, npp, w, n) == 0
    assert ok(None, mv, None, None, sc, size, npp, w, n) == 0
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == rv).all() and (mv.cpu().numpy() == rm).all() and w.item() == 0
    vb = torch.empty(n, dtype=torch.int32, device="cuda")
    assert raw(lib, bt, None, MIX_DEPTH, MIX_SPLIT, w8, vb, None, None, None, sc, size, npp, w, n) == 0  # Black everywhere
    torch.cuda.synchronize()
    assert (vb.cpu().numpy() == lane_search(b, np.ones(n, np.uint8), MIX_DEPTH, TABLES["default"])[0]).all()
    E = _lib.OTH_EINVAL
    args = (val, None, None, None)
    for depth, split in ((4, 0), (4, 5), (4, -1), (4, 4), (2, 3), (10, 1), (13, 4), (0, 1)):
        assert raw(lib, bt, tt, depth, split, w8, *args, sc, size, npp, w, n) == E, (depth, split)
    assert ok(*args, sc, size, 63, w, n) == E                  # a slab below the minimum
    assert ok(*args, sc, size - 1, npp, w, n) == E             # scratch too small
    assert ok(*args, sc, size, npp * 2, w, n) == E             # ... for this slab
    assert ok(*args, None, size, npp, w, n) == E               # no scratch
    assert ok(*args, sc, size, npp, None, n) == E              # no work word
    assert ok(*args, sc, size, npp, w, -1) == E
    assert raw(lib, bt, tt, MIX_DEPTH, MIX_SPLIT, None, *args, sc, size, npp, w, n) == E  # NULL weights
    assert raw(lib, None, tt, MIX_DEPTH, MIX_SPLIT, w8, *args, sc, size, npp, w, n) == E  # NULL boards
    assert ok(*args, None, 0, npp, w, 0) == 0                  # n == 0: nothing launched
    for bad in (dict(split=5), dict(split=-1), dict(split=4), dict(split=2, nodes_per_position=63)):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.search(bt, tt, MIX_DEPTH, **bad)
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.search(bt, tt, 11, split=2)
    e = ops.search(bt[:0], tt[:0], MIX_DEPTH, split=MIX_SPLIT, want_nodes=True)
    assert e.value.numel() == e.status.numel() == e.nodes.numel() == 0 and e.value.dtype == torch.int32
    # the failed calls launched nothing and the stream's next launch finds a zero word
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    # overlapping boards are INVALID, their neighbours searched
    rows = np.array([[FULL ^ 0xF, 0x10], b[0], [FULL, FULL], b[1]], np.uint64)
    b4, t4 = dev(rows, np.array([1, t[0], 2, t[1]], np.uint8))
    r = ops.search(b4, t4, MIX_DEPTH, node_limit=NODE_LIMIT, split=MIX_SPLIT, want_nodes=True)
    assert r.status.cpu().tolist() == [INVALID, SEARCHED, INVALID, SEARCHED]
    assert r.value.cpu().tolist() == [0, rv[0], 0, rv[1]] and r.best_move.cpu().tolist() == [255, rm[0], 255, rm[1]]
    nd = r.nodes.cpu().numpy().view(np.uint32)
    assert nd[0] == 0 and nd[2] == 0 and nd[1] > 0
    assert ops.work_word("cuda").item() == 0


def test_env_search_takes_a_split():
    from subproc_amd.env import VecEnv

    b, t, rv, rm = mixed()
    env = VecEnv(len(t), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(b), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(t)).cuda())
    r = env.search(MIX_DEPTH, node_limit=NODE_LIMIT, split=MIX_SPLIT)
    assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()


# ---------------------------------------------------------------- 7. the engine
ENGINE_ROOT = 4  # of solve_cases.ladder(12, 16): three moves at the root, the checker's smallest depth-10 tree (2 s)


def engine_root():
    b, t = solve_cases.ladder(12, 16)
    return b[ENGINE_ROOT:ENGINE_ROOT + 1], t[ENGINE_ROOT:ENGINE_ROOT + 1]


def test_engine_depth_10_split_4_plays_the_checkers_move(monkeypatch, capsys):
    b, t = engine_root()
    assert solve_ref.empties(b)[0] == 12
    rv, rm, _ = search_ref.search(b, t, 10, TABLES["default"])
    assert rm[0] < 64
    eng = engine.Engine(name="S", policy="search", depth=10, split=4)
    text = oracle.serialize_str(b[0, 0], b[0, 1], t[0])
    eng.board.deserialize(text[:64], text[65], 0)
    assert eng.board.bitboards() == (int(b[0, 0]), int(b[0, 1])) and eng.board.turn == int(t[0])
    out = []
    eng.handle("go", out.append)
    assert codec.parse_engine_go("".join(out))[1] == int(rm[0])
    # the line names the split, and only when there is one
    out = []
    eng.handle("verbose p", out.append)
    assert out[0].startswith("S policy=search depth=10 split=4 weights=[")
    out = []
    engine.Engine(name="S", policy="search", depth=4).handle("verbose p", out.append)
    assert out[0].startswith("S policy=search depth=4 weights=[") and "split" not in out[0]
    for bad in (dict(depth=9), dict(depth=13, split=4), dict(depth=4, split=5), dict(depth=10, split=1)):
        with pytest.raises(ValueError):
            engine.Engine(policy="search", **bad)
    monkeypatch.setattr(sys, "stdin", io.StringIO("verbose p\nquit\n"))
    assert engine.main(["--name", "CLI", "--policy", "search", "--depth", "10", "--split", "4"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("CLI policy=search depth=10 split=4 weights=[") and lines[1] == "bye"
