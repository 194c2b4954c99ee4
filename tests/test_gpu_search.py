"""ops.search / othm_search on the GPU against the exhaustive checker
(tests/search_ref.py over the C oracle): every value, move and status on midgame
roots at depths 1..5 and on endgame roots at depth 8 (the deepest stack, with
eval and game-over leaves mixed), the identity with the exact solver where the
horizon reaches the end, depth 1 against the 1-ply eval policy, and the launch
plumbing (shapes, refill, work word, node limit)."""
import functools

import numpy as np
import pytest
import torch

import oracle
import search_ref
import solve_cases
import solve_ref

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops, params  # noqa: E402

SEARCHED, INVALID, LIMIT = _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT
T = search_ref.T
FULL = (1 << 64) - 1
NODE_LIMIT = 1 << 22  # no case here needs more than 38,434 nodes (host build): a defect ends as LIMIT, not as a long kernel
TABLES = {"default": np.asarray(params.DEFAULT_WEIGHTS, np.int8), "rng7": search_ref.WEIGHTS_B}
BOTH = ("default", "rng7")
# the second table pushed to the ends of int8: +127 where it is positive, -128 elsewhere, its one -127 kept
TABLES["extreme"] = np.where(search_ref.WEIGHTS_B > 0, 127, -128).astype(np.int8)
TABLES["extreme"][search_ref.WEIGHTS_B == -127] = -127
MID_CASES = {1: 1024, 2: 256, 3: 64, 4: 32, 5: 8}  # depth -> roots


def gpu_search(boards, turn, depth, weights, node_limit=NODE_LIMIT, **kw):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    t = torch.from_numpy(np.array(turn, np.uint8)).cuda()
    r = ops.search(b, t, depth, weights=weights, node_limit=node_limit, want_nodes=True, **kw)
    torch.cuda.synchronize()
    return (r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy(),
            r.nodes.cpu().numpy().view(np.uint32))


@functools.lru_cache(maxsize=None)
def midgame():
    g = oracle.sample_midgame(4096, 0x5EED)
    for v in g.values():
        v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(kind, depth, table):
    """The checker's (boards, turn, value, best_move) of a case, computed once."""
    if kind == "mid":
        g = midgame()
        k = MID_CASES[depth]
        b, t = g["boards"][:k], g["turn"][:k]
    elif kind == "special":  # every forced-pass and game-over root of the solver's cases
        cs = solve_cases.cases()
        sel = {e: cs[e]["forced_pass"] | cs[e]["over"] for e in cs}
        b = np.concatenate([cs[e]["boards"][sel[e]] for e in sorted(cs)])
        t = np.concatenate([cs[e]["turn"][sel[e]] for e in sorted(cs)])
    else:  # ("end", empties) of the solver's pool
        e, k = kind[1], {9: 32, 8: 64, 6: 256}[kind[1]]
        p = solve_cases.pool()[e]
        b, t = p["boards"][:k], p["turn"][:k]
    v, m, _ = search_ref.search(b, t, depth, TABLES[table])
    for a in (v, m):
        a.setflags(write=False)
    return b, t, v, m


def assert_equals_checker(b, t, rv, rm, depth, table):
    v, m, s, nd = gpu_search(b, t, depth, TABLES[table])
    assert (s == SEARCHED).all()
    bad = np.nonzero((v != rv) | (m != rm))[0]
    assert len(bad) == 0, (depth, table, bad[:8], v[bad[:8]], rv[bad[:8]], m[bad[:8]], rm[bad[:8]])
    return v, m, nd


# ---------------------------------------------------------------- 1. checker parity, midgame
@pytest.mark.parametrize("table", BOTH)
@pytest.mark.parametrize("depth", sorted(MID_CASES))
def test_midgame_matches_the_checker(depth, table):
    b, t, rv, rm = reference("mid", depth, table)
    assert len(t) == MID_CASES[depth]
    emp = solve_ref.empties(b)
    assert emp.min() >= 11 and emp.max() <= 50
    assert_equals_checker(b, t, rv, rm, depth, table)


# ---------------------------------------------------------------- 2. checker parity, endgame
@pytest.mark.parametrize("table", BOTH)
def test_depth_8_at_9_empties_mixes_eval_and_terminal_leaves(table):
    b, t, rv, rm = reference(("end", 9), 8, table)
    assert len(t) == 32 and (solve_ref.empties(b) == 9).all()
    assert_equals_checker(b, t, rv, rm, 8, table)
    # every root's value is eval-derived: the horizon cuts the tree one ply short
    assert (np.abs(rv.astype(np.int64)) < T).all()


@pytest.mark.parametrize("e", [8, 6])
@pytest.mark.parametrize("table", BOTH)
def test_depth_8_reaching_the_end_is_t_times_the_solver(e, table):
    b, t, rv, rm = reference(("end", e), 8, table)
    assert len(t) == {8: 64, 6: 256}[e] and (solve_ref.empties(b) == e).all()
    v, m, _ = assert_equals_checker(b, t, rv, rm, 8, table)
    r = ops.solve(ops.from_numpy_u64(np.array(b), "cuda"), torch.from_numpy(np.array(t)).cuda(), max_empties=e,
                  node_limit=NODE_LIMIT)
    assert (r.status.cpu().numpy() == _lib.SOLVE_SOLVED).all()
    sv, sm = r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy()
    assert (v == T * sv).all() and (m == sm).all()
    assert (rv == T * sv).all() and (rm == sm).all()  # the identity holds in the checker too


@pytest.mark.parametrize("table", BOTH)
def test_depth_3_on_forced_pass_and_game_over_roots(table):
    b, t, rv, rm = reference("special", 3, table)
    cs = solve_cases.cases()
    fp = np.concatenate([cs[e]["forced_pass"][cs[e]["forced_pass"] | cs[e]["over"]] for e in sorted(cs)])
    assert fp.any() and (~fp).any()
    v, m, nd = assert_equals_checker(b, t, rv, rm, 3, table)
    assert (m[fp] == 64).all() and (m[~fp] == 255).all()
    assert (nd[~fp] == 0).all() and (nd[fp] >= 2).all()
    res = oracle.result(b[~fp])["diff"].astype(np.int64) * np.where(solve_ref.mover(t[~fp]) == 1, 1, -1)
    assert (v[~fp] == T * res).all()


# ---------------------------------------------------------------- 3. depth 1 is the eval policy
def test_depth_1_is_the_eval_policy():
    g = midgame()
    b, t = g["boards"], g["turn"]
    own = oracle.legal(b, t)
    assert (own != 0).all() and len(t) == 4096
    idx, sq = solve_ref._bits(own)
    kids = oracle.step(b[idx], t[idx], sq)
    # no child is a finished game (rule 1 never interferes): checked on the CPU
    assert (oracle.result(kids["boards"])["terminal"] == 0).all()
    kb = ops.from_numpy_u64(kids["boards"], "cuda")
    st = ops.step(ops.from_numpy_u64(np.array(b[idx]), "cuda"), torch.from_numpy(np.array(t[idx])).cuda(),
                  torch.from_numpy(sq).cuda())
    assert torch.equal(st.boards, kb)
    ev = ops.evaluate(st.boards, torch.from_numpy(np.array(t[idx])).cuda(), TABLES["default"]).cpu().numpy()
    v, m, s, _ = gpu_search(b, t, 1, TABLES["default"])
    assert (s == SEARCHED).all()
    best = np.full(len(t), -(1 << 40), np.int64)
    np.maximum.at(best, idx, ev.astype(np.int64))
    hit = ev == best[idx]
    low = np.full(len(t), 255, np.int64)
    np.minimum.at(low, idx[hit], sq[hit].astype(np.int64))
    assert (v == best).all() and (m == low).all()
    ties = np.bincount(idx[hit], minlength=len(t)) > 1
    assert ties.sum() == 167  # the tie rule is exercised


# ---------------------------------------------------------------- 4. contract
def mixed(n):
    """n roots drawn in turn from the 64 roots of the depth-3 midgame case and 64 of the forced-pass / game-over
    roots, shuffled once, with the checker's depth-3 answers."""
    mid, special = reference("mid", 3, "default"), reference("special", 3, "default")
    some = np.sort(np.random.default_rng(4).permutation(len(special[1]))[:64])
    b, t, v, m = (np.concatenate([x, y[some]]) for x, y in zip(mid, special))
    order = np.random.default_rng(3).permutation(len(t))
    pick = order[np.arange(n) % len(order)]
    return b[pick], t[pick], v[pick], m[pick]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(n):
    b, t, rv, rm = mixed(n)
    v, m, s, _ = gpu_search(b, t, 3, TABLES["default"])
    assert (s == SEARCHED).all() and (v == rv).all() and (m == rm).all()
    assert ops.work_word("cuda").item() == 0


def test_results_do_not_depend_on_the_batch():
    b, t, rv, rm = mixed(777)
    v, m, s, nd = gpu_search(b, t, 3, TABLES["default"])
    perm = np.random.default_rng(5).permutation(len(t))
    vp, mp, sp, ndp = gpu_search(b[perm], t[perm], 3, TABLES["default"])
    assert (vp == v[perm]).all() and (mp == m[perm]).all() and (sp == s[perm]).all() and (ndp == nd[perm]).all()
    v1, m1, _, nd1 = gpu_search(b[:5], t[:5], 3, TABLES["default"])
    assert (v1 == v[:5]).all() and (m1 == m[:5]).all() and (nd1 == nd[:5]).all()
    assert (v == rv).all() and (m == rm).all()


def test_one_block_refills_through_the_whole_batch(monkeypatch):
    b, t, rv, rm = mixed(1000)
    v0, m0, s0, nd0 = gpu_search(b, t, 3, TABLES["default"])
    assert _lib.load().othm_search_grid(1000) == 16
    monkeypatch.setenv("OTH_SEARCH_BLOCKS", "1")
    assert _lib.load().othm_search_grid(1000) == 1
    v, m, s, nd = gpu_search(b, t, 3, TABLES["default"])
    assert ops.work_word("cuda").item() == 0
    assert (v == rv).all() and (m == rm).all() and (s == SEARCHED).all()
    assert (v == v0).all() and (m == m0).all() and (nd == nd0).all()


def test_work_word_is_shared_with_a_rollout_and_a_solve_and_left_zero():
    b, t, rv, rm = mixed(333)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.search(bt, tt, 3, node_limit=NODE_LIMIT, work=w)  # two launches back to back on one word
    r2 = ops.search(bt, tt, 3, node_limit=NODE_LIMIT, work=w)
    torch.cuda.synchronize()
    assert w.item() == 0
    assert (r1.value.cpu().numpy() == rv).all() and (r2.value.cpu().numpy() == rv).all()
    assert (r2.best_move.cpu().numpy() == rm).all() and r1.nodes is None
    # a rollout, a search and a solve share the stream's word
    c = solve_cases.cases()[6]
    cb, ct = ops.from_numpy_u64(np.array(c["boards"]), "cuda"), torch.from_numpy(np.array(c["turn"])).cuda()
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r3 = ops.search(bt, tt, 3, node_limit=NODE_LIMIT)
    sv = ops.solve(cb, ct, max_empties=6, node_limit=NODE_LIMIT)
    r4 = ops.search(bt, tt, 3, node_limit=NODE_LIMIT)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    for r in (r3, r4):
        assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()
    assert (sv.value.cpu().numpy() == c["value"]).all() and (sv.best_move.cpu().numpy() == c["best_move"]).all()
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)
    go = oracle.rollout(1000, 9)
    assert (ops.to_numpy_u64(g2.final_boards) == go["final_boards"]).all()


def raw_search(lib, bt, tt, depth, w8, val, mv, st, nd, work, n):
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    return lib.othm_search(ptr(bt), ptr(tt), depth, w8, NODE_LIMIT, ptr(val), ptr(mv), ptr(st), ptr(nd), ptr(work), n,
                           torch.cuda.current_stream().cuda_stream)


def test_null_outputs_and_null_turn():
    b, t, rv, rm = mixed(300)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    n = len(t)
    w = ops.work_word("cuda")
    lib, w8 = _lib.load(), ops._weights_ptr(None)
    val = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    mv = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    assert raw_search(lib, bt, tt, 3, w8, None, None, None, None, w, n) == 0
    assert raw_search(lib, bt, tt, 3, w8, val, None, None, None, w, n) == 0
    assert raw_search(lib, bt, tt, 3, w8, None, mv, None, None, w, n) == 0
    vb = torch.empty(n, dtype=torch.int32, device="cuda")
    assert raw_search(lib, bt, None, 3, w8, vb, None, None, None, w, n) == 0  # turn NULL: Black everywhere
    assert raw_search(lib, bt, tt, 3, w8, None, None, None, None, None, n) == _lib.OTH_EINVAL  # no work word
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == rv).all() and (mv.cpu().numpy() == rm).all() and w.item() == 0
    black = gpu_search(b, np.ones(n, np.uint8), 3, TABLES["default"])[0]
    assert (vb.cpu().numpy() == black).all()


def test_empty_batch_bad_arguments_and_overlap():
    b = torch.empty((0, 2), dtype=torch.int64, device="cuda")
    t = torch.empty(0, dtype=torch.uint8, device="cuda")
    r = ops.search(b, t, 3, want_nodes=True)
    assert r.value.numel() == r.best_move.numel() == r.status.numel() == r.nodes.numel() == 0
    assert r.value.dtype == torch.int32
    lib = _lib.load()
    assert lib.othm_search_grid(0) == 0 and lib.othm_search_grid(-1) == _lib.OTH_EINVAL
    assert lib.othm_search_grid(1) == 1 and lib.othm_search_grid(65) == 2
    assert 2 <= lib.othm_search_grid(1 << 30) <= 1 << 20
    bb, tt, rv, rm = mixed(4)
    bt, tt = ops.from_numpy_u64(bb, "cuda"), torch.from_numpy(tt).cuda()
    for bad in (0, 9, -1):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.search(bt, tt, bad)
    w = ops.work_word("cuda")
    val = torch.empty(4, dtype=torch.int32, device="cuda")
    assert raw_search(lib, bt, tt, 3, None, val, None, None, None, w, 4) == _lib.OTH_EINVAL  # NULL weights
    with pytest.raises(ValueError, match="32 bits"):
        ops.search(bt, tt, 3, node_limit=1 << 32)
    with pytest.raises(TypeError):
        ops.search(bt, tt.to(torch.int32), 3)
    # the failed calls launched nothing and the stream's next launch finds a zero word
    r = ops.search(bt, tt, 3, node_limit=NODE_LIMIT)
    assert (r.status.cpu().numpy() == SEARCHED).all() and (r.value.cpu().numpy() == rv).all()
    assert ops.work_word("cuda").item() == 0
    # overlapping boards are INVALID, their neighbours searched
    rows = np.array([[FULL ^ 0xF, 0x10], bb[0], [FULL, FULL], bb[1]], np.uint64)
    v, m, s, nd = gpu_search(rows, np.array([1, tt[0].item(), 2, tt[1].item()], np.uint8), 3, TABLES["default"])
    assert s.tolist() == [INVALID, SEARCHED, INVALID, SEARCHED]
    assert v.tolist() == [0, rv[0], 0, rv[1]] and m.tolist() == [255, rm[0], 255, rm[1]]
    assert nd[0] == 0 and nd[2] == 0


def test_node_limit_splits_exactly_at_the_count():
    b, t, rv, rm = reference("mid", 3, "default")
    v0, m0, s0, nd0 = gpu_search(b, t, 3, TABLES["default"])
    assert (s0 == SEARCHED).all()
    limit = int(np.sort(nd0)[len(nd0) // 2])  # a count that occurs: that position is still searched
    assert nd0.min() < limit < nd0.max()
    v, m, s, nd = gpu_search(b, t, 3, TABLES["default"], node_limit=limit)
    over = nd0 > limit
    assert over.any() and (~over).any() and (nd0 == limit).any()
    assert (s[over] == LIMIT).all() and (v[over] == 0).all() and (m[over] == 255).all() and (nd[over] == limit).all()
    assert (s[~over] == SEARCHED).all() and (v[~over] == v0[~over]).all() and (m[~over] == m0[~over]).all()
    assert (nd[~over] == nd0[~over]).all() and (nd <= limit).all()
    # one position alone: its own count is enough, one less is not
    i = int(np.argmax(nd0))
    v1, m1, s1, nd1 = gpu_search(b[i:i + 1], t[i:i + 1], 3, TABLES["default"], node_limit=int(nd0[i]))
    assert (s1[0], v1[0], m1[0], nd1[0]) == (SEARCHED, v0[i], m0[i], nd0[i])
    v1, m1, s1, nd1 = gpu_search(b[i:i + 1], t[i:i + 1], 3, TABLES["default"], node_limit=int(nd0[i]) - 1)
    assert (s1[0], v1[0], m1[0], nd1[0]) == (LIMIT, 0, 255, nd0[i] - 1)


def test_extreme_weights_need_the_32_bit_window():
    """The second table with its weights at +127, -127 and -128, depth 3: eval
    values far outside the solver's 8-bit window, and, on the forced-pass and
    game-over roots, terminal values of up to 56 * 2**17 beside them."""
    w = TABLES["extreme"]
    assert set(np.unique(w).tolist()) == {-128, -127, 127}
    b, t, rv, rm = reference("mid", 3, "extreme")
    assert_equals_checker(b, t, rv, rm, 3, "extreme")
    assert np.abs(rv.astype(np.int64)).max() > 127
    sb, st, srv, srm = reference("special", 3, "extreme")
    assert_equals_checker(sb, st, srv, srm, 3, "extreme")
    big = np.abs(srv.astype(np.int64))
    assert big.max() == 56 * T and ((big > 0) & (big < T)).any()


def test_env_search():
    from subproc_amd.env import VecEnv

    b, t, rv, rm = reference("mid", 2, "default")
    env = VecEnv(len(t), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(b), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(t)).cuda())
    r = env.search(2, node_limit=NODE_LIMIT)
    assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()
