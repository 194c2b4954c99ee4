"""The ordered searches (order = 1; include/othello_order.h) on the GPU: every
value, move and status equals the exhaustive checker's and the unordered
search's, ties included, from fewer nodes; the same for whole games
(ops.play), the split search's tasks and the engine; and the launch contract
(node limit with the scoring placements counted, independence of the batch and
the grid, null outputs)."""
import functools

import numpy as np
import pytest
import torch

import oracle
import order_cases
import search_ref
import tree_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, engine, ops  # noqa: E402

SEARCHED, INVALID, LIMIT = _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT
T = search_ref.T
FULL = (1 << 64) - 1
NODE_LIMIT = 1 << 24  # the hardest case here (depth 6, order 0) needs 1,239,852 nodes on the host build
TABLES = order_cases.TABLES


def gpu_search(boards, turn, depth, order, table="default", node_limit=NODE_LIMIT, **kw):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    t = torch.from_numpy(np.array(turn, np.uint8)).cuda()
    r = ops.search(b, t, depth, weights=TABLES[table], node_limit=node_limit, want_nodes=True, order=order, **kw)
    torch.cuda.synchronize()
    return (r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy(),
            r.nodes.cpu().numpy().view(np.uint32))


def assert_same(got, want, what):
    for k, (x, y) in enumerate(zip(got[:3], want[:3])):
        bad = np.nonzero(np.asarray(x) != np.asarray(y))[0]
        assert len(bad) == 0, (what, ("value", "move", "status")[k], bad[:8], np.asarray(x)[bad[:8]],
                               np.asarray(y)[bad[:8]])


@functools.lru_cache(maxsize=None)
def both_orders(depth):
    """order 0's and order 1's answers on order_cases.versus(depth), computed once."""
    b, t = order_cases.versus(depth)
    return gpu_search(b, t, depth, 0), gpu_search(b, t, depth, 1)


# ---------------------------------------------------------------- 1. the checker
@pytest.mark.parametrize("table", order_cases.BOTH)
@pytest.mark.parametrize("depth", sorted(order_cases.MID))
def test_midgame_matches_the_checker(depth, table):
    b, t = order_cases.mid(depth)
    rv, rm = order_cases.mid_reference(depth, table)
    v, m, s, _ = gpu_search(b, t, depth, 1, table)
    assert_same((v, m, s), (rv, rm, np.full(len(t), SEARCHED)), (depth, table))


# ---------------------------------------------------------------- 2. order 0
@pytest.mark.parametrize("depth", sorted(order_cases.VERSUS))  # 2, 3 and 4: where the rule changes, as root depths
def test_equals_order_0(depth):
    r0, r1 = both_orders(depth)
    assert len(r0[0]) == order_cases.VERSUS[depth] and (r0[2] == SEARCHED).all()
    assert_same(r1, r0, depth)
    print("depth %d: nodes %d -> %d" % (depth, r0[3].sum(dtype=np.int64), r1[3].sum(dtype=np.int64)))


def test_depth_5_searches_half_the_nodes():
    """The point of the feature: the node sum of the 4,096 roots at depth 5,
    scoring placements included, against order 0's.  The bound is the host
    build's ratio on these roots (0.4934; order_cases.DEPTH5_HOST_NODES)
    rounded up to the next 0.05."""
    r0, r1 = both_orders(5)
    n0, n1 = int(r0[3].sum(dtype=np.int64)), int(r1[3].sum(dtype=np.int64))
    print("depth 5 x4096: nodes %d -> %d, ratio %.4f; max/mean %.1f -> %.1f" % (
        n0, n1, n1 / n0, r0[3].max() / r0[3].mean(), r1[3].max() / r1[3].mean()))
    assert n1 < n0 and n1 / n0 <= order_cases.DEPTH5_RATIO_BOUND


# ---------------------------------------------------------------- 3. the end of the game
def solver(b, t, e):
    r = ops.solve(ops.from_numpy_u64(np.array(b), "cuda"), torch.from_numpy(np.array(t)).cuda(), max_empties=e,
                  node_limit=NODE_LIMIT)
    assert (r.status.cpu().numpy() == _lib.SOLVE_SOLVED).all()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy()


def test_depth_8_at_up_to_8_empties_is_the_solver():
    b, t = order_cases.endgame(8)
    sv, sm = solver(b, t, 8)
    v, m, s, _ = gpu_search(b, t, 8, 1)
    assert_same((v, m, s), (T * sv, sm, np.full(len(t), SEARCHED)), "depth 8")


def test_depth_10_split_2_at_up_to_10_empties_is_the_solver():
    b, t = order_cases.endgame(10)
    sv, sm = solver(b, t, 10)
    # at most 10 moves per node: 1 + 10 + 100 nodes and the passes fit 256
    v, m, s, _ = gpu_search(b, t, 10, 1, split=2, nodes_per_position=256)
    assert_same((v, m, s), (T * sv, sm, np.full(len(t), SEARCHED)), "depth 10 split 2")


# ---------------------------------------------------------------- 4. ties
@functools.lru_cache(maxsize=None)
def opening_reference(depth):
    ob, ot = tree_cases.opening_ties()
    rv, rm, _ = search_ref.search(ob, ot, depth, TABLES["default"])
    return rv, rm


@pytest.mark.parametrize("depth,value", [(4, 560), (5, 900), (6, 660)])
def test_opening_ties_keep_the_lowest_maximiser(depth, value):
    ob, ot = tree_cases.opening_ties()
    rv, rm = opening_reference(depth)
    assert rv[0] == value and rm[0] == 19 and (rv == value).all()
    v, m, s, _ = gpu_search(ob, ot, depth, 1)
    assert_same((v, m, s), (rv, rm, np.full(16, SEARCHED)), depth)
    v, m, s, _ = gpu_search(ob, ot, depth, 1, split=2)
    assert_same((v, m, s), (rv, rm, np.full(16, SEARCHED)), (depth, "split 2"))


def test_ties_whose_lowest_maximiser_is_in_a_later_class():
    """Where the ordered root meets another maximiser first, the root tie rule
    hands the move back to the lowest one (the flags are worked out on the CPU:
    tests/order_cases.py)."""
    b, t, rv, rm, later = order_cases.two_empties()
    assert later.sum() >= 1
    v, m, s, _ = gpu_search(b, t, 2, 1)
    assert_same((v, m, s), (rv, rm, np.full(len(t), SEARCHED)), "two empties")
    for table in order_cases.BOTH:
        b, t, rv, rm, later = order_cases.depth1_ties(table)
        assert later.sum() >= 5
        v, m, s, _ = gpu_search(b, t, 1, 1, table)
        assert_same((v, m, s), (rv, rm, np.full(len(t), SEARCHED)), ("depth 1", table))


@pytest.mark.parametrize("depth,roots,least", [(3, 1024, 20), (4, 128, 3)])
def test_mobility_ordered_roots_that_meet_a_higher_maximiser_first(depth, roots, least):
    """The tie rule's own mechanism: at these roots (chosen on the CPU from every
    root move's exhaustive value, tests/order_cases.py) the mobility order plays
    a maximiser at a higher square before the lowest one, which is then
    searched from alpha - 1 and must take the move over on exactly alpha."""
    b, t, rv, rm = order_cases.mobility_ties(depth, roots)
    assert len(t) >= least
    v, m, s, _ = gpu_search(b, t, depth, 1)
    assert_same((v, m, s), (rv, rm, np.full(len(t), SEARCHED)), ("mobility ties", depth))
    assert_same(gpu_search(b, t, depth, 0), (rv, rm, np.full(len(t), SEARCHED)), ("order 0", depth))


# ---------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("table", order_cases.BOTH)
def test_forced_pass_and_game_over_roots(table):
    b, t = order_cases.special()
    rv, rm = order_cases.special_reference(table)
    assert (rm == 64).any() and (rm == 255).any()
    v, m, s, nd = gpu_search(b, t, 3, 1, table)
    assert_same((v, m, s), (rv, rm, np.full(len(t), SEARCHED)), table)
    assert (nd[rm == 255] == 0).all() and (nd[rm == 64] >= 2).all()


def test_single_move_roots_and_overlapping_boards():
    b, t, sq = order_cases.single_move_roots()
    assert len(t) >= 8
    for depth in (1, 3, 5):
        r0, r1 = gpu_search(b, t, depth, 0), gpu_search(b, t, depth, 1)
        assert_same(r1, r0, depth)
        assert (r1[1] == sq).all()
    rows = np.array([[FULL ^ 0xF, 0x10], b[0], [FULL, FULL], b[1]], np.uint64)
    turn = np.array([1, t[0], 2, t[1]], np.uint8)
    v, m, s, nd = gpu_search(rows, turn, 3, 1)
    v0, m0, s0, _ = gpu_search(rows, turn, 3, 0)
    assert s.tolist() == [INVALID, SEARCHED, INVALID, SEARCHED] and nd[0] == 0 and nd[2] == 0
    assert v.tolist() == v0.tolist() and m.tolist() == m0.tolist() and m[0] == 255 and v[0] == 0


def raw_search(lib, bt, tt, depth, order, val, mv, st, nd, work, n):
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    return lib.otho_search_ordered(ptr(bt), ptr(tt), depth, order, ops._weights_ptr(None), NODE_LIMIT, ptr(val),
                                   ptr(mv), ptr(st), ptr(nd), ptr(work), n, torch.cuda.current_stream().cuda_stream)


def test_null_outputs_null_turn_and_order_0_through_the_new_entry():
    b, t = order_cases.mid(3)
    rv, rm = order_cases.mid_reference(3, "default")
    bt, tt = ops.from_numpy_u64(np.array(b), "cuda"), torch.from_numpy(np.array(t)).cuda()
    n, w, lib = len(t), ops.work_word("cuda"), _lib.load()
    val = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    mv = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    assert raw_search(lib, bt, tt, 3, 1, None, None, None, None, w, n) == 0
    assert raw_search(lib, bt, tt, 3, 1, val, None, None, None, w, n) == 0
    assert raw_search(lib, bt, tt, 3, 1, None, mv, None, None, w, n) == 0
    vb = torch.empty(n, dtype=torch.int32, device="cuda")
    assert raw_search(lib, bt, None, 3, 1, vb, None, None, None, w, n) == 0  # turn NULL: Black everywhere
    assert raw_search(lib, bt, tt, 3, 2, val, None, None, None, w, n) == _lib.OTH_EINVAL
    v0 = torch.empty(n, dtype=torch.int32, device="cuda")
    nd0 = torch.empty(n, dtype=torch.int32, device="cuda")
    assert raw_search(lib, bt, tt, 3, 0, v0, None, None, nd0, w, n) == 0  # order 0: the unordered kernel
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == rv).all() and (mv.cpu().numpy() == rm).all() and w.item() == 0
    assert (vb.cpu().numpy() == gpu_search(b, np.ones(n, np.uint8), 3, 0)[0]).all()
    plain = gpu_search(b, t, 3, 0)
    assert (v0.cpu().numpy() == plain[0]).all() and (nd0.cpu().numpy().view(np.uint32) == plain[3]).all()
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.search(bt, tt, 3, order=2)
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.search(bt, tt, 5, order=-1, split=2)
    assert ops.search(bt, tt, 3, node_limit=NODE_LIMIT, order=1).nodes is None and ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 6. the node limit
def test_node_limit_counts_the_scoring_placements():
    b, t = order_cases.mid(4)
    (v0, m0, s0, nd0), (v1, m1, s1, nd1) = gpu_search(b, t, 4, 0), gpu_search(b, t, 4, 1)
    assert (s1 == SEARCHED).all()
    # depth 4 orders its root and the frames below it by mobility: a root with k >= 2 moves scores k before it plays
    # one, so the count exceeds what the ordered tree alone could hold whenever the trees are equal in size
    own = oracle.legal(b, t)
    k = np.array([bin(int(x)).count("1") for x in own])
    assert (nd1[k >= 2] >= k[k >= 2] + 1).all()
    limit = int(np.sort(nd1)[len(nd1) // 2])
    assert nd1.min() < limit < nd1.max()
    v, m, s, nd = gpu_search(b, t, 4, 1, node_limit=limit)
    over = nd1 > limit
    assert over.any() and (~over).any() and (nd1 == limit).any()
    assert (s[over] == LIMIT).all() and (v[over] == 0).all() and (m[over] == 255).all() and (nd[over] == limit).all()
    assert (s[~over] == SEARCHED).all() and (v[~over] == v1[~over]).all() and (m[~over] == m1[~over]).all()
    assert (nd[~over] == nd1[~over]).all()
    for i in (int(np.argmax(nd1)), int(np.argmin(np.where(k >= 2, nd1, 1 << 30)))):
        one = gpu_search(b[i:i + 1], t[i:i + 1], 4, 1, node_limit=int(nd1[i]))
        assert (one[2][0], one[0][0], one[1][0], one[3][0]) == (SEARCHED, v1[i], m1[i], nd1[i])
        one = gpu_search(b[i:i + 1], t[i:i + 1], 4, 1, node_limit=int(nd1[i]) - 1)
        assert (one[2][0], one[0][0], one[1][0], one[3][0]) == (LIMIT, 0, 255, nd1[i] - 1)
    # a limit that ends the search inside the root's first scoring pass
    i = int(np.argmax(k))
    one = gpu_search(b[i:i + 1], t[i:i + 1], 4, 1, node_limit=int(k[i]) - 1)
    assert (one[2][0], one[3][0]) == (LIMIT, k[i] - 1)


# ---------------------------------------------------------------- 7. independence
@functools.lru_cache(maxsize=None)
def mixed():
    """200 roots: midgame ones and forced-pass / game-over ones, shuffled once, with order 1's depth-4 answers."""
    g = tree_cases.midgame()
    sb, st = order_cases.special()
    some = np.sort(np.random.default_rng(4).permutation(len(st))[:60])
    b, t = np.concatenate([g["boards"][:140], sb[some]]), np.concatenate([g["turn"][:140], st[some]])
    perm = np.random.default_rng(3).permutation(len(t))
    b, t = b[perm], t[perm]
    return b, t, gpu_search(b, t, 4, 1)


def test_one_block_refills_while_others_score(monkeypatch):
    b, t, want = mixed()
    assert len(t) == 200 and _lib.load().otho_search_ordered_grid(200, 1) == 4
    assert_same(want, gpu_search(b, t, 4, 0), "order 0")
    monkeypatch.setenv("OTH_SEARCH_BLOCKS", "1")
    assert _lib.load().otho_search_ordered_grid(200, 1) == 1
    got = gpu_search(b, t, 4, 1)
    assert ops.work_word("cuda").item() == 0
    assert_same(got, want, "one block")
    assert (got[3] == want[3]).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_and_neighbours(n):
    b, t, want = mixed()
    pick = np.random.default_rng(n).permutation(len(t))[:n]
    got = gpu_search(b[pick], t[pick], 4, 1)
    assert_same(got, tuple(x[pick] for x in want), n)
    assert (got[3] == want[3][pick]).all() and ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 8. play
KEYS = ("a_black", "final_boards", "diff", "plies", "status", "moves", "hist")


def gpu_play(case, order):
    c = order_cases.PLAY[case]
    b, t = order_cases.play_starts(case)
    start = None if b is None else ops.from_numpy_u64(np.array(b), "cuda")
    turn = None if t is None else torch.from_numpy(np.array(t)).cuda()
    r = ops.play(c["n"], c["seed"], c["game_id0"], TABLES[c["tables"][0]], TABLES[c["tables"][1]], c["depth"][0],
                 c["depth"][1], c["exact"], c["n_rand"][0], c["n_rand"][1], c["swap"], start, turn, record_moves=True,
                 node_limit=NODE_LIMIT, want_nodes=True, order=order)
    torch.cuda.synchronize()
    out = {k: getattr(r, k).cpu().numpy() for k in KEYS}
    out["final_boards"] = ops.to_numpy_u64(r.final_boards)
    return out, r.nodes.cpu().numpy()


@pytest.mark.parametrize("case", sorted(order_cases.PLAY))
def test_games_are_the_same_move_for_move(case):
    g0, n0 = gpu_play(case, 0)
    g1, n1 = gpu_play(case, 1)
    ref = order_cases.play_reference(case)
    assert len(n1) == 128 and sum(c["n"] for c in order_cases.PLAY.values()) == 256 and (g1["status"] == SEARCHED).all()
    for k in KEYS:
        assert (g1[k] == g0[k]).all(), (case, k)
        assert (g1[k].astype(np.int64) == np.asarray(ref[k]).astype(np.int64)).all(), (case, k, "checker")
    print("%s: nodes %d -> %d" % (case, n0.sum(), n1.sum()))
    assert n1.sum() < n0.sum()
    assert ops.work_word("cuda").item() == 0


def test_runner_and_env_pass_the_order_on():
    from subproc_amd import runner
    from subproc_amd.env import VecEnv

    conf = {"proc_n_rand_hands_for_a": 2, "proc_n_rand_hands_for_b": 2, "proc_randomize_black_white": 1}
    a = runner.do_matches(conf, n=16, seed=5, policy="search", depth=(3, 2), exact_empties=4, order=0)
    b = runner.do_matches(conf, n=16, seed=5, policy="search", depth=(3, 2), exact_empties=4, order=1)
    assert torch.equal(a.games.moves, b.games.moves) and torch.equal(a.games.final_boards, b.games.final_boards)
    assert a.won == b.won and a.meta == b.meta and (a.a_black == b.a_black).all()
    assert torch.equal(a.books.pos.boards, b.books.pos.boards)
    with pytest.raises(ValueError):
        runner.do_matches(conf, n=1, policy="eval", order=1)
    pb, pt = order_cases.mid(2)
    rv, rm = order_cases.mid_reference(2, "default")
    env = VecEnv(len(pt), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(pb), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(pt)).cuda())
    r = env.search(2, node_limit=NODE_LIMIT, order=1)
    assert (r.value.cpu().numpy() == rv).all() and (r.best_move.cpu().numpy() == rm).all()


# ---------------------------------------------------------------- 9. the split search
@pytest.mark.parametrize("slab", [32768, 64])
@pytest.mark.parametrize("name,depth", [("mid5", 6), ("deep10", 10)])
def test_split_2_equals_order_0(name, depth, slab):
    """tree_cases' inputs: 8 midgame roots at depth 6, 2 roots at 11 empties at depth 10."""
    b, t = tree_cases.inputs(name)
    r0 = gpu_search(b, t, depth, 0, split=2, nodes_per_position=slab)
    r1 = gpu_search(b, t, depth, 1, split=2, nodes_per_position=slab)
    assert_same(r1, r0, (name, depth, slab))  # status too: OTHT_NOROOM comes from the expansion, which is not ordered
    assert set(r1[2].tolist()) <= {SEARCHED, _lib.TREE_NOROOM}
    if slab == 64 and name == "deep10":  # one of its two roots does not fit 64 nodes two plies down, the other does
        assert sorted(r1[2].tolist()) == [SEARCHED, _lib.TREE_NOROOM]
    if slab == 32768:
        assert (r1[2] == SEARCHED).all()
        if name == "deep10":
            rv, rm, _ = tree_cases.reference(name, "default")
            assert (r1[0] == rv).all() and (r1[1] == rm).all()
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 10. the engine
def go(eng):
    out = []
    eng.handle("go", out.append)
    from subproc_amd import codec

    return codec.parse_engine_go("".join(out))[1]


def engine_at(black, white, turn, **kw):
    eng = engine.Engine(**kw)
    text = oracle.serialize_str(black, white, turn)
    eng.board.deserialize(text[:64], text[65], 0)
    return eng


def test_engine_answers_the_same_go():
    g = tree_cases.midgame()
    for i in range(6):
        bl, wh, tn = g["boards"][i, 0], g["boards"][i, 1], g["turn"][i]
        for kw in (dict(depth=4), dict(depth=6, split=2)):
            assert go(engine_at(bl, wh, tn, policy="search", order=1, **kw)) == go(
                engine_at(bl, wh, tn, policy="search", **kw)), (i, kw)
    out = []
    engine.Engine(name="E", policy="search", depth=4, order=1).handle("verbose p", out.append)
    assert out[0].startswith("E policy=search depth=4 order=1 weights=[")
    with pytest.raises(ValueError):
        engine.Engine(policy="search", depth=4, order=2)


def test_engine_command_line_takes_order_and_still_shows():
    from test_gpu_engine import Player

    p = Player(["--policy", "search", "--depth", "3", "--order", "1", "--name", "GPU-ordered"])
    q = engine.Engine(name="Q", policy="search", depth=3)
    p.init()
    q.handle("init", [].append)
    assert "order=1" in p.show_hamlet_param()
    mv = p.go()
    from subproc_amd import codec

    assert p.name == "GPU-ordered" and codec.move_code(mv.lower()) == go(q)
    assert p.show() == (False, "None")
    p.end_process()
    assert p.proc.returncode == 0
