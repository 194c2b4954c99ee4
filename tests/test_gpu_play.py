"""ops.play / othp_play on the GPU: whole games between two searching players
against the checker (tests/play_ref.py over the C oracle and search_ref), the
exact endgame against the solver, the kernel's games against a host loop of
ops.search + ops.step, depth 1 against the 1-ply eval runner, the launch
plumbing (shapes, split, refill, work word, bad arguments), the node limit and
runner.do_matches(policy="search").  Every comparison is bit-exact."""
import functools

import numpy as np
import pytest
import torch

import oracle
import play_cases
import play_ref
import search_ref
import solve_cases

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops, runner  # noqa: E402

SEARCHED, INVALID, LIMIT = _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT
NODE_LIMIT = 1 << 22  # per search; the cases' largest WHOLE GAME needs 177,525 nodes (host build): a defect ends as LIMIT
DEFAULT, WB = play_cases.DEFAULT, search_ref.WEIGHTS_B
FULL = (1 << 64) - 1
KEYS = ("a_black", "final_boards", "diff", "plies", "moves", "status", "hist")


def dev_starts(boards, turn):
    b = None if boards is None else ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")
    t = None if turn is None else torch.from_numpy(np.array(turn, np.uint8)).cuda()
    return b, t


def gpu_play(n, seed, boards=None, turn=None, node_limit=NODE_LIMIT, **kw):
    """ops.play's result as a dict of numpy arrays (nodes as uint64)."""
    b, t = dev_starts(boards, turn)
    r = ops.play(n, seed, start=b, start_turn=t, record_moves=True, node_limit=node_limit, want_nodes=True, **kw)
    torch.cuda.synchronize()
    out = {k: getattr(r, k).cpu().numpy() for k in ("a_black", "diff", "plies", "moves", "status", "hist")}
    out["final_boards"] = ops.to_numpy_u64(r.final_boards).reshape(-1, 2)
    out["nodes"] = r.nodes.cpu().numpy().view(np.uint64)
    return out


def play_case(case, **kw):
    c = play_cases.CASES[case]
    b, t = play_cases.starts(case)
    args = dict(game_id0=c["game_id0"], weights_a=play_cases.TABLES[c["tables"][0]],
                weights_b=play_cases.TABLES[c["tables"][1]], depth_a=c["depth"][0], depth_b=c["depth"][1],
                exact_empties=c["exact"], n_rand_a=c["n_rand"][0], n_rand_b=c["n_rand"][1], swap_colours=c["swap"])
    args.update(kw)
    return gpu_play(c["n"], c["seed"], b, t, **args)


def assert_same_games(got, ref, keys=KEYS, where=None):
    for k in keys:
        a, b = (got[k], ref[k]) if where is None or k == "hist" else (got[k][where], ref[k][where])
        bad = np.nonzero(np.asarray(a != b).reshape(len(a), -1).any(1))[0]
        assert len(bad) == 0, (k, bad[:8], a[bad[:4]], b[bad[:4]])


# ---------------------------------------------------------------- the checker
@pytest.mark.parametrize("case", sorted(play_cases.CASES))
def test_games_match_the_checker(case):
    """Colours, final boards, diff, plies, every move byte, status and the
    histogram: depths (3, 2) and (2, 3) from 64 midgame starts, (3, 3) from the
    opening with budgets (3, 12) (coins, passes, both colour assignments),
    (4, 1), (5, 2), the extreme table, and the exact endgame."""
    got = play_case(case)
    ref = play_cases.reference(case)
    assert (got["status"] == SEARCHED).all()
    assert_same_games(got, ref)
    assert ops.work_word("cuda").item() == 0
    c = play_cases.CASES[case]
    if c["swap"] and c["n"] >= 32:
        assert 0 < int(got["a_black"].sum()) < c["n"]
    if case == "open32_d3v3":
        assert (got["moves"] == 64).any()  # a pass was played somewhere


def test_exact_endgame_plays_the_solvers_value():
    """With exact_empties = 8 and no random moves both sides play perfectly
    from the first position with at most eight empties on: the solver's value
    there, from its mover's side, is the game's final disc difference.  Without
    it at least one game ends otherwise."""
    got = play_case("mid64_d2v3_exact8")
    plain = play_cases.reference("mid64_d2v3")
    assert (got["final_boards"] != plain["final_boards"]).any()
    b, t = dev_starts(*play_cases.starts("mid64_d2v3_exact8"))
    rp = ops.replay(torch.from_numpy(got["moves"]).cuda(), torch.from_numpy(got["plies"]).cuda(), b, t)
    pos, turn = ops.to_numpy_u64(rp.boards), rp.turn.cpu().numpy()
    n = len(got["plies"])
    first = np.zeros(n, np.int64)
    for g in range(n):
        emp = [64 - bin(int(x[0] | x[1])).count("1") for x in pos[g, :int(got["plies"][g]) + 1]]
        first[g] = next(p for p, e in enumerate(emp) if e <= 8)
    pb, pt = pos[np.arange(n), first], turn[np.arange(n), first]
    assert pt.min() >= 1 and pt.max() <= 2
    sv = ops.solve(ops.from_numpy_u64(pb, "cuda"), torch.from_numpy(pt).cuda(), max_empties=8, node_limit=NODE_LIMIT)
    assert (sv.status.cpu().numpy() == _lib.SOLVE_SOLVED).all()
    want = got["diff"].astype(np.int64) * np.where(pt == 1, 1, -1)
    assert (sv.value.cpu().numpy().astype(np.int64) == want).all()


# ---------------------------------------------------------------- composition
def host_loop(b0, t0, wa, wb, da, db):
    """The parent's route to the same games, A on Black: one ops.search per
    table and one ops.step per ply over the whole batch.  The search's move is
    the rule's on every turn: 255 when the game is over, 64 on a forced pass,
    the only move where there is one (all asserted)."""
    b, t = b0.clone(), t0.clone()
    n = len(t)
    moves = torch.full((n, ops.MOVES_STRIDE), 255, dtype=torch.uint8, device="cuda")
    plies = torch.zeros(n, dtype=torch.int64, device="cuda")
    live = torch.ones(n, dtype=torch.bool, device="cuda")
    rows = torch.arange(n, device="cuda")
    for _ in range(130):
        ra = ops.search(b, t, da, weights=wa, node_limit=NODE_LIMIT)
        rb = ops.search(b, t, db, weights=wb, node_limit=NODE_LIMIT)
        assert bool((ra.status == SEARCHED).all() and (rb.status == SEARCHED).all())
        mv = torch.where(t == 1, ra.best_move, rb.best_move)
        live = live & (mv != 255)
        if not bool(live.any()):
            break
        own = ops.legal(b, t)
        assert bool(((mv == 64) == (own == 0))[live].all())
        single = live & (own != 0) & ((own & (own - 1)) == 0)
        assert bool(((torch.ones_like(own) << mv.long().clamp(max=63)) == own)[single].all())
        st = ops.step(b, t, torch.where(live, mv, torch.full_like(mv, 64)))
        assert bool((st.ret[live] >= 0).all())
        b = torch.where(live[:, None], st.boards, b)
        t = torch.where(live, st.turn, t)
        moves[rows[live], plies[live]] = mv[live]
        plies += live
    assert not bool(live.any())
    return b, plies, moves


def test_kernel_equals_a_host_loop_of_search_and_step():
    g = play_cases.midgame()
    n = 4097
    b0, t0 = dev_starts(g["boards"][:n], g["turn"][:n])
    r = ops.play(n, 1, weights_a=DEFAULT, weights_b=WB, depth_a=3, depth_b=2, start=b0, start_turn=t0,
                 record_moves=True, node_limit=NODE_LIMIT)
    hb, hp, hm = host_loop(b0, t0, DEFAULT, WB, 3, 2)
    assert bool((r.status == SEARCHED).all() and (r.a_black == 1).all())
    assert torch.equal(r.final_boards, hb) and torch.equal(r.plies.long(), hp) and torch.equal(r.moves, hm)


# ---------------------------------------------------------------- depth 1
def test_depth_1_is_the_eval_runner_until_a_move_can_end_the_game():
    """Depth 1 scores a child by the mover's eval -- the 1-ply eval policy --
    unless the child ends the game, which outranks any eval (othello_search.h,
    rule 1).  So a game may leave the eval runner's only at a ply whose mover
    has a child that ends the game."""
    n, seed = 4096, 31
    e = ops.rollout_runner(n, seed, 50, "eval", DEFAULT, WB, 3, 12, True, record_moves=True)
    got = gpu_play(n, seed, game_id0=50, weights_a=DEFAULT, weights_b=WB, depth_a=1, depth_b=1, n_rand_a=3,
                   n_rand_b=12, swap_colours=True)
    em, ep = e.moves.cpu().numpy(), e.plies.cpu().numpy()
    assert (got["a_black"] == e.a_black.cpu().numpy()).all() and (got["status"] == SEARCHED).all()
    differs = (got["moves"] != em).any(1)
    same = ~differs
    assert same.sum() >= 1
    assert (got["final_boards"][same] == ops.to_numpy_u64(e.final_boards).reshape(-1, 2)[same]).all()
    assert (got["plies"][same] == ep[same]).all() and (got["diff"][same] == e.diff.cpu().numpy()[same]).all()
    idx = np.nonzero(differs)[0]
    if len(idx):
        rp = oracle.replay(em[idx], ep[idx])
        for k, g in enumerate(idx):
            p = int(np.nonzero(got["moves"][g] != em[g])[0][0])
            assert p < ep[g]
            b, t = rp["boards"][k, p:p + 1], rp["turn"][k, p:p + 1]
            sq = np.array([s for s in range(64) if int(oracle.legal(b, t)[0]) >> s & 1], np.uint8)
            child = oracle.step(np.repeat(b, len(sq), 0), np.repeat(t, len(sq)), sq)["boards"]
            over = (oracle.legal(child, np.full(len(sq), 1, np.uint8)) == 0) & (
                oracle.legal(child, np.full(len(sq), 2, np.uint8)) == 0)
            assert over.any(), (g, p)


# ---------------------------------------------------------------- the contract
def mid_args(**kw):
    a = dict(game_id0=11, weights_a=DEFAULT, weights_b=WB, depth_a=2, depth_b=2, swap_colours=True)
    a.update(kw)
    return a


@functools.lru_cache(maxsize=None)
def big():
    """4,097 depth-2 games from the midgame starts, once: the batch the other
    sizes and splits are compared with."""
    g = play_cases.midgame()
    r = gpu_play(4097, 7, g["boards"], g["turn"], **mid_args())
    for v in r.values():
        v.setflags(write=False)
    return r


def test_the_big_batchs_first_games_match_the_checker():
    g = play_cases.midgame()
    ref = play_ref.play(65, 7, play_ref.search_chooser(DEFAULT, WB, 2, 2), game_id0=11, swap=True,
                        start=g["boards"][:65], start_turn=g["turn"][:65])
    r = big()
    assert (r["status"] == SEARCHED).all()
    assert_same_games(r, ref, keys=("a_black", "final_boards", "diff", "plies", "moves"), where=slice(0, 65))
    assert (r["hist"] == play_ref.histogram(r["diff"], r["plies"])).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(n):
    g = play_cases.midgame()
    r = gpu_play(n, 7, g["boards"][:n], g["turn"][:n], **mid_args())
    assert_same_games(r, big(), keys=KEYS[:-1] + ("nodes",), where=slice(0, n))
    assert (r["hist"] == play_ref.histogram(r["diff"], r["plies"])).all()
    assert ops.work_word("cuda").item() == 0


def test_results_do_not_depend_on_the_split_or_the_order():
    g = play_cases.midgame()
    one = big()
    cuts = [0, 100, 500, 777]
    parts = [gpu_play(hi - lo, 7, g["boards"][lo:hi], g["turn"][lo:hi], **mid_args(game_id0=11 + lo))
             for lo, hi in zip(cuts, cuts[1:])]
    for k in KEYS[:-1] + ("nodes",):
        assert (np.concatenate([p[k] for p in parts]) == one[k][:777]).all(), k
    assert (sum(p["hist"] for p in parts) == play_ref.histogram(one["diff"][:777], one["plies"][:777])).all()
    # a game's draws follow its id: single games launched in another order, each with its id and start
    perm = np.random.default_rng(5).permutation(777)[:12]
    for i in perm:
        r = gpu_play(1, 7, g["boards"][i:i + 1], g["turn"][i:i + 1], **mid_args(game_id0=11 + int(i)))
        for k in KEYS[:-1] + ("nodes",):
            assert (r[k][0] == one[k][i]).all(), (k, i)


def test_a_permutation_of_the_starts_without_draws():
    """No swap and no budgets: a game makes no draw, so it depends on its start
    alone and a permuted batch plays the permuted games."""
    g = play_cases.midgame()
    b, t = g["boards"][:777], g["turn"][:777]
    a = gpu_play(777, 7, b, t, **mid_args(swap_colours=False))
    perm = np.random.default_rng(6).permutation(777)
    p = gpu_play(777, 99, b[perm], t[perm], **mid_args(swap_colours=False, game_id0=0))
    for k in KEYS[:-1] + ("nodes",):
        assert (p[k] == a[k][perm]).all(), k
    assert (p["hist"] == a["hist"]).all()


def test_one_block_refills_through_the_whole_batch(monkeypatch):
    g = play_cases.midgame()
    assert _lib.load().othp_play_grid(1000) == 16
    monkeypatch.setenv("OTH_PLAY_BLOCKS", "1")
    assert _lib.load().othp_play_grid(1000) == 1
    r = gpu_play(1000, 7, g["boards"][:1000], g["turn"][:1000], **mid_args())
    assert ops.work_word("cuda").item() == 0
    assert_same_games(r, big(), keys=KEYS[:-1] + ("nodes",), where=slice(0, 1000))


def test_work_word_is_shared_with_a_rollout_a_solve_and_a_search_and_left_zero():
    g = play_cases.midgame()
    b, t = dev_starts(g["boards"][:333], g["turn"][:333])
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    kw = dict(start=b, start_turn=t, node_limit=NODE_LIMIT, **mid_args())
    r1 = ops.play(333, 7, work=w, **kw)  # two launches back to back on one word
    r2 = ops.play(333, 7, work=w, **kw)
    torch.cuda.synchronize()
    assert w.item() == 0 and r1.nodes is None and r1.moves is None
    c = solve_cases.cases()[6]
    cb, ct = dev_starts(c["boards"], c["turn"])
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r3 = ops.play(333, 7, **kw)
    sv = ops.solve(cb, ct, max_empties=6, node_limit=NODE_LIMIT)
    r4 = ops.play(333, 7, **kw)
    se = ops.search(b, t, 3, node_limit=NODE_LIMIT)
    r5 = ops.play(333, 7, **kw)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    for r in (r1, r2, r3, r4, r5):
        assert (ops.to_numpy_u64(r.final_boards).reshape(-1, 2) == big()["final_boards"][:333]).all()
        assert (r.plies.cpu().numpy() == big()["plies"][:333]).all()
    assert (sv.value.cpu().numpy() == c["value"]).all() and bool((se.status == SEARCHED).all())
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)
    assert (ops.to_numpy_u64(g2.final_boards) == oracle.rollout(1000, 9)["final_boards"]).all()


def raw_play(lib, start, turn, outs, work, n, depth=(2, 2), exact=0, n_rand=(0, 0), wa="default", wb="default",
             seed=7, game_id0=11):
    """othp_play itself, colours drawn; outs: the eight outputs in the header's order."""
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    w = {"default": ops._weights_ptr(DEFAULT), "rng7": ops._weights_ptr(WB), None: None}
    return lib.othp_play(ptr(start), ptr(turn), seed, game_id0, w[wa], w[wb], depth[0], depth[1], exact, n_rand[0],
                         n_rand[1], 1, NODE_LIMIT, *[ptr(o) for o in outs], ptr(work), n,
                         torch.cuda.current_stream().cuda_stream)


def test_null_outputs_null_start_and_null_turn():
    g = play_cases.midgame()
    n = 300
    b, t = dev_starts(g["boards"][:n], g["turn"][:n])
    lib, w = _lib.load(), ops.work_word("cuda")
    none = [None] * 8
    assert raw_play(lib, b, t, none, w, n, wb="rng7") == 0  # every output NULL
    fb = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    assert raw_play(lib, b, t, [None, fb] + [None] * 6, w, n, wb="rng7") == 0  # one output at a time
    pl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert raw_play(lib, b, t, [None, None, None, pl] + [None] * 4, w, n, wb="rng7") == 0
    hist = torch.zeros(ops.HIST_BINS, dtype=torch.int64, device="cuda")
    assert raw_play(lib, b, t, [None] * 7 + [hist], w, n, wb="rng7") == 0
    assert raw_play(lib, b, t, [None] * 7 + [hist], w, n, wb="rng7") == 0  # accumulated
    torch.cuda.synchronize()
    one = big()
    assert (ops.to_numpy_u64(fb).reshape(-1, 2) == one["final_boards"][:n]).all()
    assert (pl.cpu().numpy() == one["plies"][:n]).all() and w.item() == 0
    assert (hist.cpu().numpy() == 2 * play_ref.histogram(one["diff"][:n], one["plies"][:n])).all()
    # start_turn NULL: Black to move everywhere; start NULL: the opening
    fb1, fb2 = torch.zeros_like(fb), torch.zeros_like(fb)
    assert raw_play(lib, b, None, [None, fb1] + [None] * 6, w, n, wb="rng7") == 0
    assert raw_play(lib, None, None, [None, fb2] + [None] * 6, w, n, wb="rng7") == 0
    torch.cuda.synchronize()
    black = gpu_play(n, 7, g["boards"][:n], np.ones(n, np.uint8), **mid_args())
    opening = gpu_play(n, 7, **mid_args())
    assert (ops.to_numpy_u64(fb1).reshape(-1, 2) == black["final_boards"]).all()
    assert (ops.to_numpy_u64(fb2).reshape(-1, 2) == opening["final_boards"]).all()
    # start_turn without start is not read: the opening, Black to move
    fb3 = torch.zeros_like(fb)
    assert raw_play(lib, None, t, [None, fb3] + [None] * 6, w, n, wb="rng7") == 0
    torch.cuda.synchronize()
    assert (ops.to_numpy_u64(fb3).reshape(-1, 2) == opening["final_boards"]).all() and w.item() == 0


def test_empty_batch_bad_arguments_and_overlap():
    r = ops.play(0, 1, record_moves=True, want_nodes=True)
    assert r.final_boards.shape == (0, 2) and r.moves.shape == (0, ops.MOVES_STRIDE) and r.nodes.dtype == torch.int64
    assert int(r.hist.sum()) == 0
    lib = _lib.load()
    assert lib.othp_play_grid(0) == 0 and lib.othp_play_grid(-1) == _lib.OTH_EINVAL
    assert lib.othp_play_grid(1) == 1 and lib.othp_play_grid(65) == 2
    assert 2 <= lib.othp_play_grid(1 << 30) <= 1 << 20
    for bad in (dict(depth_a=0), dict(depth_a=9), dict(depth_a=2, depth_b=0), dict(depth_a=2, depth_b=9),
                dict(exact_empties=-1), dict(exact_empties=9), dict(n_rand_a=-1), dict(n_rand_b=-1)):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.play(4, 1, **bad)
    w = ops.work_word("cuda")
    none = [None] * 8
    assert raw_play(lib, None, None, none, w, 4, wa=None) == _lib.OTH_EINVAL  # NULL weights
    assert raw_play(lib, None, None, none, w, 4, wb=None) == _lib.OTH_EINVAL
    assert raw_play(lib, None, None, none, None, 4) == _lib.OTH_EINVAL  # no work word
    assert raw_play(lib, None, None, none, w, -1) == _lib.OTH_EINVAL
    with pytest.raises(ValueError, match="32 bits"):
        ops.play(4, 1, node_limit=1 << 32)
    # the failed calls launched nothing and the stream's next launch finds a zero word
    g = play_cases.midgame()
    r = gpu_play(4, 7, g["boards"][:4], g["turn"][:4], **mid_args())
    assert_same_games(r, big(), keys=KEYS[:-1], where=slice(0, 4))
    assert ops.work_word("cuda").item() == 0
    # a budget above 10 plays as 10
    a = gpu_play(64, 3, depth_a=2, n_rand_a=10, n_rand_b=37, swap_colours=True)
    b = gpu_play(64, 3, depth_a=2, n_rand_a=10, n_rand_b=10, swap_colours=True)
    assert (a["moves"] == b["moves"]).all()
    # overlapping starts are INVALID beside played neighbours
    rows = np.array([[FULL ^ 0xF, 0x10], g["boards"][0], [FULL, FULL], g["boards"][1]], np.uint64)
    turn = np.array([1, g["turn"][0], 2, g["turn"][1]], np.uint8)
    r = gpu_play(4, 7, rows, turn, **mid_args(game_id0=10))
    assert r["status"].tolist() == [INVALID, SEARCHED, INVALID, SEARCHED]
    assert (r["final_boards"][[0, 2]] == rows[[0, 2]]).all() and r["plies"][[0, 2]].tolist() == [0, 0]
    assert r["diff"][[0, 2]].tolist() == [0, 0] and r["a_black"][[0, 2]].tolist() == [1, 1]
    assert r["nodes"][[0, 2]].tolist() == [0, 0] and (r["moves"][[0, 2]] == 255).all()
    assert (r["moves"][1] == big()["moves"][0]).all()  # id 11, start 0: the big batch's game 0
    ref = play_ref.play(4, 7, play_ref.search_chooser(DEFAULT, WB, 2, 2), game_id0=10, swap=True, start=rows,
                        start_turn=turn)
    assert_same_games(r, ref)
    assert r["hist"][129:132].sum() == 2


def test_nodes_are_reproducible():
    one = big()
    g = play_cases.midgame()
    again = gpu_play(500, 7, g["boards"][:500], g["turn"][:500], **mid_args())
    assert (again["nodes"] == one["nodes"][:500]).all() and one["nodes"].min() > 0


# ---------------------------------------------------------------- the node limit
def test_node_limit_stops_exactly_the_games_that_need_more():
    """Each game's largest single search, from ops.search over the unlimited
    run's recorded positions; with a limit at the median of those, exactly the
    games above it stop, at the first position whose search needs more, with the
    unlimited game's moves up to there; the others are unchanged and the
    histogram counts only them."""
    case = "mid64_d3v2"
    c = play_cases.CASES[case]
    full = play_case(case)
    assert (full["status"] == SEARCHED).all()
    n = c["n"]
    b, t = dev_starts(*play_cases.starts(case))
    rp = ops.replay(torch.from_numpy(full["moves"]).cuda(), torch.from_numpy(full["plies"]).cuda(), b, t)
    pb, pt = rp.boards.reshape(-1, 2).contiguous(), rp.turn.reshape(-1).contiguous()
    nodes = []
    for d, tab in zip(c["depth"], c["tables"]):
        r = ops.search(pb, pt, d, weights=play_cases.TABLES[tab], node_limit=NODE_LIMIT, want_nodes=True)
        nodes.append(r.nodes.cpu().numpy().view(np.uint32).astype(np.int64).reshape(n, -1))
    own = ops.to_numpy_u64(ops.legal(pb, pt)).reshape(n, -1)
    turn = pt.cpu().numpy().reshape(n, -1)
    searched = (own & (own - np.uint64(1))) != 0  # two legal moves or more (budgets are 0: no coin)
    searched &= np.arange(turn.shape[1])[None, :] < full["plies"][:, None]
    a_moves = (turn == 1) == (full["a_black"][:, None] == 1)
    need = np.where(searched, np.where(a_moves, nodes[0], nodes[1]), 0)
    limit = int(np.median(need.max(1)))
    assert 0 < limit <= NODE_LIMIT
    stop = need.max(1) > limit
    assert 0 < stop.sum() < n
    got = play_case(case, node_limit=limit)
    assert (got["status"] == np.where(stop, LIMIT, SEARCHED)).all()
    assert_same_games(got, full, keys=("a_black", "final_boards", "diff", "plies", "moves", "nodes"), where=~stop)
    pos = ops.to_numpy_u64(rp.boards)
    for g in np.nonzero(stop)[0]:
        p = int(np.nonzero(need[g] > limit)[0][0])
        assert got["plies"][g] == p and got["a_black"][g] == full["a_black"][g]
        assert (got["moves"][g, :p] == full["moves"][g, :p]).all() and (got["moves"][g, p:] == 255).all()
        assert (got["final_boards"][g] == pos[g, p]).all()
        assert got["diff"][g] == bin(int(pos[g, p, 0])).count("1") - bin(int(pos[g, p, 1])).count("1")
    assert (got["hist"] == play_ref.histogram(full["diff"][~stop], full["plies"][~stop])).all()
    # a limit of exactly the largest need stops nothing
    top = play_case(case, node_limit=int(need.max()))
    assert (top["status"] == SEARCHED).all() and (top["moves"] == full["moves"]).all()


# ---------------------------------------------------------------- the runner
def test_do_matches_with_searching_players():
    conf = {"proc_n_rand_hands_for_a": 2, "proc_n_rand_hands_for_b": 3, "proc_randomize_black_white": 1}
    wa = np.random.default_rng(8).integers(-100, 100, (4, 9)).astype(np.int8)
    n = 256
    mb = runner.do_matches(conf, wa, n=n, seed=17, game_id0=300, weights_b=WB, policy="search", depth=(3, 1),
                           exact_empties=6)
    r = mb.games
    direct = gpu_play(n, 17, game_id0=300, weights_a=wa, weights_b=WB, depth_a=3, depth_b=1, exact_empties=6,
                      n_rand_a=2, n_rand_b=3, swap_colours=True, node_limit=0)
    fin = ops.to_numpy_u64(r.final_boards).reshape(-1, 2)
    assert (fin == direct["final_boards"]).all() and (r.moves.cpu().numpy() == direct["moves"]).all()
    plies, diff = r.plies.cpu().numpy(), r.diff.cpu().numpy().astype(int)
    rp = oracle.replay(r.moves.cpu().numpy(), plies)  # the books' moves re-driven give the final boards
    assert (rp["boards"][np.arange(n), plies] == fin).all() and (rp["end"][np.arange(n), plies] == 1).all()
    line_a = "Hamlet policy=search depth=3 weights=%s solve_empties=6" % wa.reshape(-1).tolist()
    assert runner.hamlet_param_line("Hamlet", "search", wa, 3, 6) == line_a
    assert runner.hamlet_param_line("GPU", "search", WB, 1, 0) == "GPU policy=search depth=1 weights=%s" % (
        WB.reshape(-1).tolist())
    assert 0 < int(mb.a_black.sum()) < n
    for g in range(n):
        ab = bool(mb.a_black[g])
        assert mb.meta[g] == {"proc_a": "Hamlet" if ab else "GPU", "proc_b": "GPU" if ab else "Hamlet",
                              "hamletparam": line_a}
        d = diff[g]
        assert d == bin(int(fin[g, 0])).count("1") - bin(int(fin[g, 1])).count("1")
        assert mb.won[g] == (("Black", mb.meta[g]["proc_a"]) if d > 0 else
                             (("White", mb.meta[g]["proc_b"]) if d < 0 else ("None", "")))
    for g in (0, 1, n - 1):
        recs = mb.books.records(g)
        assert recs[-1]["end"] and len(recs) == int(plies[g]) + 1
    from oracle import batch_stats as ref_stats
    books = [(300 + g, [{"book": mb.books.records(g)[-1]["book"], "whosturn": mb.books.records(g)[-1]["whosturn"],
                         "turn": int(plies[g]), "end": True}], mb.meta[g]) for g in range(n)]
    assert mb.stats == ref_stats.store_batch_stats(books, reference_rule=True)
    w, l, dr = runner.wins_of_a(mb)
    assert w + l + dr == n
    sign = np.where(mb.a_black, 1, -1) * np.sign(diff)
    assert (w, l, dr) == ((sign > 0).sum(), (sign < 0).sum(), (sign == 0).sum())
    # the 1-ply policies' calls are as they were
    with pytest.raises(ValueError):
        runner.do_matches(conf, wa, n=4, policy="eval", depth=3)
    with pytest.raises(ValueError):
        runner.do_matches(conf, wa, n=4, policy="search")
