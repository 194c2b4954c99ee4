"""ops.solve_line / ops.search_line (include/othello_line.h) on
the GPU against tests/line_ref.py's walk over the oracle: the line of best play
behind a value from the exact solver and from the depth-limited search, its
agreement with ops.solve / ops.search, deep lines against the existing calls,
the node limit, depths per position, the launch plumbing, and what is built on
them (the VecEnv methods, the engine's `pv`).  All comparisons are exact."""
import numpy as np
import pytest
import torch

import host_programs as hp
import line_ref
import oracle
import solve_cases
import solve_ref
import tree_cases
from test_line_host import run_search, run_solve, same_line

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402
from subproc_amd.engine import Engine  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

SOLVED, SKIPPED, INVALID, LIMIT = _lib.SOLVE_SOLVED, _lib.SOLVE_SKIPPED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
BADDEPTH = _lib.LINE_BADDEPTH
T = line_ref.T
FIELDS = ("line", "length", "value", "best_move", "status", "nodes", "end_boards", "end_turn")
# as tests/test_gpu_solve.py: no tree of the pool at <= 9 empties needs more than 23,082 nodes
LIMIT_9 = 1 << 18


def test_the_constants_are_the_headers():
    assert (_lib.LINE_STRIDE, _lib.LINE_BADDEPTH) == (line_ref.STRIDE, 6)
    assert _lib.SEARCH_SEARCHED == SOLVED and _lib.SEARCH_LIMIT == LIMIT and _lib.SEARCH_INVALID == INVALID


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def unpack(r):
    torch.cuda.synchronize()
    out = {k: getattr(r, k).cpu().numpy().astype(np.int64) for k in FIELDS if k not in ("nodes", "end_boards")}
    out["nodes"] = None if r.nodes is None else r.nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    out["end_boards"] = ops.to_numpy_u64(r.end_boards)
    return out


def gpu_solve_line(boards, turn, **kw):
    return unpack(ops.solve_line(*dev(boards, turn), want_nodes=True, **kw))


def gpu_search_line(boards, turn, depth, weights, **kw):
    return unpack(ops.search_line(*dev(boards, turn), depth, weights=weights, want_nodes=True, **kw))


def same_all(a, b, what, rows=slice(None)):
    for k in FIELDS:
        assert (a[k][rows] == b[k][rows]).all(), (what, k)


def assert_padded(got):
    """Entries below the length are move codes, the rest is 255."""
    col = np.arange(line_ref.STRIDE)[None, :]
    inside = col < got["length"][:, None]
    assert (got["line"][inside] <= 64).all() and (got["line"][~inside] == 255).all()


def replay(boards, turn, got):
    """Every line through oracle.step, legal move by move: (i, k, boards, turn) of every prefix position (the
    position in front of entry k of line i), and the end positions."""
    b = np.array(boards, np.uint64).reshape(-1, 2)
    t = solve_ref.mover(turn).copy()
    pi, pk, pb, pt = [], [], [], []
    for k in range(int(got["length"].max(initial=0))):
        act = np.nonzero(got["length"] > k)[0]
        mv = got["line"][act, k]
        own = oracle.legal(b[act], t[act])
        opp = oracle.legal(b[act], (3 - t[act]).astype(np.uint8))
        is_pass = mv == 64
        assert ((own[is_pass] == 0) & (opp[is_pass] != 0)).all()
        sq = np.minimum(mv[~is_pass], 63).astype(np.uint64)
        assert (mv[~is_pass] < 64).all() and (((own[~is_pass] >> sq) & np.uint64(1)) == 1).all()
        pi.append(act), pk.append(np.full(len(act), k)), pb.append(b[act].copy()), pt.append(t[act].copy())
        st = oracle.step(b[act], t[act], mv.astype(np.uint8))
        assert (st["ret"] >= 0).all() and ((st["ret"] == 0) == is_pass).all()
        b[act], t[act] = st["boards"], 3 - t[act]
    cat = [np.concatenate(x) if x else np.zeros((0,) + s, d) for x, s, d in
           ((pi, (), np.int64), (pk, (), np.int64), (pb, (2,), np.uint64), (pt, (), np.uint8))]
    return cat, b, t


def assert_replays(boards, turn, got, weights=None, rows=None):
    """The line is legal move by move, ends at end_boards / end_turn, and the end position's static score from the
    root mover's side is the value."""
    rows = np.ones(len(turn), bool) if rows is None else rows
    _, eb, et = replay(boards, turn, got)
    assert (eb[rows] == got["end_boards"][rows]).all() and (et[rows] == got["end_turn"][rows]).all()
    assert (line_ref.end_score(eb[rows], np.asarray(turn)[rows], weights) == got["value"][rows]).all()


# ---------------------------------------------------------------- exact lines
def exact_batch(hi=9):
    b, t = line_ref.exact_inputs(0, hi)
    cs = solve_cases.cases()
    assert len(t) == sum(len(cs[e]["turn"]) for e in range(hi + 1))  # no position dropped
    forced = np.concatenate([cs[e]["forced_pass"] for e in range(hi + 1)])
    over = np.concatenate([cs[e]["over"] for e in range(hi + 1)])
    assert forced.any() and over.any()  # the forced-pass and finished roots are in the set
    return b, t, forced, over


def test_exact_lines_of_every_position_at_0_to_9_empties():
    b, t, forced, over = exact_batch()
    got = gpu_solve_line(b, t, max_empties=9, node_limit=LIMIT_9)
    assert (got["status"] == SOLVED).all()
    same_line(got, line_ref.exact_cases(0, 9), "exact")
    assert_padded(got)
    assert (got["line"][forced, 0] == 64).all() and (got["length"][over] == 0).all()
    assert (got["best_move"][over] == 255).all() and (got["nodes"][over] == 0).all()
    assert (got["nodes"][forced] >= 1).all() and got["length"].max() >= 10
    # value, best_move and status are ops.solve's on the same batch, overlapping and skipped boards included
    b2 = np.concatenate([b, np.array([[0xFF, 0x81], [(1 << 64) - 1, (1 << 64) - 1]], np.uint64)])
    t2 = np.concatenate([t, np.array([1, 2], np.uint8)])
    bt, tt = dev(b2, t2)
    for max_empties in (9, 6):
        r = unpack(ops.solve_line(bt, tt, max_empties=max_empties, node_limit=LIMIT_9, want_nodes=True))
        s = ops.solve(bt, tt, max_empties=max_empties, node_limit=LIMIT_9)
        for k in ("value", "best_move", "status"):
            assert (r[k] == getattr(s, k).cpu().numpy()).all(), (max_empties, k)
        off = r["status"] != SOLVED
        assert (r["status"][-2:] == INVALID).all() and ((r["status"] == SKIPPED).sum() > 0) == (max_empties == 6)
        assert (r["length"][off] == 0).all() and (r["line"][off] == 255).all() and (r["nodes"][off] == 0).all()
        assert (r["end_boards"][off] == b2[off]).all() and (r["end_turn"][off] == t2[off]).all()
        same_all(r, got, max_empties, np.nonzero(~off)[0])
    assert_replays(b, t, got)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- search lines
SEARCH_CASES = [(name, d) for name in ("mid3", "mid4", "special3") for d in (1, 2, 3, 4)] + [("mid5", 5)]


@pytest.mark.parametrize("name,depth", SEARCH_CASES)
def test_search_lines_are_the_walk_over_the_oracle(name, depth):
    b, t = tree_cases.inputs(name)
    bt, tt = dev(b, t)
    for table in tree_cases.BOTH:
        w = tree_cases.TABLES[table]
        want = line_ref.search_case(name, depth, table)
        s = ops.search(bt, tt, depth, weights=w)
        for order in (0, 1):
            got = unpack(ops.search_line(bt, tt, depth, weights=w, order=order, want_nodes=True))
            assert (got["status"] == SOLVED).all()
            same_line(got, want, (name, depth, table, order))
            assert_padded(got)
            for k in ("value", "best_move", "status"):
                assert (got[k] == getattr(s, k).cpu().numpy()).all(), (name, depth, table, order, k)
            assert_replays(b, t, got, w)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("empties", [6, 8])
def test_depth_eight_is_the_exact_line(empties):
    cs = solve_cases.cases()
    lo = sum(len(cs[e]["turn"]) for e in range(empties))
    k = 48 if empties == 6 else 24
    b, t = cs[empties]["boards"][:k], cs[empties]["turn"][:k]
    want = {f: v[lo:lo + k] for f, v in line_ref.exact_cases(0, 9).items()}
    for order, table in ((0, "default"), (1, "rng7")):
        got = gpu_search_line(b, t, 8, tree_cases.TABLES[table], order=order)
        assert (got["status"] == SOLVED).all()
        same_line(got, want, (empties, order), scale=T)
    e = gpu_solve_line(b, t)
    assert (e["line"] == got["line"]).all() and (T * e["value"] == got["value"]).all()


# ---------------------------------------------------------------- deep lines against the existing calls
def test_deep_exact_lines_against_ops_solve_at_every_ply():
    parts = [solve_cases.ladder(11, 16), solve_cases.ladder(12, 4)]
    b, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(t) == 20
    got = gpu_solve_line(b, t)
    assert (got["status"] == SOLVED).all()  # none may be LIMIT
    assert_padded(got)
    assert_replays(b, t, got)
    (pi, pk, pb, pt), _, _ = replay(b, t, got)
    s = ops.solve(*dev(pb, pt))
    torch.cuda.synchronize()
    assert (s.status.cpu().numpy() == SOLVED).all()
    sign = np.where(pt == solve_ref.mover(t)[pi], 1, -1)
    assert (s.value.cpu().numpy().astype(np.int64) == sign * got["value"][pi]).all()
    assert (s.best_move.cpu().numpy() == got["line"][pi, pk]).all()
    assert len(pi) == got["length"].sum() and got["length"].max() >= 12 and (got["length"] >= 8).all()


@pytest.mark.parametrize("order", [0, 1])
def test_deep_search_lines_against_ops_search_where_the_root_side_moves(order):
    b, t = tree_cases.inputs("mid5")
    w = tree_cases.TABLES["rng7"]
    got = gpu_search_line(b, t, 7, w, order=order)
    assert (got["status"] == SOLVED).all() and got["length"].max() >= 7
    assert_replays(b, t, got, w)
    (pi, pk, pb, pt), _, _ = replay(b, t, got)
    moves_before = np.array([(got["line"][i, :k] != 64).sum() for i, k in zip(pi, pk)])
    rem = 7 - moves_before
    mine = pt == solve_ref.mover(t)[pi]
    assert mine.sum() >= 3 * len(t) and (rem >= 1).all()
    for d in np.unique(rem[mine]):
        sel = mine & (rem == d)
        s = ops.search(*dev(pb[sel], pt[sel]), int(d), weights=w, order=order)
        torch.cuda.synchronize()
        assert (s.value.cpu().numpy() == got["value"][pi[sel]]).all(), (order, d)
        assert (s.best_move.cpu().numpy() == got["line"][pi[sel], pk[sel]]).all(), (order, d)


# ---------------------------------------------------------------- node limit
def assert_all_or_nothing(got, free, existing_status, what):
    cut = got["status"] == LIMIT
    assert cut.any() and (~cut).any(), what
    assert (got["length"][cut] == 0).all() and (got["value"][cut] == 0).all(), what
    assert (got["best_move"][cut] == 255).all() and (got["line"][cut] == 255).all(), what
    # every root the existing call resolves is resolved here, with the line it has without a limit
    assert (got["status"] == existing_status).all(), what
    same_all(got, free, what, np.nonzero(~cut)[0])


def test_node_limit_is_all_or_nothing_and_resolves_what_the_existing_calls_resolve():
    c = solve_cases.cases()[8]
    b, t = c["boards"], c["turn"]
    bt, tt = dev(b, t)
    n0 = ops.solve(bt, tt, want_nodes=True).nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    limit = int(np.median(n0[n0 > 0]))
    existing = ops.solve(bt, tt, node_limit=limit).status.cpu().numpy()
    assert_all_or_nothing(gpu_solve_line(b, t, node_limit=limit), gpu_solve_line(b, t), existing, "exact")
    b, t = tree_cases.inputs("mid4")
    bt, tt = dev(b, t)
    w = tree_cases.TABLES["default"]
    n0 = ops.search(bt, tt, 4, weights=w, want_nodes=True).nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    limit = int(np.median(n0))
    existing = ops.search(bt, tt, 4, weights=w, node_limit=limit).status.cpu().numpy()
    assert_all_or_nothing(gpu_search_line(b, t, 4, w, node_limit=limit), gpu_search_line(b, t, 4, w), existing,
                          "search")
    # ordered: all or nothing likewise (which roots are cut is the ordered tree's business)
    got = gpu_search_line(b, t, 4, w, order=1, node_limit=limit // 2)
    cut = got["status"] == LIMIT
    assert cut.any() and (got["length"][cut] == 0).all() and (got["line"][cut] == 255).all()
    assert (got["value"][cut] == 0).all() and (got["best_move"][cut] == 255).all()
    same_all(got, gpu_search_line(b, t, 4, w, order=1), "ordered", np.nonzero(~cut)[0])


# ---------------------------------------------------------------- depths per position
def test_depth_as_a_tensor_and_the_budget_searchs_depths():
    lb, lt = solve_cases.ladder(10, 79)  # (10 empties: depth 8 stays small)
    assert len(lt) == 79
    b = np.concatenate([lb, np.array([[3, 1]], np.uint64)])  # (an overlapping board at the end)
    t = np.concatenate([lt, np.array([1], np.uint8)])
    w = tree_cases.TABLES["rng7"]
    depths = np.array([(0, 1, 2, 3, 4, 5, 6, 9, 7, 8)[i % 10] for i in range(len(t))], np.uint8)
    bt, tt = dev(b, t)
    for order in (0, 1):
        got = unpack(ops.search_line(bt, tt, torch.from_numpy(depths).cuda(), weights=w, order=order,
                                     want_nodes=True))
        want_status = np.where(depths == 0, LIMIT, np.where(depths == 9, BADDEPTH, SOLVED))
        want_status[-1] = INVALID
        assert (got["status"] == want_status).all()
        off = got["status"] != SOLVED
        assert (got["length"][off] == 0).all() and (got["value"][off] == 0).all() and (got["nodes"][off] == 0).all()
        assert (got["best_move"][off] == 255).all() and (got["line"][off] == 255).all()
        for d in range(1, 9):
            sel = np.nonzero((depths == d) & ~off)[0]
            one = gpu_search_line(b[sel], t[sel], d, w, order=order)
            for k in FIELDS:
                assert (got[k][sel] == one[k]).all(), (order, d, k)
    for budget in (32, 2048):
        r = ops.search_budget(bt, tt, budget, weights=w)
        got = unpack(ops.search_line(bt, tt, r.depth, weights=w))
        reached = r.depth.cpu().numpy()
        assert (got["value"] == r.value.cpu().numpy()).all() and (got["best_move"] == r.best_move.cpu().numpy()).all()
        assert (got["status"] == r.status.cpu().numpy()).all(), budget
        assert (got["length"][reached == 0] == 0).all() and (got["length"][reached > 0] >= 1).all()
        assert len(set(reached.tolist())) >= 2
    with pytest.raises(TypeError, match="uint8"):
        ops.search_line(bt, tt, torch.ones(len(t), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="depth must lie"):
        ops.search_line(bt, tt, 9)


# ---------------------------------------------------------------- batch sizes and launch behaviour
def cycle(n, pool):
    k = np.arange(n) % len(pool[1])
    return k, pool[0][k], pool[1][k]


def search_pool():
    g = tree_cases.midgame()
    return np.concatenate([g["boards"][:100], tree_cases.inputs("special3")[0]]), \
        np.concatenate([g["turn"][:100], tree_cases.inputs("special3")[1]])


@pytest.fixture(scope="module")
def search_pool_want():
    b, t = search_pool()
    return line_ref.search(b, t, 3, tree_cases.TABLES["rng7"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(n, search_pool_want):
    want = line_ref.exact_cases(0, 6)
    k, b, t = cycle(n, line_ref.exact_inputs(0, 6))
    assert len(t) == n
    got = gpu_solve_line(b, t, max_empties=6)
    assert (got["status"] == SOLVED).all()
    same_line(got, {f: v[k] for f, v in want.items()}, n)
    k, b, t = cycle(n, search_pool())
    for order in (0, 1):
        got = gpu_search_line(b, t, 3, tree_cases.TABLES["rng7"], order=order)
        assert (got["status"] == SOLVED).all()
        same_line(got, {f: v[k] for f, v in search_pool_want.items()}, (n, order))
    assert ops.work_word("cuda").item() == 0


def test_results_do_not_depend_on_the_batch_or_the_grid(monkeypatch):
    eb, et = line_ref.exact_inputs(0, 7)
    sb, st = search_pool()
    w = tree_cases.TABLES["rng7"]
    e0 = gpu_solve_line(eb, et, max_empties=7)
    s0 = [gpu_search_line(sb, st, 3, w, order=order) for order in (0, 1)]
    perm = np.random.default_rng(5).permutation(len(et))
    ep = gpu_solve_line(eb[perm], et[perm], max_empties=7)
    assert all((ep[k] == e0[k][perm]).all() for k in FIELDS)
    perm = np.random.default_rng(6).permutation(len(st))
    sp = gpu_search_line(sb[perm], st[perm], 3, w)
    assert all((sp[k] == s0[0][k][perm]).all() for k in FIELDS)
    full = _lib.load().othl_solve_line_grid(len(et))
    assert full > 1 and _lib.load().othl_search_line_grid(len(st), 1) > 1
    monkeypatch.setenv("OTH_SOLVE_BLOCKS", "1")
    monkeypatch.setenv("OTH_SEARCH_BLOCKS", "1")
    assert _lib.load().othl_solve_line_grid(len(et)) == 1 and _lib.load().othl_search_line_grid(len(st), 0) == 1
    same_all(gpu_solve_line(eb, et, max_empties=7), e0, "one block")
    for order in (0, 1):
        same_all(gpu_search_line(sb, st, 3, w, order=order), s0[order], ("one block", order))
    assert ops.work_word("cuda").item() == 0


def test_node_counts_are_the_host_programs(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "line_host")
    b, t, _, _ = exact_batch()
    got = gpu_solve_line(b, t, max_empties=9)
    h = run_solve(exe, tmp_path, b, t, max_empties=9)
    assert got["nodes"].max() > 1000
    same_all(got, h, "exact")
    for name, depth in (("mid3", 3), ("mid4", 4), ("special3", 3)):
        b, t = tree_cases.inputs(name)
        w = tree_cases.TABLES["rng7"]
        for order in (0, 1):
            same_all(gpu_search_line(b, t, depth, w, order=order), run_search(exe, tmp_path, b, t, depth, w, order),
                     (name, order))


def test_the_work_word_is_shared_and_left_zero():
    eb, et = line_ref.exact_inputs(0, 5)
    want = line_ref.exact_cases(0, 5)
    bt, tt = dev(eb, et)
    sb, st = dev(*tree_cases.inputs("mid3"))
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.solve_line(bt, tt, max_empties=5, work=w)
    r2 = ops.search_line(sb, st, 3, work=w)
    r3 = ops.search_line(sb, st, 3, order=1, work=w)
    torch.cuda.synchronize()
    assert w.item() == 0
    assert (r1.line.cpu().numpy() == want["line"]).all()
    assert (r2.line.cpu().numpy() == line_ref.search_case("mid3", 3, "default")["line"]).all()
    assert torch.equal(r2.line, r3.line)
    # a rollout, the line calls, a solve and a search share the stream's word
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r4 = ops.solve_line(bt, tt, max_empties=5)
    s = ops.solve(bt, tt, max_empties=5)
    r5 = ops.search_line(sb, st, 3)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    assert torch.equal(r4.line, r1.line) and (s.value.cpu().numpy() == want["value"]).all()
    assert torch.equal(r5.line, r2.line)
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)


def test_null_outputs_null_turn_empty_batches_and_bad_arguments():
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    eb, et = line_ref.exact_inputs(0, 5)
    n = len(et)
    bt, tt = dev(eb, et)
    w = ops.work_word("cuda")
    line = torch.full((n, 32), 77, dtype=torch.uint8, device="cuda")
    val = torch.full((n,), 77, dtype=torch.int8, device="cuda")
    # every output NULL; the line alone; turn NULL: Black everywhere
    none = (None,) * 8
    assert lib.othl_solve_line(bt.data_ptr(), tt.data_ptr(), 5, 0, *none, w.data_ptr(), n, stream) == 0
    assert lib.othl_solve_line(bt.data_ptr(), tt.data_ptr(), 5, 0, line.data_ptr(), *none[1:], w.data_ptr(), n,
                               stream) == 0
    assert lib.othl_solve_line(bt.data_ptr(), None, 5, 0, None, None, val.data_ptr(), *none[3:], w.data_ptr(), n,
                               stream) == 0
    torch.cuda.synchronize()
    assert (line.cpu().numpy() == line_ref.exact_cases(0, 5)["line"]).all() and w.item() == 0
    black = ops.solve(bt, torch.ones_like(tt), max_empties=5)
    assert (val.cpu().numpy() == black.value.cpu().numpy()).all()
    mb, mt = dev(*tree_cases.inputs("mid3"))
    wp = ops._weights_ptr(None)
    line32 = torch.full((64, 32), 77, dtype=torch.uint8, device="cuda")
    val32 = torch.full((64,), 77, dtype=torch.int32, device="cuda")
    assert lib.othl_search_line(mb.data_ptr(), mt.data_ptr(), 3, None, 0, wp, 0, *none, w.data_ptr(), 64, stream) == 0
    assert lib.othl_search_line(mb.data_ptr(), None, 3, None, 1, wp, 0, line32.data_ptr(), None, val32.data_ptr(),
                                *none[3:], w.data_ptr(), 64, stream) == 0
    torch.cuda.synchronize()
    blk = ops.search(mb, torch.ones_like(mt), 3)
    assert (val32.cpu().numpy() == blk.value.cpu().numpy()).all() and w.item() == 0
    assert (line32[:, 0].cpu().numpy() == blk.best_move.cpu().numpy()).all()
    # n == 0: nothing launched, whatever the pointers
    assert lib.othl_solve_line(None, None, 5, 0, *none, w.data_ptr(), 0, stream) == 0
    assert lib.othl_search_line(None, None, 3, None, 0, wp, 0, *none, w.data_ptr(), 0, stream) == 0
    e = ops.solve_line(bt[:0], tt[:0], want_nodes=True)
    assert e.line.shape == (0, 32) and e.value.numel() == e.nodes.numel() == 0 and e.end_boards.shape == (0, 2)
    e = ops.search_line(bt[:0], tt[:0], 2)
    assert e.line.shape == (0, 32) and e.value.dtype == torch.int32
    # bad arguments: OTH_EINVAL, nothing launched
    good = (bt.data_ptr(), tt.data_ptr(), 5, 0, line.data_ptr(), *none[1:], w.data_ptr(), n, stream)
    for k, v in ((2, -1), (2, 13), (4, line.data_ptr() + 8), (10, line.data_ptr() + 8), (12, None), (13, -1),
                 (0, None)):
        a = list(good)
        a[k] = v
        assert lib.othl_solve_line(*a) == _lib.OTH_EINVAL, (k, v)
    qgood = (mb.data_ptr(), mt.data_ptr(), 3, None, 0, wp, 0, line32.data_ptr(), *none[1:], w.data_ptr(), 64, stream)
    for k, v in ((2, 0), (2, 9), (4, 2), (5, None), (7, line32.data_ptr() + 4), (15, None), (16, -1), (0, None)):
        a = list(qgood)
        a[k] = v
        assert lib.othl_search_line(*a) == _lib.OTH_EINVAL, (k, v)
    torch.cuda.synchronize()
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.solve_line(bt, tt, max_empties=13)
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.search_line(mb, mt, 3, order=2)
    # the failed calls launched nothing: the stream's next launch finds a zero word
    r = ops.solve_line(bt, tt, max_empties=5)
    torch.cuda.synchronize()
    assert (r.line.cpu().numpy() == line_ref.exact_cases(0, 5)["line"]).all() and ops.work_word("cuda").item() == 0


def test_both_calls_are_captured_and_replayed():
    eb, et = line_ref.exact_inputs(0, 6)
    want = line_ref.exact_cases(0, 6)
    bt, tt = dev(eb, et)
    mb, mt = dev(*tree_cases.inputs("mid3"))
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.solve_line(bt, tt, max_empties=6)
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.search_line(mb, mt, 3)
        r = ops.solve_line(bt, tt, max_empties=6, work=w)
        s = ops.search_line(mb, mt, 3, work=w)
    for _ in range(2):
        r.line.zero_(), r.value.zero_(), s.line.zero_(), s.end_boards.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (r.line.cpu().numpy() == want["line"]).all() and (r.value.cpu().numpy() == want["value"]).all()
        sw = line_ref.search_case("mid3", 3, "default")
        assert (s.line.cpu().numpy() == sw["line"]).all()
        assert (ops.to_numpy_u64(s.end_boards) == sw["end_boards"]).all() and w.item() == 0


# ---------------------------------------------------------------- VecEnv and the engine's pv
def test_vecenv_methods():
    env = VecEnv(8)
    r = env.search_line(3, want_nodes=True)
    s = env.search(3)
    assert torch.equal(r.value, s.value) and torch.equal(r.best_move, s.best_move)
    assert (r.length == 3).all() and torch.equal(r.line[:, 0], s.best_move) and (r.nodes > 0).all()
    assert (r.end_turn == 2).all()  # three plies from the opening: White to move
    e = env.solve_line(max_empties=12)
    assert (e.status == SKIPPED).all() and (e.length == 0).all() and (e.line == 255).all()
    assert torch.equal(e.end_boards, env.boards)


def engine_at(plies, **kw):
    """An engine after the first `plies` plies of a recorded random game."""
    o = oracle.rollout(1, 0xE17, record_moves=True)
    assert int(o["plies"][0]) > plies
    eng = Engine(**kw)
    sink = []
    for code in o["moves"][0, :plies].tolist():
        eng.handle("ps" if code == 64 else "%s%s" % ("abcdefgh"[code & 7], "12345678"[code >> 3]), sink.append)
    return eng


def position(eng):
    bl, wh = eng.board.bitboards()
    return np.array([[bl, wh]], np.uint64), np.array([eng.board.turn], np.uint8)


def pv(eng):
    out = []
    assert eng.handle("pv\n", out.append)
    assert len(out) == 1
    return out[0]


def pv_text(r):
    return " ".join(["%d" % int(r["value"][0])] + [
        "PS" if s == 64 else "%s%s" % ("ABCDEFGH"[s & 7], "12345678"[s >> 3])
        for s in r["line"][0, :int(r["length"][0])].tolist()])


@pytest.mark.parametrize("policy,depth,want_depth", [("search", 3, 3), ("eval", 3, 1)])
def test_pv_in_the_midgame(policy, depth, want_depth):
    w = tree_cases.TABLES["rng7"]
    eng = engine_at(20, policy=policy, depth=depth, weights=w)
    b, t = position(eng)
    want = pv_text(line_ref.search(b, t, want_depth, w))
    assert len(want.split()) == 1 + want_depth and pv(eng) == want
    # nothing was played: the same line again, and `go` plays its first move
    assert pv(eng) == want and (position(eng)[0] == b).all()
    out = []
    eng.handle("go", out.append)
    assert out[1].endswith(want.split()[1])


def test_pv_in_the_endgame_is_exact_whatever_the_policy():
    o = oracle.rollout(1, 0xE17, record_moves=True)
    rp = oracle.replay(o["moves"], o["plies"])
    plies = int(o["plies"][0])
    k = next(p for p in range(plies) if solve_ref.empties(rp["boards"][0, p:p + 1])[0] <= 8)
    for kw in (dict(policy="greedy", solve_empties=8), dict(policy="search", depth=2, solve_empties=10),
               dict(policy="random", solve_empties=12)):
        eng = engine_at(k, **kw)
        b, t = position(eng)
        want = pv_text(line_ref.exact(b, t))
        assert len(want.split()) >= 4 and pv(eng) == want and (position(eng)[0] == b).all()


def test_pv_unavailable_for_greedy_and_random_for_a_split_and_above_12_empties():
    for kw in (dict(policy="greedy"), dict(policy="random"), dict(policy="greedy", solve_empties=8),
               dict(policy="search", depth=6, split=2), dict(policy="greedy", solve_empties=16, solve_task_empties=8)):
        eng = engine_at(47 if "solve_task_empties" in kw else 20, **kw)
        b, _ = position(eng)
        if "solve_task_empties" in kw:
            assert 12 < solve_ref.empties(b)[0] <= 16
        assert pv(eng) == "pv unavailable" and (position(eng)[0] == b).all()


def test_pv_with_a_node_budget_uses_the_depth_the_last_go_reached():
    w = tree_cases.TABLES["default"]
    eng = engine_at(20, policy="search", depth=6, nodes=512, weights=w)
    assert pv(eng) == "pv unavailable"  # no go yet: no depth reached
    eng.handle("go", [].append)
    assert eng.reached and 1 <= eng.reached <= 6
    b, t = position(eng)
    assert pv(eng) == pv_text(gpu_search_line(b, t, eng.reached, w))
