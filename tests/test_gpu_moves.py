"""ops.solve_moves / ops.search_moves (include/othello_moves.h)
on the GPU against tests/moves_ref.py: the value of every root move from the
exact solvers and from the depth-limited search, their agreement with
ops.solve / ops.search, the node limit per move, the launch plumbing, and what
is built on them (GameBooks.endgame_losses, the engine's `hint`).  All
comparisons are exact."""
import os

import numpy as np
import pytest
import torch

import host_programs as hp
import moves_ref
import oracle
import solve_cases
import solve_ref
import tree_cases
from test_moves_host import run as moves_host_run

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, books, ops  # noqa: E402
from subproc_amd.engine import Engine  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz")
SOLVED, SKIPPED, INVALID, LIMIT = _lib.SOLVE_SOLVED, _lib.SOLVE_SKIPPED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
NAM, UNK, NAM32, UNK32 = moves_ref.NOT_A_MOVE, moves_ref.UNKNOWN, moves_ref.NOT_A_MOVE32, moves_ref.UNKNOWN32
T = moves_ref.T
# as tests/test_gpu_solve.py: no tree of the pool at <= 9 empties needs more than 23,082 nodes
LIMIT_9 = 1 << 18
NODE_LIMIT = 1 << 24


def test_the_constants_are_the_headers():
    assert (_lib.MOVES_NOT_A_MOVE, _lib.MOVES_UNKNOWN, _lib.MOVES_NOT_A_MOVE32, _lib.MOVES_UNKNOWN32) == (
        NAM, UNK, NAM32, UNK32)


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def unpack(r):
    torch.cuda.synchronize()
    nodes = None if r.nodes is None else r.nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    return (r.move_value.cpu().numpy().astype(np.int64), r.value.cpu().numpy().astype(np.int64),
            r.best_move.cpu().numpy().astype(np.int64), r.status.cpu().numpy().astype(np.int64), nodes)


def gpu_solve_moves(boards, turn, **kw):
    return unpack(ops.solve_moves(*dev(boards, turn), want_nodes=True, **kw))


def gpu_search_moves(boards, turn, depth, weights, **kw):
    return unpack(ops.search_moves(*dev(boards, turn), depth, weights=weights, want_nodes=True, **kw))


def assert_rows(got, want, status, what):
    rows, value, move, st, nodes = got
    wrows, wvalue, wmove = want
    assert rows.shape == wrows.shape, what
    assert (st == status).all(), (what, np.nonzero(st != status)[0][:8])
    bad = np.nonzero((rows != wrows).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:8], rows[bad[:2]], wrows[bad[:2]])
    assert (value == wvalue).all() and (move == wmove).all(), what


def exact_batch(hi=9):
    b, t, rows, value, move, forced, over = moves_ref.exact_cases(0, hi)
    assert len(t) == sum(len(solve_cases.cases()[e]["turn"]) for e in range(hi + 1))  # no position dropped
    assert forced.any() and over.any()  # the forced-pass and finished roots are in the set
    return b, t, (rows, value, move), forced, over


# ---------------------------------------------------------------- exact rows
def test_exact_rows_of_every_position_at_0_to_9_empties():
    b, t, want, forced, over = exact_batch()
    got = gpu_solve_moves(b, t, max_empties=9, node_limit=LIMIT_9)
    assert_rows(got, want, SOLVED, "one lane")
    rows, value, move, st, nodes = got
    assert (rows[forced | over] == NAM).all() and (move[forced] == 64).all() and (move[over] == 255).all()
    assert (nodes[over] == 0).all() and (nodes[forced] >= 1).all()
    assert (nodes[~over & ~forced] >= (rows[~over & ~forced] != NAM).sum(axis=1)).all()
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("npp", [64, 4096])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3, 6])
def test_the_split_form_gives_identical_rows(task_empties, order, npp):
    b, t, want, _, _ = exact_batch()
    got = gpu_solve_moves(b, t, max_empties=9, node_limit=LIMIT_9, task_empties=task_empties, order=order,
                          nodes_per_position=npp)
    assert_rows(got, want, SOLVED, (task_empties, order, npp))
    assert ops.work_word("cuda").item() == 0


def test_the_split_form_with_a_16_entry_table_gives_identical_rows():
    b, t, want, _, _ = exact_batch()
    table = ops.SolveTable(4)
    got = gpu_solve_moves(b, t, max_empties=9, node_limit=LIMIT_9, task_empties=3, order=1, nodes_per_position=64,
                          table=table, hash_min_empties=1)
    assert_rows(got, want, SOLVED, "table")
    assert int((table.data != 0).sum()) > 0  # the table was used


def test_value_move_and_status_are_ops_solves():
    b, t, want, _, _ = exact_batch()
    b = np.concatenate([b, np.array([[0xFF, 0x81], [(1 << 64) - 1, (1 << 64) - 1]], np.uint64)])  # two overlaps
    t = np.concatenate([t, np.array([1, 2], np.uint8)])
    bt, tt = dev(b, t)
    for kw in (dict(), dict(task_empties=3, nodes_per_position=64)):
        rows, value, move, st, nodes = unpack(ops.solve_moves(bt, tt, max_empties=6, node_limit=LIMIT_9,
                                                              want_nodes=True, **kw))
        s = ops.solve(bt, tt, max_empties=6, node_limit=LIMIT_9, **kw)
        assert (value == s.value.cpu().numpy()).all() and (move == s.best_move.cpu().numpy()).all()
        assert (st == s.status.cpu().numpy()).all()
        deep = np.append(solve_ref.empties(b[:-2]) > 6, [False, False])
        assert deep.sum() > 100 and (st[deep] == SKIPPED).all() and (st[-2:] == INVALID).all()
        off = deep | (st == INVALID)
        assert (rows[off] == NAM).all() and (value[off] == 0).all() and (move[off] == 255).all()
        assert (nodes[off] == 0).all()
        assert (rows[~off] == want[0][~off[:-2]]).all()


# ---------------------------------------------------------------- deep positions
def test_deep_roots_through_the_split_solver():
    """13, 14 and 16 empties: no exhaustive truth is affordable, so each entry
    is compared with ops.solve of the oracle's child solved on its own, and the
    row's maximum and lowest argmax with the fixture."""
    fx = np.load(FIXTURE)
    idx = np.concatenate([np.nonzero(fx["empties"] == e)[0][:k] for e, k in ((13, 4), (14, 2), (16, 1))])
    assert len(idx) == 7
    b, t = fx["boards"][idx], fx["turn"][idx]
    kw = dict(max_empties=16, task_empties=8, order=1)
    rows, value, move, st, nodes = gpu_solve_moves(b, t, **kw)
    assert (st == SOLVED).all()
    assert (value == fx["value"][idx]).all() and (move == fx["best_move"][idx]).all()
    assert (rows.max(axis=1) == fx["value"][idx]).all() and (rows.argmax(axis=1) == fx["best_move"][idx]).all()
    ci, csq, cb, ct, forced, over = moves_ref.children(b, t)
    assert not forced.any() and not over.any()
    s = ops.solve(*dev(cb, ct), **kw)
    assert (s.status.cpu().numpy() == SOLVED).all()
    want = moves_ref.rows_of(len(t), ci, csq, -s.value.cpu().numpy().astype(np.int64), NAM)
    assert (rows == want).all()


# ---------------------------------------------------------------- search rows
SEARCH_CASES = [("mid3", 1), ("mid3", 2), ("mid3", 3), ("mid4", 4), ("mid5", 5), ("special3", 3)]


def assert_is_ops_search(b, t, depth, weights, got):
    s = ops.search(*dev(b, t), depth, weights=weights)
    assert (got[1] == s.value.cpu().numpy()).all() and (got[2] == s.best_move.cpu().numpy()).all()
    assert (got[3] == s.status.cpu().numpy()).all()


@pytest.mark.parametrize("table", tree_cases.BOTH)
@pytest.mark.parametrize("name,depth", SEARCH_CASES)
def test_search_rows_match_the_checker(name, depth, table):
    b, t = tree_cases.inputs(name)
    assert len(t) == tree_cases.MID_ROOTS.get(name, len(t)) and len(t) >= 8
    w = tree_cases.TABLES[table]
    got = gpu_search_moves(b, t, depth, w, node_limit=NODE_LIMIT)
    want = moves_ref.search_case(name, depth, table)
    assert_rows(got, want, _lib.SEARCH_SEARCHED, (name, depth, table))
    if name == "special3":
        assert (want[2] == 64).all() and (got[0] == NAM32).all()  # the pool's special roots at 3..9 empties all pass
    assert_is_ops_search(b, t, depth, w, got)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("table", tree_cases.BOTH)
def test_search_of_finished_roots(table):
    """The pool's finished roots (they have at most two empties): T times the disc difference, move 255, no task."""
    eb, et, _, _, _, _, over = moves_ref.exact_cases(0, 9)
    b, t = eb[over], et[over]
    assert len(t) >= 8
    w = tree_cases.TABLES[table]
    got = gpu_search_moves(b, t, 3, w)
    want = moves_ref.search(b, t, 3, w)
    assert_rows(got, want, _lib.SEARCH_SEARCHED, table)
    assert (got[2] == 255).all() and (got[0] == NAM32).all() and (got[4] == 0).all()
    assert (got[1] == T * oracle.result(b)["diff"].astype(np.int64) * np.where(t == 1, 1, -1)).all()
    assert_is_ops_search(b, t, 3, w, got)


@pytest.mark.parametrize("table", tree_cases.BOTH)
@pytest.mark.parametrize("e", [6, 8])
def test_depth_8_rows_are_T_times_the_exact_rows(e, table):
    c = solve_cases.cases()[e]
    rows, value, move = moves_ref.exact(moves_ref.window_ref.case_roots(e))
    assert len(value) == len(c["turn"]) >= 64
    want = (np.where(rows == NAM, NAM32, rows * T), value * T, move)
    w = tree_cases.TABLES[table]
    got = gpu_search_moves(c["boards"], c["turn"], 8, w, node_limit=NODE_LIMIT)
    assert_rows(got, want, _lib.SEARCH_SEARCHED, (e, table))
    assert_is_ops_search(c["boards"], c["turn"], 8, w, got)


@pytest.mark.parametrize("table", tree_cases.BOTH)
def test_depth_1_rows_are_the_childrens_evals_from_the_root_movers_side(table):
    mb, mt = tree_cases.inputs("mid3")
    eb, et, *_ = moves_ref.exact_cases(0, 3)
    b, t = np.concatenate([mb, eb]), np.concatenate([mt, et])
    assert len(t) == 64 + len(et)
    w = tree_cases.TABLES[table]
    ci, csq, cb, ct, forced, over = moves_ref.children(b, t)
    cbt, _ = dev(cb, ct)
    ev = ops.evaluate(cbt, torch.from_numpy(np.ascontiguousarray(t[ci])).cuda(), w).cpu().numpy().astype(np.int64)
    done = (oracle.legal(cb, ct) == 0) & (oracle.legal(cb, (3 - ct).astype(np.uint8)) == 0)
    diff = oracle.result(cb)["diff"].astype(np.int64) * np.where(t[ci] == 1, 1, -1)
    assert done.any() and (~done).any()
    want = moves_ref.rows_of(len(t), ci, csq, np.where(done, T * diff, ev), NAM32)
    got = gpu_search_moves(b, t, 1, w)
    assert (got[0] == want).all()
    assert_is_ops_search(b, t, 1, w, got)
    has = ~forced & ~over
    assert (got[1][has] == want[has].max(axis=1)).all() and (got[2][has] == want[has].argmax(axis=1)).all()


# ---------------------------------------------------------------- the host program's node counts
def test_one_lane_node_counts_are_the_host_programs(tmp_path_factory, tmp_path):
    exe = hp.compiled(tmp_path_factory, "moves_host")

    def host(mode, b, t, level, weights=None):
        value, move, status, nodes, rows = moves_host_run(exe, tmp_path, mode, b, t, level, weights)
        return np.column_stack([value, move, status, nodes, rows])

    b, t, want, _, _ = exact_batch()
    got = gpu_solve_moves(b, t, max_empties=9)
    h = host("solve", b, t, 9)
    assert (h[:, 3] == got[4]).all() and (h[:, 4:] == got[0]).all() and got[4].max() > 1000
    for name, depth in (("mid3", 3), ("mid4", 4), ("special3", 3)):
        b, t = tree_cases.inputs(name)
        w = tree_cases.TABLES["rng7"]
        got = gpu_search_moves(b, t, depth, w)
        h = host("search", b, t, depth, w)
        assert (h[:, 3] == got[4]).all() and (h[:, 4:] == got[0]).all(), name


# ---------------------------------------------------------------- node limit
def test_solve_node_limit_bounds_each_root_move():
    c = solve_cases.cases()[8]
    b, t = c["boards"], c["turn"]
    full = gpu_solve_moves(b, t, max_empties=8)
    assert (full[3] == SOLVED).all()
    # every move's own count: the task is oths_solve's solve of the child
    ci, csq, cb, ct, forced, over = moves_ref.children(b, t)
    s = ops.solve(*dev(cb, ct), max_empties=8, want_nodes=True)
    cn = s.nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    total = np.bincount(ci, cn + 1, len(t)).astype(np.int64)
    has = ~forced & ~over
    assert has.sum() >= 64 and (full[4][has] == total[has]).all()  # want_nodes of the first run
    i = int(np.argmax(np.where(has, full[4], -1)))  # the position, and its most expensive move
    mine = np.nonzero(ci == i)[0]
    k = mine[np.argmax(cn[mine])]
    limit = int(cn[k])
    assert limit > 100
    at = gpu_solve_moves(b, t, max_empties=8, node_limit=limit)
    assert (at[0][i] == full[0][i]).all() and at[3][i] == SOLVED and at[1][i] == full[1][i] and at[2][i] == full[2][i]
    below = gpu_solve_moves(b, t, max_empties=8, node_limit=limit - 1)
    want = moves_ref.rows_of(len(t), ci, csq, np.where(cn >= limit, UNK, full[0][ci, csq]), NAM)
    assert below[0][i, csq[k]] == UNK and (below[0][has] == want[has]).all()
    cut = np.bincount(ci, cn >= limit, len(t)) > 0
    assert cut[i] and (~cut & has).any()
    assert (below[3][cut & has] == LIMIT).all() and (below[1][cut & has] == 0).all()
    assert (below[2][cut & has] == 255).all()
    keep = ~cut & has
    assert (below[3][keep] == SOLVED).all() and (below[1][keep] == full[1][keep]).all()
    assert (below[2][keep] == full[2][keep]).all()


def test_search_node_limit_bounds_each_root_move():
    g = tree_cases.midgame()
    own = oracle.legal(g["boards"], g["turn"])
    single = np.nonzero(np.array([bin(int(x)).count("1") for x in own]) == 1)[0]
    few = np.nonzero(np.array([bin(int(x)).count("1") for x in own]) == 3)[0][:32]
    assert len(single) >= 1 and len(few) == 32
    idx = np.concatenate([single[:8], few])
    b, t = g["boards"][idx], g["turn"][idx]
    w = tree_cases.TABLES["default"]
    ns = len(single[:8])
    full = gpu_search_moves(b, t, 4, w)
    assert (full[3] == _lib.SEARCH_SEARCHED).all()
    c = int(full[4][0]) - 1  # a root with one move: its subtree's count is the position's less the root task
    assert c > 10
    sq = int(full[2][0])
    at = gpu_search_moves(b, t, 4, w, node_limit=c)
    assert (at[0][0] == full[0][0]).all() and at[3][0] == _lib.SEARCH_SEARCHED and at[1][0] == full[1][0]
    below = gpu_search_moves(b, t, 4, w, node_limit=c - 1)
    assert below[0][0, sq] == UNK32 and (below[0][0] != NAM32).sum() == 1
    assert below[3][0] == _lib.SEARCH_LIMIT and below[1][0] == 0 and below[2][0] == 255
    # every other single-move root is cut exactly when its subtree needs at least c
    need = full[4][:ns] - 1 >= c
    assert ((below[3][:ns] == _lib.SEARCH_LIMIT) == need).all()
    # everywhere: a square is unknown or keeps its value; the status is LIMIT exactly with an unknown square
    unknown = below[0] == UNK32
    assert (below[0][~unknown] == full[0][~unknown]).all()
    assert ((below[3] == _lib.SEARCH_LIMIT) == unknown.any(axis=1)).all()
    cut = unknown.any(axis=1)
    assert (below[1][cut] == 0).all() and (below[2][cut] == 255).all()
    assert (below[1][~cut] == full[1][~cut]).all() and (below[2][~cut] == full[2][~cut]).all()


# ---------------------------------------------------------------- batch sizes and launch behaviour
def cycle(n, pool):
    k = np.arange(n) % len(pool[1])
    return k, pool[0][k], pool[1][k]


def search_pool():
    g = tree_cases.midgame()
    return np.concatenate([g["boards"][:200], tree_cases.inputs("special3")[0]]), \
        np.concatenate([g["turn"][:200], tree_cases.inputs("special3")[1]])


@pytest.fixture(scope="module")
def search_pool_want():
    b, t = search_pool()
    return moves_ref.search(b, t, 2, tree_cases.TABLES["rng7"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(n, search_pool_want):
    eb, et, rows, value, move, _, _ = moves_ref.exact_cases(0, 6)
    k, b, t = cycle(n, (eb, et))
    assert len(t) == n
    assert_rows(gpu_solve_moves(b, t, max_empties=6, node_limit=LIMIT_9), (rows[k], value[k], move[k]), SOLVED, n)
    if n <= 65:
        assert_rows(gpu_solve_moves(b, t, max_empties=6, node_limit=LIMIT_9, task_empties=3, nodes_per_position=64),
                    (rows[k], value[k], move[k]), SOLVED, n)
    k, b, t = cycle(n, search_pool())
    assert len(t) == n
    got = gpu_search_moves(b, t, 2, tree_cases.TABLES["rng7"])
    assert_rows(got, tuple(x[k] for x in search_pool_want), _lib.SEARCH_SEARCHED, n)
    assert ops.work_word("cuda").item() == 0


def test_results_do_not_depend_on_the_batch_or_the_grid(monkeypatch, search_pool_want):
    eb, et, *_ = moves_ref.exact_cases(0, 7)
    sb, st = search_pool()
    w = tree_cases.TABLES["rng7"]
    e0 = gpu_solve_moves(eb, et, max_empties=7)
    s0 = gpu_search_moves(sb, st, 3, w)
    perm = np.random.default_rng(5).permutation(len(et))
    ep = gpu_solve_moves(eb[perm], et[perm], max_empties=7)
    assert all((x == y[perm]).all() for x, y in zip(ep, e0))
    perm = np.random.default_rng(6).permutation(len(st))
    sp = gpu_search_moves(sb[perm], st[perm], 3, w)
    assert all((x == y[perm]).all() for x, y in zip(sp, s0))
    e5 = gpu_solve_moves(eb[-5:], et[-5:], max_empties=7)
    assert all((x == y[-5:]).all() for x, y in zip(e5, e0))
    monkeypatch.setenv("OTH_SOLVE_BLOCKS", "1")
    monkeypatch.setenv("OTH_SEARCH_BLOCKS", "1")
    e1 = gpu_solve_moves(eb, et, max_empties=7)
    s1 = gpu_search_moves(sb, st, 3, w)
    assert all((x == y).all() for x, y in zip(e1, e0)) and all((x == y).all() for x, y in zip(s1, s0))
    assert ops.work_word("cuda").item() == 0


def test_the_work_word_is_shared_and_left_zero():
    eb, et, rows, value, move, _, _ = moves_ref.exact_cases(0, 5)
    bt, tt = dev(eb, et)
    sb, st = dev(*tree_cases.inputs("mid3"))
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.solve_moves(bt, tt, max_empties=5, work=w)
    r2 = ops.search_moves(sb, st, 3, work=w)
    r3 = ops.solve_moves(bt, tt, max_empties=5, work=w, task_empties=2, nodes_per_position=64)
    torch.cuda.synchronize()
    assert w.item() == 0
    assert (r1.move_value.cpu().numpy() == rows).all() and (r3.move_value.cpu().numpy() == rows).all()
    assert (r2.move_value.cpu().numpy() == moves_ref.search_case("mid3", 3, "default")[0]).all()
    # a rollout, the per-move calls and a solve share the stream's word
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r4 = ops.solve_moves(bt, tt, max_empties=5)
    s = ops.solve(bt, tt, max_empties=5)
    r5 = ops.search_moves(sb, st, 3)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    assert (r4.move_value.cpu().numpy() == rows).all() and (s.value.cpu().numpy() == value).all()
    assert (r5.move_value.cpu().numpy() == r2.move_value.cpu().numpy()).all()
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)


def raw_args(n, dtype, size):
    rows = torch.full((n, 64), 77, dtype=dtype, device="cuda")
    val = torch.full((n,), 77, dtype=dtype, device="cuda")
    scratch = torch.empty(max(size, 16) // 8, dtype=torch.int64, device="cuda")
    return rows, val, scratch


def test_null_outputs_null_turn_empty_batches_and_bad_arguments():
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    eb, et, rows, value, move, _, _ = moves_ref.exact_cases(0, 5)
    n = len(et)
    bt, tt = dev(eb, et)
    w = ops.work_word("cuda")
    size = lib.otha_solve_moves_scratch_bytes(n, 5)
    assert size > 0 and lib.otha_solve_moves_scratch_bytes(-1, 5) == _lib.OTH_EINVAL
    assert lib.otha_solve_moves_scratch_bytes(n, 13) == _lib.OTH_EINVAL
    assert lib.otha_solve_moves_split_scratch_bytes(n, 17, 64) == _lib.OTH_EINVAL
    assert lib.otha_solve_moves_split_scratch_bytes(n, 16, 63) == _lib.OTH_EINVAL
    assert lib.otha_solve_moves_split_scratch_bytes(n, 16, 64) > lib.othe_scratch_bytes(16 * n, 64)
    assert lib.otha_search_moves_scratch_bytes(-1) == _lib.OTH_EINVAL and lib.otha_search_moves_scratch_bytes(0) >= 0
    out, val, scratch = raw_args(n, torch.int8, size)
    sp, sb = scratch.data_ptr(), scratch.numel() * 8
    # every output NULL; the rows alone; turn NULL: Black everywhere
    assert lib.otha_solve_moves(bt.data_ptr(), tt.data_ptr(), 5, 0, None, None, None, None, None, sp, sb,
                                w.data_ptr(), n, stream) == 0
    assert lib.otha_solve_moves(bt.data_ptr(), tt.data_ptr(), 5, 0, out.data_ptr(), None, None, None, None, sp, sb,
                                w.data_ptr(), n, stream) == 0
    assert lib.otha_solve_moves(bt.data_ptr(), None, 5, 0, None, val.data_ptr(), None, None, None, sp, sb,
                                w.data_ptr(), n, stream) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == rows).all() and w.item() == 0
    black = ops.solve(bt, torch.ones_like(tt), max_empties=5)
    assert (val.cpu().numpy() == black.value.cpu().numpy()).all()
    # the search likewise
    mb, mt = dev(*tree_cases.inputs("mid3"))
    wp = ops._weights_ptr(None)
    ssize = lib.otha_search_moves_scratch_bytes(64)
    out32, val32, scratch32 = raw_args(64, torch.int32, ssize)
    qp, qb = scratch32.data_ptr(), scratch32.numel() * 8
    assert lib.otha_search_moves(mb.data_ptr(), mt.data_ptr(), 3, wp, 0, None, None, None, None, None, qp, qb,
                                 w.data_ptr(), 64, stream) == 0
    assert lib.otha_search_moves(mb.data_ptr(), None, 3, wp, 0, out32.data_ptr(), val32.data_ptr(), None, None, None,
                                 qp, qb, w.data_ptr(), 64, stream) == 0
    torch.cuda.synchronize()
    blk = ops.search(mb, torch.ones_like(mt), 3)
    assert (val32.cpu().numpy() == blk.value.cpu().numpy()).all() and w.item() == 0
    assert (out32.cpu().numpy().max(axis=1) == blk.value.cpu().numpy()).all()
    # n == 0: nothing launched, whatever the pointers
    assert lib.otha_solve_moves(None, None, 5, 0, None, None, None, None, None, None, 0, w.data_ptr(), 0, stream) == 0
    assert lib.otha_solve_moves_split(None, None, 16, 8, 1, 0, 64, 0, 0, None, 0, None, None, None, None, None, None,
                                      0, w.data_ptr(), 0, stream) == 0
    assert lib.otha_search_moves(None, None, 3, wp, 0, None, None, None, None, None, None, 0, w.data_ptr(), 0,
                                 stream) == 0
    e = ops.solve_moves(bt[:0], tt[:0], want_nodes=True)
    assert e.move_value.shape == (0, 64) and e.value.numel() == e.nodes.numel() == 0
    e = ops.search_moves(bt[:0], tt[:0], 2)
    assert e.move_value.shape == (0, 64) and e.move_value.dtype == torch.int32
    # bad arguments: OTH_EINVAL, nothing launched
    EINVAL = _lib.OTH_EINVAL
    good = (bt.data_ptr(), tt.data_ptr(), 5, 0, out.data_ptr(), None, None, None, None, sp, sb, w.data_ptr(), n, stream)

    def with_(k, v):
        a = list(good)
        a[k] = v
        return a

    for k, v in ((2, -1), (2, 13), (9, None), (9, sp + 8), (10, size - 1), (11, None), (12, -1), (0, None)):
        assert lib.otha_solve_moves(*with_(k, v)) == EINVAL, (k, v)
    ssz = lib.otha_solve_moves_split_scratch_bytes(4, 16, 64)
    _, _, s2 = raw_args(4, torch.int8, ssz)
    table = ops.SolveTable(4)
    sgood = (bt.data_ptr(), tt.data_ptr(), 16, 8, 1, 0, 64, 4, 8, table.data.data_ptr(), table.nbytes, None, None,
             None, None, None, s2.data_ptr(), s2.numel() * 8, w.data_ptr(), 4, stream)
    assert lib.otha_solve_moves_split(*sgood) == 0
    for k, v in ((2, 17), (3, 0), (3, 13), (4, 2), (6, 63), (7, 3), (7, 27), (8, 0), (8, 13), (10, table.nbytes - 1),
                 (9, table.data.data_ptr() + 8), (17, ssz - 1), (18, None), (19, -1)):
        a = list(sgood)
        a[k] = v
        assert lib.otha_solve_moves_split(*a) == EINVAL, (k, v)
    qgood = (mb.data_ptr(), mt.data_ptr(), 3, wp, 0, out32.data_ptr(), None, None, None, None, qp, qb, w.data_ptr(),
             64, stream)
    for k, v in ((2, 0), (2, 9), (3, None), (10, None), (11, ssize - 1), (12, None), (13, -1), (0, None)):
        a = list(qgood)
        a[k] = v
        assert lib.otha_search_moves(*a) == EINVAL, (k, v)
    torch.cuda.synchronize()
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.solve_moves(bt, tt, max_empties=13)
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.search_moves(mb, mt, 9)
    with pytest.raises(ValueError, match="order needs task_empties"):
        ops.solve_moves(bt, tt, order=1)
    with pytest.raises(ValueError, match="table needs task_empties"):
        ops.solve_moves(bt, tt, table=table)
    with pytest.raises(ValueError, match="32 bits"):
        ops.search_moves(mb, mt, 2, node_limit=1 << 32)
    # the failed calls launched nothing: the stream's next launch finds a zero word
    r = ops.solve_moves(bt, tt, max_empties=5)
    torch.cuda.synchronize()
    assert (r.move_value.cpu().numpy() == rows).all() and ops.work_word("cuda").item() == 0


def test_the_one_lane_forms_are_captured_and_replayed():
    eb, et, rows, value, move, _, _ = moves_ref.exact_cases(0, 6)
    bt, tt = dev(eb, et)
    mb, mt = dev(*tree_cases.inputs("mid3"))
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.solve_moves(bt, tt, max_empties=6)
        with pytest.raises(RuntimeError, match="graph capture"):
            ops.solve_moves(bt, tt, max_empties=6, task_empties=3, work=w)
        r = ops.solve_moves(bt, tt, max_empties=6, work=w)
        s = ops.search_moves(mb, mt, 3, work=w)
    for _ in range(2):
        r.move_value.zero_(), r.value.zero_(), s.move_value.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (r.move_value.cpu().numpy() == rows).all() and (r.value.cpu().numpy() == value).all()
        assert (s.move_value.cpu().numpy() == moves_ref.search_case("mid3", 3, "default")[0]).all()
        assert w.item() == 0


def test_vecenv_methods():
    env = VecEnv(8)
    r = env.search_moves(2)
    s = env.search(2)
    assert torch.equal(r.value, s.value) and torch.equal(r.best_move, s.best_move)
    assert ((r.move_value != NAM32).sum(dim=1) == 4).all()  # the opening has four moves
    e = env.solve_moves(max_empties=12)
    assert (e.status == SKIPPED).all() and (e.move_value == NAM).all()


# ---------------------------------------------------------------- books
def test_endgame_losses_of_recorded_games():
    n, seed, max_empties = 64, 0xB00C, 7
    g = ops.rollout(n, seed, record_moves=True)
    bk = books.GameBooks.from_rollout(g)
    got = bk.endgame_losses(max_empties=max_empties).cpu().numpy().astype(np.int64)
    o = oracle.rollout(n, seed, record_moves=True)
    rp = oracle.replay(o["moves"], o["plies"])
    want = []
    for i in range(n):
        plies = int(o["plies"][i])
        b, t = rp["boards"][i, :plies + 1], rp["turn"][i, :plies + 1]
        code = np.append(o["moves"][i, :plies].astype(np.int64), 255)
        own = oracle.legal(b, t)
        sel = (np.arange(plies + 1) < plies) & (solve_ref.empties(b) <= max_empties) & (code < 64)
        sel &= ((own >> np.minimum(code, 63).astype(np.uint64)) & np.uint64(1)) == 1
        loss = np.full(plies + 1, -1, np.int64)
        if sel.any():
            rows, value, _ = moves_ref.exact(moves_ref.window_ref.roots(b[sel], t[sel]))
            loss[sel] = value - rows[np.arange(sel.sum()), code[sel]]
        want.append(loss)
    want = np.concatenate(want)
    assert got.shape == want.shape and (got == want).all()
    assert (got > 0).any() and (got == 0).any() and (got == -1).any() and (got >= -1).all()
    assert (got >= 0).sum() >= n  # some rows of about every game


# ---------------------------------------------------------------- the engine's hint
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


def hint(eng):
    out = []
    assert eng.handle("hint\n", out.append)
    assert out[-1] == "" and "" not in out[:-1]
    return out[:-1]


def lines(row, fill):
    return ["%s%s %d" % ("ABCDEFGH"[s & 7], "12345678"[s >> 3], v) for s, v in moves_ref.hint_lines(row, fill)]


@pytest.mark.parametrize("policy,depth,want_depth", [("search", 3, 3), ("eval", 1, 1), ("eval", 3, 1)])
def test_hint_in_the_midgame(policy, depth, want_depth):
    w = tree_cases.TABLES["rng7"]
    eng = engine_at(20, policy=policy, depth=depth, weights=w)
    b, t = position(eng)
    rows, _, _ = moves_ref.search(b, t, want_depth, w)
    want = lines(rows[0], NAM32)
    assert len(want) >= 2 and hint(eng) == want
    # nothing was played: the same hint again, and `go` plays what it would have played
    assert hint(eng) == want and (position(eng)[0] == b).all()
    other = engine_at(20, policy=policy, depth=depth, weights=w)
    a, c = [], []
    eng.handle("go", a.append)
    other.handle("go", c.append)
    assert a == c and (position(eng)[0] == position(other)[0]).all()


def test_hint_in_the_endgame_is_exact_whatever_the_policy():
    o = oracle.rollout(1, 0xE17, record_moves=True)
    rp = oracle.replay(o["moves"], o["plies"])
    plies = int(o["plies"][0])
    k = next(p for p in range(plies) if solve_ref.empties(rp["boards"][0, p:p + 1])[0] <= 8
             and bin(int(oracle.legal(rp["boards"][0, p:p + 1], rp["turn"][0, p:p + 1])[0])).count("1") >= 2)
    for kw in (dict(policy="greedy", solve_empties=8), dict(policy="search", depth=2, solve_empties=10),
               dict(policy="eval", solve_empties=12, solve_task_empties=4, solve_hash_bits=4)):
        eng = engine_at(k, **kw)
        b, t = position(eng)
        rows, _, _ = moves_ref.exact(moves_ref.window_ref.roots(b, t))
        want = lines(rows[0], NAM)
        assert len(want) >= 2 and hint(eng) == want
        assert (position(eng)[0] == b).all()


def test_hint_unavailable_for_greedy_and_random():
    for policy in ("greedy", "random"):
        eng = engine_at(20, policy=policy)
        b, _ = position(eng)
        assert hint(eng) == ["hint unavailable"] and (position(eng)[0] == b).all()
        # outside --solve-empties the same
        assert hint(engine_at(20, policy=policy, solve_empties=8)) == ["hint unavailable"]
