"""ops.solve(window=..., wld=...) / othw_solve / othw_solve_split on the GPU
(include/othello_solve_window.h): the value clamped into each
position's window and the move the window proves, against tests/window_ref.py
(the exhaustive checker over every root move) at 0..9 empties in every window
family, one launch mixing the windows; the split solver against the one-lane
windowed call at 10 and 12 empties; the deep fixture at 13..16 empties;
independence of the grid and of the table; the statuses with OTHS_BADWINDOW;
forced passes, the eight images, graph capture, the engine and VecEnv.

Every comparison asserts status == SOLVED where a search was expected."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
import solve_cases
import solve_ref
import tree_cases
import window_ref

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, codec, engine, ops  # noqa: E402

SKIPPED, SOLVED, INVALID, LIMIT = _lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
BADWINDOW = _lib.SOLVE_BADWINDOW
FULL = (1 << 64) - 1
NODE_LIMIT = 1 << 26  # per position / per task: a defect ends as LIMIT, which every test below refuses
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(boards, turn):
    return (ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda"),
            torch.from_numpy(np.array(turn, np.uint8)).cuda())


def i8(x):
    return torch.from_numpy(np.array(x, np.int8)).cuda()


def solve(boards, turn, alpha=None, beta=None, max_empties=16, node_limit=NODE_LIMIT, **kw):
    """(value, move, status, nodes) as numpy; alpha / beta arrays become per-position tensors."""
    b, t = dev(boards, turn)
    if alpha is not None:
        kw["window"] = (i8(alpha), i8(beta))
    if "task_empties" not in kw:
        max_empties = min(max_empties, 12)
    r = ops.solve(b, t, max_empties=max_empties, node_limit=node_limit, want_nodes=True, **kw)
    torch.cuda.synchronize()
    return (r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy().astype(np.int64),
            r.status.cpu().numpy().astype(np.int64), r.nodes.cpu().numpy().view(np.uint32).astype(np.int64))


def assert_same(got, want, what):
    (v, m, s), (rv, rm) = got[:3], want
    assert (s == SOLVED).all(), (what, np.nonzero(s != SOLVED)[0][:8], s[s != SOLVED][:8])
    bad = np.nonzero((v != rv) | (m != rm))[0]
    assert len(bad) == 0, (what, bad[:8], v[bad[:8]], rv[bad[:8]], m[bad[:8]], rm[bad[:8]])


@functools.lru_cache(maxsize=None)
def checker_batch():
    """cases() at 0..9 empties x every family, with the helper's answers."""
    out = window_ref.case_batch(0, 9)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ladder_batch(e, k):
    """ladder(e, k) x every family around the one-lane solver's exact values,
    answered by the one-lane WINDOWED call (checked against the helper above)."""
    b, t = solve_cases.ladder(e, k)
    V = solve(b, t, max_empties=e)[0]
    bb, tt, aa, be, vv = [], [], [], [], []
    for name in window_ref.FAMILIES:
        a, c, keep = window_ref.family(name, V)
        bb.append(b[keep]), tt.append(t[keep]), aa.append(a[keep]), be.append(c[keep]), vv.append(V[keep])
    bb, tt, aa, be, vv = (np.concatenate(x) for x in (bb, tt, aa, be, vv))
    v, m, s, _ = solve(bb, tt, aa, be, max_empties=e)
    assert (s == SOLVED).all() and (v == np.clip(vv, aa, be)).all()
    out = (bb, tt, aa, be, v, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz"))
    out = (fx["boards"], fx["turn"], fx["value"].astype(np.int64), fx["best_move"].astype(np.int64),
           fx["empties"].astype(np.int64))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture_root_moves():
    """Every root move of the fixture's 13- and 14-empties roots with its exact
    value from the root mover's side, by the split solver WITHOUT a window
    (ops.step + ops.solve(task_empties=...): the code before this feature):
    (root index, square, value) arrays."""
    b, t, rv, rm, emp = fixture()
    sel = np.nonzero((emp <= 14) & (rm < 64))[0]
    own = oracle.legal(b[sel], solve_ref.mover(t[sel]))
    ci, csq = solve_ref._bits(own)
    side = solve_ref.mover(t[sel][ci])
    bt, tt = dev(b[sel][ci], side)
    st = ops.step(bt, tt, torch.from_numpy(np.ascontiguousarray(csq, np.uint8)).cuda(), want_flips=False,
                  want_legal=False)
    # the child with the OPPONENT to move, whatever it can do: the solver's rules handle its pass
    r = ops.solve(st.boards, (3 - tt).to(torch.uint8), max_empties=13, node_limit=NODE_LIMIT, task_empties=8, order=1)
    torch.cuda.synchronize()
    assert (r.status.cpu().numpy() == SOLVED).all()
    cval = -r.value.cpu().numpy().astype(np.int64)
    # the children's maxima are the fixture's values and their lowest maximisers its moves
    best = np.full(len(sel), -99, np.int64)
    np.maximum.at(best, ci, cval)
    assert (best == rv[sel]).all()
    return sel[ci], csq.astype(np.int64), cval


def fixture_expect(alpha, beta):
    """(value, move, known) of the fixture's roots under (alpha, beta): the move
    is known inside the window (the fixture's), on a fail-low (255), at a forced
    pass (64), and on a fail-high at 13 and 14 empties (fixture_root_moves)."""
    b, t, rv, rm, emp = fixture()
    value = np.clip(rv, alpha, beta)
    move = np.where(rm == 64, 64, np.where(rv <= alpha, 255, rm))
    known = (rm == 64) | (rv <= alpha) | (rv < beta)
    ri, sq, cv = fixture_root_moves()
    for i in np.nonzero(~known & (emp <= 14))[0]:
        mine = (ri == i) & (cv >= beta[i])
        move[i], known[i] = sq[mine].min(), True
    return value, move, known


# ---------------------------------------------------------------- 1. the one-lane solver
def test_one_lane_matches_the_helper_in_every_family_in_one_launch():
    b, t, a, be, rv, rm, fam = checker_batch()
    assert set(fam.tolist()) == set(range(9)) and len(t) > 40000
    v, m, s, nd = solve(b, t, a, be)
    assert_same((v, m, s), (rv, rm), "one lane")
    # a narrower window searches a subtree of the full window's
    full = solve(b, t)
    assert (nd <= full[3]).all(), np.nonzero(nd > full[3])[0][:8]
    assert (nd[fam != 0] < full[3][fam != 0]).any()
    assert ops.work_word("cuda").item() == 0


def test_the_full_window_is_the_call_without_a_window_bit_for_bit():
    b, t = [np.concatenate(x) for x in zip(*[(solve_cases.cases()[e]["boards"], solve_cases.cases()[e]["turn"])
                                             for e in range(0, 10)])]
    plain = solve(b, t)
    assert (plain[2] == SOLVED).all()
    bt, tt = dev(b, t)
    for window in ((-65, 65), (i8(np.full(len(t), -65)), 65), (-65, i8(np.full(len(t), 65)))):
        r = ops.solve(bt, tt, max_empties=12, node_limit=NODE_LIMIT, want_nodes=True, window=window)
        torch.cuda.synchronize()
        got = (r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy(),
               r.nodes.cpu().numpy().view(np.uint32))
        for x, y in zip(got, plain):
            assert (x == y).all()
    for te in (3, 6):
        p, w = solve(b, t, task_empties=te, nodes_per_position=1024), solve(b, t, task_empties=te, window=(-65, 65),
                                                                            nodes_per_position=1024)
        for x, y in zip(p[:3], w[:3]):
            assert (x == y).all()


# ---------------------------------------------------------------- 2. the split solver
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3, 6])
def test_split_matches_the_helper_in_every_family(task_empties, order):
    b, t, a, be, rv, rm, fam = checker_batch()
    got = solve(b, t, a, be, task_empties=task_empties, order=order, nodes_per_position=1024)
    assert_same(got, (rv, rm), (task_empties, order))
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [4, 8])
@pytest.mark.parametrize("e,k", [(10, 64), (12, 16)])
def test_split_equals_the_one_lane_windowed_call(e, k, task_empties, order):
    b, t, a, be, rv, rm = ladder_batch(e, k)
    got = solve(b, t, a, be, max_empties=e, task_empties=task_empties, order=order, nodes_per_position=4096)
    assert_same(got, (rv, rm), (e, task_empties, order))


# ---------------------------------------------------------------- 3. the deep fixture
def deep_wld(**kw):
    b, t, rv, rm, emp = fixture()
    bt, tt = dev(b, t)
    r = ops.solve(bt, tt, max_empties=16, node_limit=NODE_LIMIT, task_empties=8, order=1, wld=True, **kw)
    torch.cuda.synchronize()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy().astype(np.int64), r.status.cpu().numpy()


def check_deep(got, alpha, beta, what):
    v, m, s = got[:3]
    rv, rm, known = fixture_expect(alpha, beta)
    assert (s == SOLVED).all(), (what, s)
    assert (v == rv).all(), (what, v, rv)
    assert (m[known] == rm[known]).all(), (what, m, rm, known)
    return known


def test_fixture_win_draw_loss_in_one_launch():
    b, t, rv, rm, emp = fixture()
    assert len(t) == 38
    got = deep_wld()
    known = check_deep(got, np.full(38, -1), np.full(38, 1), "wld")
    assert (got[0] == np.sign(rv)).all()
    assert known[emp <= 14].all() and (got[1][(rv < 0) & (rm < 64)] == 255).all()
    # a winning move of a root the fixture cannot name is at least a legal move
    own = oracle.legal(b, solve_ref.mover(t))
    for i in np.nonzero(~known)[0]:
        assert int(own[i]) >> int(got[1][i]) & 1
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("name", ["around"] + list(window_ref.ON_BOUND))
def test_fixture_at_13_and_14_empties_with_the_value_inside_and_on_a_bound(name):
    b, t, rv, rm, emp = fixture()
    a, be, keep = window_ref.family(name, rv)
    assert keep.all()
    sel = emp <= 14
    got = solve(b[sel], t[sel], a[sel], be[sel], max_empties=14, task_empties=8, order=1)
    ev, em, known = fixture_expect(a, be)
    assert known[sel].all()
    assert_same(got, (ev[sel], em[sel]), name)


# ---------------------------------------------------------------- 4. timing independence
def test_the_grid_and_the_table_do_not_change_a_deep_answer(monkeypatch):
    want = deep_wld()
    assert (want[2] == SOLVED).all()
    lib = _lib.load()
    for blocks in ("512", "1024"):
        monkeypatch.setenv("OTH_SOLVE_BLOCKS", blocks)
        assert lib.othe_solve_grid(1 << 20) == int(blocks)
        got = deep_wld()
        for x, y in zip(got, want):
            assert (x == y).all(), blocks
    monkeypatch.delenv("OTH_SOLVE_BLOCKS")
    for bits in (4, 20):
        got = deep_wld(table=ops.SolveTable(bits, "cuda"))
        for x, y in zip(got, want):
            assert (x == y).all(), bits
    # a table filled by a full-window solve is valid input to the windowed one, and the other way round
    b, t, rv, rm, emp = fixture()
    table = ops.SolveTable(20, "cuda")
    exact = solve(b, t, task_empties=8, order=1, table=table)
    assert_same(exact, (rv, rm), "full window, empty table")
    got = deep_wld(table=table)
    for x, y in zip(got, want):
        assert (x == y).all()
    table = ops.SolveTable(20, "cuda")
    got = deep_wld(table=table)
    for x, y in zip(got, want):
        assert (x == y).all()
    assert_same(solve(b, t, task_empties=8, order=1, table=table), (rv, rm), "full window, table of the windowed call")
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 5. statuses
def status_batch():
    b, t, a, be, rv, rm, fam = checker_batch()
    pick = np.nonzero((solve_ref.empties(b) == 8) & (fam == 2))[0][:12]
    pool = solve_cases.pool()
    over = solve_cases.cases()[1]["over"]  # one empty square that neither side can take
    ob, ot = solve_cases.cases()[1]["boards"][over][:2], solve_cases.cases()[1]["turn"][over][:2]
    assert len(ot) == 2
    bad = np.array([[FULL ^ 0xF, 0x10]], np.uint64)  # overlaps on square 4
    boards = np.concatenate([pool[20]["boards"][:2], b[pick[:4]], bad, b[pick[4:8]], ob, b[pick[8:]]])
    turn = np.concatenate([pool[20]["turn"][:2], t[pick[:4]], [1], t[pick[4:8]], ot, t[pick[8:]]]).astype(np.uint8)
    alpha = np.concatenate([[66, 0], a[pick[:4]], [3], [0, 2, 66, -66], [4, -65], a[pick[8:]]])
    beta = np.concatenate([[0, 1], be[pick[:4]], [3], [0, 1, 67, 0], [5, -64], be[pick[8:]]])
    kind = np.concatenate([[SKIPPED] * 2, [SOLVED] * 4, [INVALID], [BADWINDOW] * 4, [SOLVED] * 6])
    r = window_ref.roots(ob, ot)
    ov, om = window_ref.expect(r, [4, -65], [5, -64])
    assert (om == 255).all()
    value = np.concatenate([[0] * 2, rv[pick[:4]], [0] * 5, ov, rv[pick[8:]]])
    move = np.concatenate([[255] * 2, rm[pick[:4]], [255] * 5, om, rm[pick[8:]]])
    return boards, turn, alpha, beta, kind, value, move


@pytest.mark.parametrize("task_empties", [None, 4])
def test_one_batch_mixes_skipped_invalid_bad_window_and_finished_roots(task_empties):
    """The statuses that are not windows' are classified first: a skipped or
    invalid root with a bad window keeps its own status.  Bad windows: alpha ==
    beta, alpha > beta, 66 and -66."""
    boards, turn, alpha, beta, kind, value, move = status_batch()
    kw = {} if task_empties is None else dict(task_empties=task_empties, order=1)
    v, m, s, nd = solve(boards, turn, alpha, beta, max_empties=12, **kw)
    assert (s == kind).all(), (s, kind)
    assert (v == value).all() and (m == move).all(), (v, value, m, move)
    assert (nd[kind != SOLVED] == 0).all()
    assert ops.work_word("cuda").item() == 0


def test_node_limit_one_and_failed_calls_leave_the_work_word_zero():
    b, t = solve_cases.ladder(12, 16)
    for kw in (dict(), dict(task_empties=10, order=0), dict(task_empties=10, order=1)):
        v, m, s, _ = solve(b, t, max_empties=12, node_limit=1, wld=True, **kw)
        assert (s == LIMIT).all() and (v == 0).all() and (m == 255).all()
        assert ops.work_word("cuda").item() == 0
    bt, tt = dev(b, t)
    for bad in (dict(max_empties=13), dict(max_empties=17, task_empties=8), dict(task_empties=13),
                dict(task_empties=8, nodes_per_position=63)):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.solve(bt, tt, **{**dict(max_empties=12, wld=True), **bad})
        torch.cuda.synchronize()
        assert ops.work_word("cuda").item() == 0
    for window in ((-66, 0), (0, 66), (3, 3), (5, -5), (0,), 7, (0.5, 1)):
        with pytest.raises(ValueError):
            ops.solve(bt, tt, window=window)
    with pytest.raises(ValueError):
        ops.solve(bt, tt, window=(-1, 1), wld=True)
    with pytest.raises((ValueError, TypeError)):
        ops.solve(bt, tt, window=(torch.zeros(len(tt), dtype=torch.int32, device="cuda"), 1))
    e = ops.solve(bt[:0], tt[:0], wld=True, want_nodes=True)
    assert e.value.numel() == e.status.numel() == e.nodes.numel() == 0
    e = ops.solve(bt[:0], tt[:0], wld=True, task_empties=6)
    assert e.value.numel() == 0


# ---------------------------------------------------------------- 6. special roots
def test_forced_passes_at_the_root_with_windows_on_both_sides_of_the_value():
    c = solve_cases.cases()
    b = np.concatenate([c[e]["boards"][c[e]["forced_pass"]] for e in range(2, 10)])
    t = np.concatenate([c[e]["turn"][c[e]["forced_pass"]] for e in range(2, 10)])
    V = np.concatenate([c[e]["value"][c[e]["forced_pass"]] for e in range(2, 10)]).astype(np.int64)
    assert len(t) >= 8
    for a, be in ((V, V + 1), (V - 1, V), (np.clip(V + 3, -65, 64), np.full_like(V, 65)),
                  (np.full_like(V, -65), np.clip(V - 3, -64, 65)), (V - 1, V + 1)):
        want = np.clip(V, a, be)
        for kw in (dict(), dict(task_empties=3, order=1, nodes_per_position=1024)):
            v, m, s, _ = solve(b, t, a, be, **kw)
            assert (s == SOLVED).all() and (v == want).all() and (m == 64).all(), (kw, v, want, m)


def test_the_eight_images_of_a_root_keep_their_own_lowest_qualifying_square():
    """Against the helper at 8 empties, under the open window and a fail-high
    one (beta = V - 2: every move within two discs of the best qualifies, and
    which of them is lowest differs from image to image)."""
    b, t = solve_cases.ladder(8, 8)
    ib = np.array([[bb, ww] for k in range(8) for bb, ww in
                   zip(tree_cases.symmetries(int(b[k, 0])), tree_cases.symmetries(int(b[k, 1])))], np.uint64)
    it = np.repeat(t, 8)
    r = window_ref.roots(ib, it)
    assert (r.value.reshape(8, 8) == r.value.reshape(8, 8)[:, :1]).all()
    for a, be in ((np.full(64, -65), np.full(64, 65)), (np.full(64, -65), np.clip(r.value - 2, -64, 65))):
        rv, rm = window_ref.expect(r, a, be)
        assert max(len(set(row.tolist())) for row in rm.reshape(8, 8)) > 1
        assert_same(solve(ib, it, a, be), (rv, rm), "one lane")
        for te in (3, 6):
            assert_same(solve(ib, it, a, be, task_empties=te, order=1, nodes_per_position=1024), (rv, rm), te)


# ---------------------------------------------------------------- 7. graph capture
def test_the_one_lane_form_is_captured_with_tensor_windows_and_replayed():
    b, t, a, be, rv, rm, fam = checker_batch()
    sel = np.nonzero(solve_ref.empties(b) == 7)[0]
    bt, tt = dev(b[sel], t[sel])
    at, bet = i8(a[sel]), i8(be[sel])
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        r = ops.solve(bt, tt, max_empties=12, node_limit=NODE_LIMIT, work=w, window=(at, bet))
    for _ in range(2):
        r.value.zero_(), r.best_move.zero_(), r.status.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same((r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy().astype(np.int64),
                     r.status.cpu().numpy()), (rv[sel], rm[sel]), "replay")
        assert w.item() == 0
    # the windows are read at replay: the full window in the same tensors gives the exact answers
    at.fill_(-65), bet.fill_(65)
    g.replay()
    torch.cuda.synchronize()
    exact = solve(b[sel], t[sel])
    assert (r.value.cpu().numpy() == exact[0]).all() and (r.best_move.cpu().numpy() == exact[1]).all()


# ---------------------------------------------------------------- 8. the engine and the env
def engine_on(i, **kw):
    b, t, rv, rm, emp = fixture()
    eng = engine.Engine(name="S", policy="greedy", **kw)
    text = oracle.serialize_str(b[i, 0], b[i, 1], t[i])
    eng.board.deserialize(text[:64], text[65], 0)
    assert eng.board.bitboards() == (int(b[i, 0]), int(b[i, 1])) and eng.board.turn == int(t[i])
    out = []
    eng.handle("go", out.append)
    return codec.parse_engine_go("".join(out))[1]


def test_engine_plays_the_proved_win_and_the_policys_move_on_a_proved_loss():
    b, t, rv, rm, emp = fixture()
    ri, sq, cv = fixture_root_moves()
    win = int(np.nonzero((emp == 14) & (rm < 64) & (rv > 0))[0][0])
    loss = int(np.nonzero((emp == 14) & (rm < 64) & (rv < 0))[0][0])
    kw = dict(solve_wld_empties=14, solve_task_empties=8)
    assert engine_on(win, **kw) == sq[(ri == win) & (cv >= 1)].min()
    assert engine_on(loss, **kw) == engine_on(loss)  # greedy's move: the solver proved no move
    # below solve_empties the exact solve still answers
    assert engine_on(loss, solve_empties=14, solve_task_empties=8) == rm[loss]
    out = []
    engine.Engine(name="S", policy="greedy", solve_empties=10, **kw).handle("verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=10 solve_wld_empties=14 solve_task_empties=8"]
    out = []
    engine.Engine(name="S", policy="greedy", solve_wld_empties=12).handle("verbose p", out.append)
    assert out == ["S policy=greedy solve_wld_empties=12"]


def test_env_solve_takes_wld_and_a_window():
    from subproc_amd.env import VecEnv

    b, t, a, be, rv, rm, fam = checker_batch()
    sel = np.nonzero((solve_ref.empties(b) == 8) & (fam == 1))[0]
    env = VecEnv(len(sel), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(b[sel]), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(t[sel])).cuda())
    for kw in (dict(wld=True), dict(window=(-1, 1)), dict(wld=True, task_empties=4, order=1)):
        r = env.solve(max_empties=12, node_limit=NODE_LIMIT, **kw)
        torch.cuda.synchronize()
        assert_same((r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy().astype(np.int64),
                     r.status.cpu().numpy()), (rv[sel], rm[sel]), kw)
