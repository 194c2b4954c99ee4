"""ops.solve / oths_solve on the GPU against the exhaustive checker
(tests/solve_ref.py over the C oracle): every value, best move and status at
0..9 empties, hand-built corner cases, a ladder that chains 10..12 empties down
to the checked levels, and the launch plumbing (shapes, refill, work word,
node limit)."""
import numpy as np
import pytest
import torch

import oracle
import solve_cases
import solve_ref

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402

SOLVED, SKIPPED, INVALID, LIMIT = _lib.SOLVE_SOLVED, _lib.SOLVE_SKIPPED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
FULL = (1 << 64) - 1
# no tree at <= 9 empties of the pool needs more than 23,082 nodes and none of
# the ladder's more than 2,315,382 (host build of the same state machine): a
# defect ends as LIMIT, not as a long kernel
LIMIT_9, LIMIT_LADDER = 1 << 18, 1 << 23


def gpu_solve(boards, turn, **kw):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    t = torch.from_numpy(np.array(turn, np.uint8)).cuda()
    r = ops.solve(b, t, want_nodes=True, **kw)
    torch.cuda.synchronize()
    return (r.value.cpu().numpy(), r.best_move.cpu().numpy(), r.status.cpu().numpy(),
            r.nodes.cpu().numpy().view(np.uint32))


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("e", range(10))
def test_every_value_and_move_matches_the_checker(e):
    c = solve_cases.cases()[e]
    v, m, s, nd = gpu_solve(c["boards"], c["turn"], max_empties=e, node_limit=LIMIT_9)
    assert (s == SOLVED).all()
    bad = np.nonzero((v != c["value"]) | (m != c["best_move"]))[0]
    assert len(bad) == 0, (e, bad[:8], v[bad[:8]], c["value"][bad[:8]], m[bad[:8]], c["best_move"][bad[:8]])
    assert (m[c["forced_pass"]] == 64).all() and (m[c["over"]] == 255).all()
    assert (nd[c["over"]] == 0).all() and (nd[~c["over"]] >= 1).all()


def test_cases_cover_passes_and_early_ends():
    cs = solve_cases.cases()
    for e in range(1, 10):
        assert cs[e]["forced_pass"].any(), e
    assert any(cs[e]["over"].any() for e in range(1, 10))
    assert sum(cs[e]["inner_passes"] for e in cs) >= 1
    assert {1, 2} <= set(np.concatenate([cs[e]["turn"] for e in cs]).tolist())
    for e, k in solve_cases.OTHERS.items():
        assert (~(cs[e]["forced_pass"] | cs[e]["over"])).sum() == (k if e else 0), e


# ---------------------------------------------------------------- hand-built
def test_hand_built_positions():
    a1_b1 = 0b11
    rows = [
        # full board, 33 black / 31 white
        ((0x1FFFFFFFF, FULL ^ 0x1FFFFFFFF, 1), (2, 255, SOLVED)),
        ((0x1FFFFFFFF, FULL ^ 0x1FFFFFFFF, 2), (-2, 255, SOLVED)),
        # wipe-out: 20 black discs, no white one, 44 empties > 12: skipped ...
        ((0xFFFFF, 0, 1), (0, 255, SKIPPED)),
        # ... and with 5 empties: over at once
        ((FULL ^ 0x1F, 0, 1), (59, 255, SOLVED)),
        ((FULL ^ 0x1F, 0, 2), (-59, 255, SOLVED)),
        # 60 black discs, 4 empties, no white disc
        ((FULL ^ 0xF, 0, 1), (60, 255, SOLVED)),
        ((FULL ^ 0xF, 0, 2), (-60, 255, SOLVED)),
        # only the opponent can move: a1 empty, b1 white, the rest black; White to move passes, Black takes all
        ((FULL ^ a1_b1, 2, 2), (-64, 64, SOLVED)),
        ((FULL ^ a1_b1, 2, 1), (64, 0, SOLVED)),
        # turn 0 and 3 are Black
        ((FULL ^ a1_b1, 2, 0), (64, 0, SOLVED)),
        ((FULL ^ a1_b1, 2, 3), (64, 0, SOLVED)),
        # overlap
        ((FULL ^ 0xF, 0x10, 1), (0, 255, INVALID)),
        ((FULL, FULL, 2), (0, 255, INVALID)),
    ]
    boards = np.array([[r[0][0], r[0][1]] for r in rows], np.uint64)
    turn = np.array([r[0][2] for r in rows], np.uint8)
    v, m, s, nd = gpu_solve(boards, turn, node_limit=LIMIT_9)
    got = [(int(a), int(b), int(c)) for a, b, c in zip(v, m, s)]
    assert got == [r[1] for r in rows]
    valid = [i for i, r in enumerate(rows) if r[1][2] == SOLVED]
    rv, rm, _ = solve_ref.solve(boards[valid], turn[valid])
    assert (v[valid] == rv).all() and (m[valid] == rm).all()
    assert nd.tolist() == [0, 0, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 0]


def test_pass_root_is_the_negated_child_value():
    """Forced-pass roots of the pool: move 64 and minus the value of the same board with the other side to move."""
    cs = solve_cases.cases()
    b = np.concatenate([cs[e]["boards"][cs[e]["forced_pass"]] for e in range(1, 10)])
    t = np.concatenate([cs[e]["turn"][cs[e]["forced_pass"]] for e in range(1, 10)])
    v, m, s, _ = gpu_solve(b, t, node_limit=LIMIT_9)
    v2, m2, s2, _ = gpu_solve(b, (3 - t).astype(np.uint8), node_limit=LIMIT_9)
    assert (s == SOLVED).all() and (s2 == SOLVED).all()
    assert (m == 64).all() and (m2 < 64).all() and (v == -v2).all()


# ---------------------------------------------------------------- ladder
@pytest.mark.parametrize("e,k", [(10, 64), (11, 64), (12, 16)])
def test_ladder_value_is_the_best_child(e, k):
    b, t = solve_cases.ladder(e, k)
    assert len(t) == k
    own = oracle.legal(b, t)
    idx, sq = solve_ref._bits(own)
    kids = oracle.step(b[idx], t[idx], sq)["boards"]
    kv, _, ks, _ = gpu_solve(kids, (3 - t[idx]).astype(np.uint8), max_empties=e - 1, node_limit=LIMIT_LADDER)
    v, m, s, _ = gpu_solve(b, t, max_empties=e, node_limit=LIMIT_LADDER)
    assert (ks == SOLVED).all() and (s == SOLVED).all()
    for i in range(k):
        mine = idx == i
        score = -kv[mine].astype(np.int64)
        assert int(v[i]) == score.max(), i
        assert int(m[i]) == int(sq[mine][np.argmax(score)]), i  # argmax: the first = lowest square


# ---------------------------------------------------------------- shapes and plumbing
def mixed(n, lo=0, hi=6):
    """n pool positions cycling through lo..hi empties, with the checker's answers."""
    cs = solve_cases.cases()
    es = [lo + i % (hi - lo + 1) for i in range(n)]
    js = [(i // (hi - lo + 1)) % len(cs[e]["turn"]) for i, e in enumerate(es)]
    pick = lambda key: np.array([cs[e][key][j] for e, j in zip(es, js)])  # noqa: E731
    return pick("boards"), pick("turn"), pick("value"), pick("best_move"), np.array(es)


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_batch_sizes(n):
    b, t, rv, rm, _ = mixed(n)
    v, m, s, _ = gpu_solve(b, t, node_limit=LIMIT_9)
    assert (s == SOLVED).all() and (v == rv).all() and (m == rm).all()
    assert ops.work_word("cuda").item() == 0


def test_empty_batch_and_bad_arguments():
    b = torch.empty((0, 2), dtype=torch.int64, device="cuda")
    t = torch.empty(0, dtype=torch.uint8, device="cuda")
    r = ops.solve(b, t, want_nodes=True)
    assert r.value.numel() == r.best_move.numel() == r.status.numel() == r.nodes.numel() == 0
    lib = _lib.load()
    assert lib.oths_solve_grid(0) == 0 and lib.oths_solve_grid(-1) == _lib.OTH_EINVAL
    assert lib.oths_solve_grid(1) == 1 and lib.oths_solve_grid(65) == 2
    assert 2 <= lib.oths_solve_grid(1 << 30) <= 1 << 20
    bb, tt, *_ = mixed(4)
    bb = ops.from_numpy_u64(bb, "cuda")
    tt = torch.from_numpy(tt).cuda()
    for bad in (-1, _lib.SOLVE_MAX_EMPTIES + 1):
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            ops.solve(bb, tt, max_empties=bad)
    # the failed calls launched nothing and the stream's next launch finds a zero word
    r = ops.solve(bb, tt, node_limit=LIMIT_9)
    assert (r.status.cpu().numpy() == SOLVED).all() and ops.work_word("cuda").item() == 0


def test_positions_above_max_empties_are_skipped():
    b, t, rv, rm, es = mixed(500, 0, 9)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    n = len(t)
    val = torch.full((n,), 77, dtype=torch.int8, device="cuda")
    mv = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    nd = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    w = ops.work_word("cuda")
    rc = _lib.load().oths_solve(bt.data_ptr(), tt.data_ptr(), 5, LIMIT_9, val.data_ptr(), mv.data_ptr(), st.data_ptr(),
                                nd.data_ptr(), w.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    v, m, s, k = (x.cpu().numpy() for x in (val, mv, st, nd))
    deep = es > 5
    assert deep.any() and (~deep).any()
    assert (s[deep] == SKIPPED).all() and (v[deep] == 0).all() and (m[deep] == 255).all() and (k[deep] == 0).all()
    assert (s[~deep] == SOLVED).all() and (v[~deep] == rv[~deep]).all() and (m[~deep] == rm[~deep]).all()


def test_null_outputs():
    b, t, rv, rm, _ = mixed(300)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    n = len(t)
    w = ops.work_word("cuda")
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    val = torch.full((n,), 77, dtype=torch.int8, device="cuda")
    mv = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    assert lib.oths_solve(bt.data_ptr(), tt.data_ptr(), 12, LIMIT_9, None, None, None, None, w.data_ptr(), n,
                          stream) == 0
    assert lib.oths_solve(bt.data_ptr(), tt.data_ptr(), 12, LIMIT_9, val.data_ptr(), None, None, None, w.data_ptr(),
                          n, stream) == 0
    assert lib.oths_solve(bt.data_ptr(), tt.data_ptr(), 12, LIMIT_9, None, mv.data_ptr(), None, None, w.data_ptr(),
                          n, stream) == 0
    # turn NULL: Black everywhere
    vb = torch.empty(n, dtype=torch.int8, device="cuda")
    assert lib.oths_solve(bt.data_ptr(), None, 12, LIMIT_9, vb.data_ptr(), None, None, None, w.data_ptr(), n,
                          stream) == 0
    assert lib.oths_solve(bt.data_ptr(), tt.data_ptr(), 12, LIMIT_9, None, None, None, None, None, n,
                          stream) == _lib.OTH_EINVAL  # no work word
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == rv).all() and (mv.cpu().numpy() == rm).all() and w.item() == 0
    black = gpu_solve(b, np.ones(n, np.uint8), node_limit=LIMIT_9)[0]
    assert (vb.cpu().numpy() == black).all()


def test_results_do_not_depend_on_the_batch():
    b, t, rv, rm, _ = mixed(777, 0, 8)
    v, m, s, nd = gpu_solve(b, t, node_limit=LIMIT_9)
    perm = np.random.default_rng(5).permutation(len(t))
    vp, mp, sp, ndp = gpu_solve(b[perm], t[perm], node_limit=LIMIT_9)
    assert (vp == v[perm]).all() and (mp == m[perm]).all() and (sp == s[perm]).all() and (ndp == nd[perm]).all()
    v1, m1, s1, nd1 = gpu_solve(b[:5], t[:5], node_limit=LIMIT_9)
    assert (v1 == v[:5]).all() and (m1 == m[:5]).all() and (nd1 == nd[:5]).all()
    assert (v == rv).all() and (m == rm).all()


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_one_block_refills_through_the_whole_batch(blocks, monkeypatch):
    b, t, rv, rm, _ = mixed(1000)
    v0, m0, s0, nd0 = gpu_solve(b, t, node_limit=LIMIT_9)
    monkeypatch.setenv("OTH_SOLVE_BLOCKS", blocks)
    assert _lib.load().oths_solve_grid(1000) == int(blocks)
    v, m, s, nd = gpu_solve(b, t, node_limit=LIMIT_9)
    assert ops.work_word("cuda").item() == 0
    assert (v == rv).all() and (m == rm).all() and (s == SOLVED).all()
    assert (v == v0).all() and (m == m0).all() and (nd == nd0).all()


def test_work_word_is_shared_and_left_zero():
    b, t, rv, rm, _ = mixed(333)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.solve(bt, tt, node_limit=LIMIT_9, work=w)  # two launches back to back on one word
    r2 = ops.solve(bt, tt, node_limit=LIMIT_9, work=w)
    torch.cuda.synchronize()
    assert w.item() == 0
    assert (r1.value.cpu().numpy() == rv).all() and (r2.value.cpu().numpy() == rv).all()
    assert (r2.best_move.cpu().numpy() == rm).all()
    # a rollout and a solve share the stream's word
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r3 = ops.solve(bt, tt, node_limit=LIMIT_9)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    assert (r3.value.cpu().numpy() == rv).all() and (r3.best_move.cpu().numpy() == rm).all()
    assert torch.equal(g1.final_boards, g2.final_boards) and torch.equal(g1.hist, g2.hist)
    go = oracle.rollout(1000, 9)
    assert (ops.to_numpy_u64(g2.final_boards) == go["final_boards"]).all()


def test_argument_checks():
    b, t, *_ = mixed(8)
    bt, tt = ops.from_numpy_u64(b, "cuda"), torch.from_numpy(t).cuda()
    with pytest.raises(ValueError, match="32 bits"):
        ops.solve(bt, tt, node_limit=1 << 32)
    with pytest.raises(TypeError):
        ops.solve(bt, tt.to(torch.int32))


# ---------------------------------------------------------------- node limit
def test_node_limit_splits_exactly_at_the_count():
    c = solve_cases.cases()[8]
    b, t = c["boards"], c["turn"]
    v0, m0, s0, nd0 = gpu_solve(b, t, node_limit=LIMIT_9)
    assert (s0 == SOLVED).all()
    limit = int(np.sort(nd0)[len(nd0) // 2])  # a count that occurs: that position is still solved
    assert nd0.min() < limit < nd0.max()
    v, m, s, nd = gpu_solve(b, t, node_limit=limit)
    over = nd0 > limit
    assert over.any() and (~over).any() and (nd0 == limit).any()
    assert (s[over] == LIMIT).all() and (v[over] == 0).all() and (m[over] == 255).all() and (nd[over] == limit).all()
    assert (s[~over] == SOLVED).all() and (v[~over] == v0[~over]).all() and (m[~over] == m0[~over]).all()
    assert (nd[~over] == nd0[~over]).all() and (nd <= limit).all()
    # limit 1: only the positions of at most one node survive
    v, m, s, nd = gpu_solve(b, t, node_limit=1)
    assert ((s == SOLVED) == (nd0 <= 1)).all() and (nd <= 1).all()
