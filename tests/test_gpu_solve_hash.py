"""ops.solve(task_empties=..., table=...) / othh_solve_hashed on the GPU: the
split solver with its transposition table gives the answers it gives without
one.  Against the exhaustive checker (tests/solve_ref.py) at 0..9 empties and
on the synthetic boards, against the deep fixture at 13..16 empties, bit for
bit against the one-lane solver at 12 empties; ties; 64 twins of one root
fighting over the same slots; one table, never cleared, through calls of either
order, other task sizes and other batches; the arguments; the engine.

Unless a case says otherwise it runs on the smallest table (16 entries: every
store replaces and every slot is fought over) and on 2**20 entries, with
hash_min_empties 1 (every frame probes and stores) and with the default.
Every comparison asserts status == SOLVED for every root first."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import oracle
import solve_cases
import solve_ref
import synthetic_cases as sc

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, codec, engine, ops  # noqa: E402

SKIPPED, SOLVED, INVALID, LIMIT = _lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT
FULL = (1 << 64) - 1
NODE_LIMIT = 1 << 26  # as tests/test_gpu_solve_tree.py: a defect ends as LIMIT, which every test below refuses
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLEST, LARGE = _lib.SOLVE_HASH_MIN_BITS, 20
DEFAULT_GATE = _lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES
# (table bits, hash_min_empties)
TABLES = [(SMALLEST, 1), (SMALLEST, DEFAULT_GATE), (LARGE, 1), (LARGE, DEFAULT_GATE)]
tables = pytest.mark.parametrize("bits,gate", TABLES)


def dev(boards, turn):
    return (ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda"),
            torch.from_numpy(np.array(turn, np.uint8)).cuda())


def answers(r):
    torch.cuda.synchronize()
    return r.value.cpu().numpy().astype(np.int64), r.best_move.cpu().numpy(), r.status.cpu().numpy()


def hashed(boards, turn, task_empties, order, table, gate, max_empties=16, node_limit=NODE_LIMIT, **kw):
    """ops.solve with the table: (value, move, status)."""
    assert (1 << SMALLEST) <= 16
    b, t = dev(boards, turn)
    return answers(ops.solve(b, t, max_empties=max_empties, node_limit=node_limit, task_empties=task_empties,
                             order=order, table=table, hash_min_empties=gate, **kw))


def fresh(bits):
    return ops.SolveTable(bits, "cuda")


@functools.lru_cache(maxsize=None)
def lane_solve(e, k):
    """The one-lane solver's answers on solve_cases.ladder(e, k)."""
    b, t = solve_cases.ladder(e, k)
    assert len(t) == k and (solve_ref.empties(b) == e).all()
    bt, tt = dev(b, t)
    out = (b, t) + answers(ops.solve(bt, tt, max_empties=e, node_limit=NODE_LIMIT))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "solve_deep", "solve_deep.npz"))
    out = (fx["boards"], fx["turn"], fx["value"].astype(np.int64), fx["best_move"], fx["empties"].astype(np.int64))
    for a in out:
        a.setflags(write=False)
    return out


def assert_same(got, want, what):
    (v, m, s), (rv, rm) = got, want
    assert (s == SOLVED).all(), (what, np.nonzero(s != SOLVED)[0][:8], s[s != SOLVED][:8])
    bad = np.nonzero((v != rv) | (m != rm))[0]
    assert len(bad) == 0, (what, bad[:8], v[bad[:8]], rv[bad[:8]], m[bad[:8]], rm[bad[:8]])


# ---------------------------------------------------------------- 1. the checker
@tables
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [1, 3, 6])
def test_matches_the_checker_at_0_to_9_empties(task_empties, order, bits, gate):
    """One table through all ten emptinesses (tests/test_gpu_solve_tree.py
    asserts the pool's forced passes and game-overs)."""
    cases = solve_cases.cases()
    assert sorted(cases) == list(range(10))
    table = fresh(bits)
    for e, c in sorted(cases.items()):
        got = hashed(c["boards"], c["turn"], task_empties, order, table, gate, nodes_per_position=4096)
        assert_same(got, (c["value"], c["best_move"]), (e, task_empties, order))
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 2. synthetic boards
@tables
@pytest.mark.parametrize("order", [0, 1])
def test_matches_the_checker_on_the_synthetic_boards(order, bits, gate):
    """Lopsided and island boards (passes and finished games inside the tasks)
    and the edge boards, tasks of 3 and of 6 empties."""
    table = fresh(bits)
    for name in ("lopsided6", "lopsided8", "islands6", "islands8"):
        b, t = sc.solver_inputs(name)
        rv, rm, _ = sc.solver_reference(name)
        for task_empties in (3, 6):
            assert_same(hashed(b, t, task_empties, order, table, gate), (rv, rm), (name, task_empties))
    b, t, _ = sc.edges()
    rv, rm, _ = solve_ref.solve(b, t)
    small = solve_ref.empties(b) <= 12
    for task_empties in (1, 3):
        v, m, s = hashed(b, t, task_empties, order, table, gate, max_empties=12)
        assert (s == np.where(small, SOLVED, SKIPPED)).all()
        assert_same((v[small], m[small], s[small]), (rv[small].astype(np.int64), rm[small]), ("edges", task_empties))
        assert (v[~small] == 0).all() and (m[~small] == 255).all()
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 3. ties
@tables
@pytest.mark.parametrize("order", [0, 1])
def test_ties_keep_each_images_own_lowest_square(order, bits, gate):
    """Tied roots, 16 images each in one call: an image's twin positions fill
    the table the other images read, and each image keeps its own lowest
    maximiser."""
    b, t, rv, rm = sc.tie_roots("solve")
    assert len(t) == 16 * 8
    table = fresh(bits)
    for task_empties in (1, 3, 5):
        assert_same(hashed(b, t, task_empties, order, table, gate), (rv, rm), task_empties)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 4. the deep fixture
@tables
@pytest.mark.parametrize("task_empties,order", [(8, 1), (10, 1), (8, 0)])
def test_matches_the_fixture_at_13_to_16_empties(task_empties, order, bits, gate):
    """Order 0 on the 28 roots of at most 14 empties only: at 16 empties it
    takes tens of seconds."""
    b, t, rv, rm, emp = fixture()
    assert len(t) == 38 and emp.min() == 13 and emp.max() == 16
    sel = np.ones(38, bool) if order == 1 else emp <= 14
    assert sel.sum() == (38 if order == 1 else 28)
    got = hashed(b[sel], t[sel], task_empties, order, fresh(bits), gate)
    assert_same(got, (rv[sel], rm[sel]), (task_empties, order))
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 5. the one-lane solver
@tables
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("task_empties", [4, 8])
def test_equals_the_one_lane_solver(task_empties, order, bits, gate):
    b, t, rv, rm, rs = lane_solve(12, 16)
    assert (rs == SOLVED).all()
    v, m, s = hashed(b, t, task_empties, order, fresh(bits), gate, max_empties=12)
    assert (s == rs).all()
    assert_same((v, m, s), (rv, rm), (task_empties, order))
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 6. contention
@tables
@pytest.mark.parametrize("order", [0, 1])
def test_64_twins_of_one_root_fight_over_the_same_slots(order, bits, gate):
    b, t, rv, rm, rs = lane_solve(12, 16)
    k = 5
    tb, tt = np.repeat(b[k:k + 1], 64, axis=0), np.repeat(t[k:k + 1], 64)
    got = hashed(tb, tt, 8, order, fresh(bits), gate, max_empties=12)
    assert_same(got, (np.repeat(rv[k], 64), np.repeat(rm[k], 64)), order)
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 7. persistence and mixing
def children(boards, turn, moves):
    """Every root after its move (one ops.step each; 64 is a pass, which step plays)."""
    b, t = dev(boards, turn)
    r = ops.step(b, t, torch.from_numpy(np.asarray(moves, np.uint8)).cuda())
    torch.cuda.synchronize()
    return ops.to_numpy_u64(r.boards), r.turn.cpu().numpy()


@pytest.mark.parametrize("bits,gate", [(SMALLEST, 1), (LARGE, 1), (LARGE, DEFAULT_GATE)])
def test_one_table_through_calls_of_both_orders_other_task_sizes_and_other_batches(bits, gate):
    b, t, rv, rm, emp = fixture()
    sel = emp <= 14
    b, t, rv, rm = b[sel], t[sel], rv[sel], rm[sel]
    table = fresh(bits)
    assert_same(hashed(b, t, 10, 1, table, gate), (rv, rm), "order 1")
    assert_same(hashed(b, t, 10, 0, table, gate), (rv, rm), "order 0 on order 1's table")
    # every child of those roots, named by the checker's helpers, with another task size
    own = oracle.legal(b, solve_ref.mover(t))
    idx, sq = solve_ref._bits(own)
    passes = np.nonzero(own == 0)[0]
    idx, sq = np.concatenate([idx, passes]), np.concatenate([sq, np.full(len(passes), 64)])
    cb, ct = children(b[idx], t[idx], sq)
    assert (solve_ref.empties(cb) == solve_ref.empties(b[idx]) - (sq < 64)).all()
    kept = hashed(cb, ct, 8, 1, table, gate)
    new = hashed(cb, ct, 8, 1, fresh(bits), gate)
    assert (kept[2] == SOLVED).all() and (new[2] == SOLVED).all()
    assert (kept[0] == new[0]).all() and (kept[1] == new[1]).all()
    # and the fixture's: a root's value is the best of minus its children's, its move the lowest square there
    for i in range(len(t)):
        mine = idx == i
        assert rv[i] == (-kept[0][mine]).max()
        assert rm[i] == sq[mine][np.nonzero(-kept[0][mine] == rv[i])[0][0]]
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("bits", [SMALLEST, LARGE])
def test_a_table_filled_at_0_to_9_empties_serves_the_13_empties_roots(bits):
    table = fresh(bits)
    for e, c in sorted(solve_cases.cases().items()):
        assert_same(hashed(c["boards"], c["turn"], 3, 1, table, 1), (c["value"], c["best_move"]), e)
    assert bits == SMALLEST or int((table.data != 0).sum()) > 0
    b, t, rv, rm, emp = fixture()
    sel = emp == 13
    assert_same(hashed(b[sel], t[sel], 10, 1, table, 1), (rv[sel], rm[sel]), "13 empties")
    assert_same(hashed(b[sel], t[sel], 8, 0, table, DEFAULT_GATE), (rv[sel], rm[sel]), "13 empties again")
    assert ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 8. the arguments
def test_arguments():
    b, t, rv, rm, rs = lane_solve(12, 16)
    bt, tt = dev(b, t)
    table = fresh(SMALLEST)
    with pytest.raises(ValueError, match="task_empties"):
        ops.solve(bt, tt, max_empties=12, table=table)
    for gate in (0, 13):
        with pytest.raises(ValueError):
            ops.solve(bt, tt, max_empties=12, task_empties=8, table=table, hash_min_empties=gate)
    for bits in (SMALLEST - 1, _lib.SOLVE_HASH_MAX_BITS + 1):
        with pytest.raises(ValueError):
            ops.SolveTable(bits, "cuda")
    with pytest.raises(TypeError):
        ops.solve(bt, tt, max_empties=12, task_empties=8, table=table.data)
    assert table.nbytes == _lib.load().othh_hash_bytes(SMALLEST) == 16 * 32 and int((table.data != 0).sum()) == 0
    # the split solver's own checks hold, and leave the work word alone
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        ops.solve(bt, tt, max_empties=17, task_empties=8, table=table)
    torch.cuda.synchronize()
    assert ops.work_word("cuda").item() == 0
    # a short table, through the C-ABI: refused before any launch
    lib = _lib.load()
    val = torch.full((16,), 77, dtype=torch.int8, device="cuda")
    scratch = torch.empty(lib.othe_scratch_bytes(16, 4096) // 8, dtype=torch.int64, device="cuda")
    w = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call(bits, nbytes, n=16, ptr=table.data.data_ptr()):
        return lib.othh_solve_hashed(bt.data_ptr(), tt.data_ptr(), 12, 8, 1, NODE_LIMIT, val.data_ptr(), None, None, None,
                                     scratch.data_ptr(), scratch.numel() * 8, 4096, w.data_ptr(), n, bits, 1, ptr, nbytes,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(SMALLEST + 1, table.nbytes) == _lib.OTH_EINVAL
    assert call(SMALLEST, table.nbytes - 1) == _lib.OTH_EINVAL
    assert call(SMALLEST, table.nbytes, ptr=table.data.data_ptr() + 8) == _lib.OTH_EINVAL
    assert call(SMALLEST, table.nbytes, ptr=None) == _lib.OTH_EINVAL
    assert call(SMALLEST, table.nbytes, n=0) == _lib.OTH_OK  # launches nothing
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == 77).all() and w.item() == 0 and int((table.data != 0).sum()) == 0
    assert call(SMALLEST, table.nbytes) == _lib.OTH_OK
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == rv).all() and w.item() == 0
    e = ops.solve(bt[:0], tt[:0], max_empties=12, task_empties=8, table=table, want_nodes=True)
    assert e.value.numel() == e.status.numel() == e.nodes.numel() == 0


@pytest.mark.parametrize("bits,gate", [(SMALLEST, 1), (LARGE, DEFAULT_GATE)])
def test_one_batch_mixed_with_skipped_and_invalid_roots(bits, gate):
    """tests/test_gpu_solve_tree.py's mixed batch, with the table."""
    b, t, rv, rm, _ = fixture()
    pool = solve_cases.pool()
    deep_b = np.concatenate([pool[17]["boards"][:3], pool[20]["boards"][:2], pool[40]["boards"][:1]])
    deep_t = np.concatenate([pool[17]["turn"][:3], pool[20]["turn"][:2], pool[40]["turn"][:1]])
    bad_b = np.array([[FULL ^ 0xF, 0x10]], np.uint64)  # overlaps on square 4
    boards = np.concatenate([deep_b[:3], b[:20], bad_b, deep_b[3:], b[20:]])
    turn = np.concatenate([deep_t[:3], t[:20], [1], deep_t[3:], t[20:]]).astype(np.uint8)
    kind = np.concatenate([np.full(3, SKIPPED), np.full(20, SOLVED), [INVALID], np.full(3, SKIPPED), np.full(18, SOLVED)])
    bt, tt = dev(boards, turn)
    table = fresh(bits)
    r = ops.solve(bt, tt, max_empties=16, node_limit=NODE_LIMIT, task_empties=10, order=1, want_nodes=True, table=table,
                  hash_min_empties=gate)
    v, m, s = answers(r)
    nd = r.nodes.cpu().numpy().view(np.uint32)
    assert (s == kind).all(), (s, kind)
    assert (v[kind == SOLVED] == rv).all() and (m[kind == SOLVED] == rm).all()
    assert (v[kind != SOLVED] == 0).all() and (m[kind != SOLVED] == 255).all() and (nd[kind != SOLVED] == 0).all()
    assert (nd[kind == SOLVED] > 0).all()
    assert ops.work_word("cuda").item() == 0
    v, m, s = hashed(b, t, 10, 1, table, gate, max_empties=14)
    emp = fixture()[4]
    assert (s == np.where(emp <= 14, SOLVED, SKIPPED)).all()
    assert (v == np.where(emp <= 14, rv, 0)).all() and (m == np.where(emp <= 14, rm, 255)).all()


def test_env_solve_takes_the_table():
    from subproc_amd.env import VecEnv

    b, t, rv, rm, rs = lane_solve(12, 16)
    env = VecEnv(len(t), device="cuda")
    env.boards.copy_(ops.from_numpy_u64(np.array(b), "cuda"))
    env.turn.copy_(torch.from_numpy(np.array(t)).cuda())
    table = fresh(12)
    for _ in range(2):  # the second call on what the first left
        v, m, s = answers(env.solve(max_empties=12, node_limit=NODE_LIMIT, task_empties=8, order=1, table=table,
                                    hash_min_empties=4))
        assert_same((v, m, s), (rv, rm), "env")
    assert int((table.data != 0).sum()) > 0 and ops.work_word("cuda").item() == 0


# ---------------------------------------------------------------- 9. the engine
def play_out(eng, b, w, turn):
    text = oracle.serialize_str(b, w, turn)
    eng.board.deserialize(text[:64], text[65], 0)
    moves = []
    while not eng.board.is_game_over():
        out = []
        eng.handle("go", out.append)
        moves.append("".join(out))
        assert len(moves) <= 40
    return moves


def test_engine_with_a_table_plays_the_moves_of_the_engine_without():
    b, t, rv, rm, emp = fixture()
    i = int(np.nonzero((emp == 14) & (rm < 64))[0][0])
    hashed_eng = engine.Engine(name="S", policy="greedy", solve_empties=14, solve_task_empties=8, solve_hash_bits=16)
    plain_eng = engine.Engine(name="S", policy="greedy", solve_empties=14, solve_task_empties=8)
    got = play_out(hashed_eng, int(b[i, 0]), int(b[i, 1]), int(t[i]))
    want = play_out(plain_eng, int(b[i, 0]), int(b[i, 1]), int(t[i]))
    assert got == want and len(got) >= 10
    assert ops.work_word("cuda").item() == 0
    assert codec.parse_engine_go(got[0])[1] == int(rm[i])
    # one table for the engine's life, filled by the game
    assert hashed_eng._solve_table is not None and hashed_eng._solve_table.bits == 16
    assert int((hashed_eng._solve_table.data != 0).sum()) > 0 and plain_eng._solve_table is None
    out = []
    hashed_eng.handle("verbose p", out.append)
    assert out == ["S policy=greedy solve_empties=14 solve_task_empties=8 solve_hash_bits=16"]
    for bad in (dict(solve_empties=12, solve_hash_bits=16), dict(solve_empties=14, solve_task_empties=8, solve_hash_bits=3),
                dict(solve_empties=14, solve_task_empties=8, solve_hash_bits=27)):
        with pytest.raises(ValueError):
            engine.Engine(**bad)
    with pytest.raises(SystemExit):
        engine.main(["--solve-empties", "12", "--solve-hash-bits", "16"])
