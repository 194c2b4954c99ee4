"""ops.perft / othc_perft on the GPU (include/othello_perft.h)
against the published opening values and tests/perft_ref.py's checker: leaves,
divide and status, whatever the split, the room, the grid and the launch
plumbing.  All comparisons are exact.  With the default node limit no position
of any test here may end as LIMIT."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import perft_cases
import perft_ref

pytestmark = pytest.mark.gpu

from subproc_amd import _lib, ops  # noqa: E402
from subproc_amd.env import VecEnv  # noqa: E402

OPENING_MOVES = [19, 26, 37, 44]  # d3, c4, f5, e6


def dev(boards, turn):
    b = ops.from_numpy_u64(np.array(boards, np.uint64).reshape(-1, 2), "cuda")  # (copies: the cases are read-only)
    return b, torch.from_numpy(np.array(turn, np.uint8)).cuda()


def unpack(r):
    torch.cuda.synchronize()
    return dict(leaves=r.leaves.cpu().numpy(), status=r.status.cpu().numpy().astype(np.int64),
                divide=None if r.divide is None else r.divide.cpu().numpy(),
                nodes=None if r.nodes is None else r.nodes.cpu().numpy())


def gpu(boards, turn, depth, **kw):
    kw.setdefault("want_divide", True)
    return unpack(ops.perft(*dev(boards, turn), depth, **kw))


def opening_is(got, depth, what):
    want = 1 if depth == 0 else perft_ref.OPENING[depth - 1]
    print(what, int(got["leaves"][0]), want)
    assert int(got["leaves"][0]) == want and got["status"][0] == _lib.PERFT_COUNTED, what
    if got["divide"] is not None:
        row = got["divide"][0]
        assert int(row.sum()) == (want if depth else 0), what
        assert not depth or (row[OPENING_MOVES] * 4 == want).all(), what  # (the opening's moves are images of one)
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("split", [5, 7])
@pytest.mark.parametrize("depth", range(1, 12))
def test_the_published_opening_values_to_depth_11(depth, split):
    opening_is(gpu(*perft_ref.opening(), depth, split=split), depth, (depth, split))


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("depth", range(0, 9))
def test_the_published_opening_values_from_one_lane_and_from_the_root_moves(depth, split):
    opening_is(gpu(*perft_ref.opening(), depth, split=split, want_divide=split > 0), depth, (depth, split))


def test_depth_12_over_a_million_tasks():
    got = gpu(*perft_ref.opening(), 12, split=8, max_tasks=1 << 20, want_nodes=True)
    opening_is(got, 12, "depth 12")
    assert got["nodes"][0] > 0


def test_midgame_positions_against_the_checker():
    g = oracle.sample_midgame(256, 0x5EED)
    want = perft_ref.perft(g["boards"], g["turn"], 4)
    for split in (0, 2):
        perft_cases.same(gpu(g["boards"], g["turn"], 4, split=split), want, ("midgame", split))
    got = gpu(g["boards"], g["turn"], 4, want_divide=False)
    assert got["divide"] is None and (got["leaves"] == want[0]).all()
    assert ops.work_word("cuda").item() == 0


@pytest.mark.parametrize("name", ["small", "endgames", "offtree"])
def test_the_host_tests_inputs_against_the_checker(name):
    b, t = perft_cases.inputs(name)
    for depth in perft_cases.DEPTHS[name]:
        want = perft_cases.reference(name, depth)
        for split, cap in ((0, 1 << 20), (1, 64), (3, 4096), (5, 1 << 18)):
            perft_cases.same(gpu(b, t, depth, split=split, max_tasks=cap), want, (name, depth, split, cap))
    assert ops.work_word("cuda").item() == 0


def test_per_position_depths_in_one_call():
    b, t, d, want = perft_cases.mixed()
    bt, tt = dev(b, t)
    dt = torch.from_numpy(np.array(d)).cuda()
    for split in (0, 3):
        perft_cases.same(unpack(ops.perft(bt, tt, dt, split=split, want_divide=True)), want, ("mixed", split))
    over = np.array(d)
    over[:3] = 15
    got = unpack(ops.perft(bt, tt, torch.from_numpy(over).cuda(), want_divide=True))
    assert (got["status"][:3] == _lib.PERFT_BADDEPTH).all() and not got["leaves"][:3].any()
    assert not got["divide"][:3].any() and (got["leaves"][3:] == want[0][3:]).all()


def test_the_answers_do_not_depend_on_the_grid_the_room_or_the_launch_plumbing(monkeypatch):
    b, t = perft_cases.inputs("small")
    want = perft_cases.reference("small", 4)
    ob, ot = perft_ref.opening()
    # lists of 64 tasks at split 5: the opening's fourth level (244 tasks) is void
    opening_is(gpu(ob, ot, 8, split=5, max_tasks=64), 8, "void levels")
    opening_is(gpu(ob, ot, 8, split=5, max_tasks=64, want_divide=False), 8, "void levels, no rows")
    perft_cases.same(gpu(b, t, 4, split=5, max_tasks=64), want, "void levels, batch")
    # one block
    monkeypatch.setenv("OTH_PERFT_BLOCKS", "1")
    assert _lib.load().othc_perft_grid(1000) == 1
    perft_cases.same(gpu(b, t, 4, split=2), want, "one block")
    opening_is(gpu(ob, ot, 7, split=3), 7, "one block")
    monkeypatch.delenv("OTH_PERFT_BLOCKS")
    assert _lib.load().othc_perft_grid(1000) >= 256
    # two calls sharing one work word on a stream, and the stream's word shared with a rollout
    bt, tt = dev(b, t)
    obt, ott = dev(ob, ot)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1 = ops.perft(bt, tt, 4, split=2, want_divide=True, work=w)
    r2 = ops.perft(obt, ott, 9, split=5, want_divide=True, work=w)
    torch.cuda.synchronize()
    assert w.item() == 0
    perft_cases.same(unpack(r1), want, "shared word")
    opening_is(unpack(r2), 9, "shared word")
    g1 = ops.rollout(1000, seed=9, device="cuda")
    r3 = ops.perft(bt, tt, 4)
    g2 = ops.rollout(1000, seed=9, device="cuda")
    torch.cuda.synchronize()
    assert (r3.leaves.cpu().numpy() == want[0]).all() and torch.equal(g1.hist, g2.hist)
    assert ops.work_word("cuda").item() == 0


def test_a_captured_graph_replayed_twice():
    b, t = perft_cases.inputs("small")
    want = perft_cases.reference("small", 3)
    bt, tt = dev(b, t)
    obt, ott = dev(*perft_ref.opening())
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            ops.perft(bt, tt, 3)
        r = ops.perft(bt, tt, 3, split=2, want_divide=True, want_nodes=True, work=w)
        s = ops.perft(obt, ott, 8, split=5, max_tasks=64, work=w)
    for _ in range(2):
        r.leaves.fill_(7), r.divide.fill_(7), r.status.zero_(), s.leaves.fill_(7)
        g.replay()
        perft_cases.same(unpack(r), want, "replay")
        assert int(s.leaves.cpu()[0]) == perft_ref.OPENING[7] and w.item() == 0


def test_the_node_limit():
    ob, ot = perft_ref.opening()
    got = gpu(ob, ot, 6, split=0, want_divide=False, node_limit=16, want_nodes=True)
    assert got["status"][0] == _lib.PERFT_LIMIT and got["leaves"][0] == 0 and got["nodes"][0] == 16
    got = gpu(ob, ot, 6, split=1, node_limit=16)
    assert got["status"][0] == _lib.PERFT_LIMIT and got["leaves"][0] == 0 and not got["divide"].any()
    # exactly the limit is counted; one task of a batch at the limit leaves its neighbours alone
    got = gpu(ob, ot, 6, split=0, want_divide=False, node_limit=1 + 4 + 12 + 56 + 244 + 1396, want_nodes=True)
    assert got["status"][0] == _lib.PERFT_COUNTED and got["leaves"][0] == 8200 and got["nodes"][0] == 1713
    b, t = perft_cases.inputs("endgames")
    b, t = np.concatenate([ob, b]), np.concatenate([ot, t])
    want = perft_cases.reference("endgames", 8)
    got = gpu(b, t, 8, split=0, want_divide=False, node_limit=4096)
    assert got["status"][0] == _lib.PERFT_LIMIT and got["leaves"][0] == 0
    assert (got["status"][1:] == want[2]).all() and (got["leaves"][1:] == want[0]).all()
    assert ops.work_word("cuda").item() == 0


def test_null_outputs_null_turn_and_bad_arguments():
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    b, t = perft_cases.inputs("small")
    n = len(t)
    bt, tt = dev(b, t)
    w = ops.work_word("cuda")
    size = lib.othc_perft_scratch_bytes(n, 64 * n)
    scratch = torch.empty(size // 8, dtype=torch.int64, device="cuda")
    leaves = torch.full((n,), 77, dtype=torch.int64, device="cuda")
    rows = torch.full((n, 64), 77, dtype=torch.int64, device="cuda")
    sp, sb = scratch.data_ptr(), size
    # every output NULL; the rows alone (a level is made for them at split 0); turn NULL: Black everywhere
    assert lib.othc_perft(bt.data_ptr(), tt.data_ptr(), 3, None, 0, 0, None, None, None, None, sp, sb, w.data_ptr(), n,
                          stream) == 0
    assert lib.othc_perft(bt.data_ptr(), tt.data_ptr(), 3, None, 0, 0, None, rows.data_ptr(), None, None, sp, sb,
                          w.data_ptr(), n, stream) == 0
    assert lib.othc_perft(bt.data_ptr(), None, 3, None, 2, 0, leaves.data_ptr(), None, None, None, sp, sb,
                          w.data_ptr(), n, stream) == 0
    torch.cuda.synchronize()
    want = perft_cases.reference("small", 3)
    assert (rows.cpu().numpy() == want[1]).all() and w.item() == 0
    black = perft_ref.perft(b, np.ones(n, np.uint8), 3)
    assert (leaves.cpu().numpy() == black[0]).all()
    e = ops.perft(bt[:0], tt[:0], 4, want_divide=True, want_nodes=True)
    assert e.leaves.numel() == 0 and e.divide.shape == (0, 64) and e.nodes.numel() == 0
    # bad arguments: OTH_EINVAL, nothing launched
    good = [bt.data_ptr(), tt.data_ptr(), 3, None, 0, 0, leaves.data_ptr(), rows.data_ptr(), None, None, sp, sb,
            w.data_ptr(), n, stream]
    small = lib.othc_perft_scratch_bytes(n, 64)  # room for the positions, not for the rows
    for k, v in ((2, -1), (2, 15), (4, -1), (4, 9), (10, None), (10, sp + 8), (11, small), (11, 64), (12, None),
                 (13, -1), (0, None)):
        a = list(good)
        a[k] = v
        assert lib.othc_perft(*a) == _lib.OTH_EINVAL, (k, v)
    a = list(good)
    a[7], a[11] = None, small  # without the rows the small lists do
    assert lib.othc_perft(*a) == 0
    torch.cuda.synchronize()
    assert (leaves.cpu().numpy() == want[0]).all()
    with pytest.raises(ValueError, match="depth must lie"):
        ops.perft(bt, tt, 15)
    with pytest.raises(ValueError, match="split must lie"):
        ops.perft(bt, tt, 3, split=9)
    with pytest.raises(ValueError, match="max_tasks must lie"):
        ops.perft(bt, tt, 3, max_tasks=(1 << 24) + 1)
    with pytest.raises(ValueError, match="32 bits"):
        ops.perft(bt, tt, 3, node_limit=1 << 32)
    r = ops.perft(bt, tt, 3)
    torch.cuda.synchronize()
    assert (r.leaves.cpu().numpy() == want[0]).all() and ops.work_word("cuda").item() == 0


def test_vecenv_perft():
    env = VecEnv(8)
    r = env.perft(5, want_divide=True)
    assert (r.leaves == 1396).all() and (r.divide[:, OPENING_MOVES] == 349).all() and (r.divide.sum(dim=1) == 1396).all()
    assert (r.status == _lib.PERFT_COUNTED).all()


def test_the_engines_perft_command_in_a_child_process():
    p = subprocess.run([sys.executable, "-m", "subproc_amd.engine"], input="perft 5\nd3\nperft 2\nquit\n",
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert out[:5] == ["D3 349", "C4 349", "F5 349", "E6 349", "1396"]  # a1..h8 order; 4 x 349 = 1,396
    # after d3 (White to move: three moves, 14 replies in all, perft 3 = 56 = 4 x 14)
    rest = out[8:]
    assert rest[-2] == "14" and rest[-1] == "bye" and sum(int(ln.split()[1]) for ln in rest[:-2]) == 14
    assert len(rest) == 5
