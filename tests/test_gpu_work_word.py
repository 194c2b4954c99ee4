"""The work-word launch protocol of ops.py (one statement, fourteen entry points):
a call the library refuses drops the stream's cached word or zeroes the
caller's, the next good call is the one a fresh stream makes, and a capture
without a word is refused before anything is launched.

Every refusal here is OTH_EINVAL from the library's argument checks, which
answer before any launch."""
import numpy as np
import pytest
import torch

import solve_cases
from subproc_amd import _lib, ops

pytestmark = pytest.mark.gpu

N, SEED = 4, 7


def inputs():
    """(endgame boards, turn, midgame boards, turn) on the device: 4 roots at 5 empties, 4 at 30."""
    out = []
    for e in (5, 30):
        b, t = solve_cases.ladder(e, N)
        out += [ops.from_numpy_u64(np.ascontiguousarray(b, np.uint64), "cuda"), torch.from_numpy(t.copy()).cuda()]
    torch.cuda.synchronize()
    return out


# name -> (the good call, the call the library refuses), each f(sb, st, mb, mt, work)
ENTRY = {
    "rollout": (lambda sb, st, mb, mt, w: ops.rollout(N, SEED, record_moves=True, work=w),
                lambda sb, st, mb, mt, w: ops.rollout(-1, SEED, want_boards=False, want_diff=False, want_plies=False,
                                                      work=w)),
    "rollout_runner": (lambda sb, st, mb, mt, w: ops.rollout_runner(N, SEED, policy="greedy", n_rand_a=2, work=w),
                       lambda sb, st, mb, mt, w: ops.rollout_runner(N, SEED, policy="greedy", n_rand_a=-1, work=w)),
    "solve": (lambda sb, st, mb, mt, w: ops.solve(sb, st, max_empties=6, want_nodes=True, work=w),
              lambda sb, st, mb, mt, w: ops.solve(sb, st, max_empties=13, work=w)),
    "solve_split": (lambda sb, st, mb, mt, w: ops.solve(sb, st, max_empties=6, task_empties=3, work=w),
                    lambda sb, st, mb, mt, w: ops.solve(sb, st, max_empties=6, task_empties=13, work=w)),
    "search": (lambda sb, st, mb, mt, w: ops.search(mb, mt, 2, want_nodes=True, work=w),
               lambda sb, st, mb, mt, w: ops.search(mb, mt, 0, work=w)),
    "search_split": (lambda sb, st, mb, mt, w: ops.search(mb, mt, 2, split=1, work=w),
                     lambda sb, st, mb, mt, w: ops.search(mb, mt, 1, split=1, work=w)),
    "search_budget": (lambda sb, st, mb, mt, w: ops.search_budget(mb, mt, 64, max_depth=2, want_nodes=True, work=w),
                      lambda sb, st, mb, mt, w: ops.search_budget(mb, mt, 64, max_depth=9, work=w)),
    "search_moves": (lambda sb, st, mb, mt, w: ops.search_moves(mb, mt, 2, want_nodes=True, work=w),
                     lambda sb, st, mb, mt, w: ops.search_moves(mb, mt, 0, work=w)),
    "play": (lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=1, depth_b=2, want_nodes=True, work=w),
             lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=0, work=w)),
    "play_ordered": (lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=1, depth_b=2, order=1, want_nodes=True, work=w),
                     lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=0, order=1, work=w)),
    "play_budget": (lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=2, budget=(16, 64), want_nodes=True, work=w),
                    lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=0, budget=64, work=w)),
    "play_solve": (lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=1, depth_b=2, solve_empties=6,
                                                      record_moves=True, want_nodes=True, work=w),
                   lambda sb, st, mb, mt, w: ops.play(N, SEED, depth_a=0, solve_empties=6, work=w)),
    "solve_line": (lambda sb, st, mb, mt, w: ops.solve_line(sb, st, max_empties=6, want_nodes=True, work=w),
                   lambda sb, st, mb, mt, w: ops.solve_line(sb, st, max_empties=13, work=w)),
    "search_line": (lambda sb, st, mb, mt, w: ops.search_line(mb, mt, 2, want_nodes=True, work=w),
                    lambda sb, st, mb, mt, w: ops.search_line(mb, mt, 2, order=9, work=w)),
}


def same(a, b):
    assert type(a) is type(b)
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), name
        assert x is None or torch.equal(x, y), name


def on_fresh_stream(fn):
    """fn() on a stream nothing has run on; the stream is synchronised on the way out."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = fn()
    s.synchronize()
    return out


@pytest.mark.parametrize("entry", list(ENTRY))
def test_a_refused_call_drops_the_streams_word_and_the_next_call_is_a_fresh_streams(entry):
    good, bad = ENTRY[entry]
    args = inputs()
    want = on_fresh_stream(lambda: good(*args, None))

    def refused_then_good():
        first = good(*args, None)  # the stream has its cached word now
        word = ops.work_word()
        with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
            bad(*args, None)
        assert ops.work_word() is not word  # dropped: a fresh zeroed one
        second = good(*args, None)
        return first, second, ops.work_word()

    first, second, word = on_fresh_stream(refused_then_good)
    same(first, want)
    same(second, want)
    assert word.item() == 0


@pytest.mark.parametrize("entry", list(ENTRY))
def test_a_refused_call_leaves_the_callers_word_at_zero(entry):
    good, bad = ENTRY[entry]
    args = inputs()
    want = good(*args, None)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    # the refusal comes before any launch, so nothing on the device reads the
    # word: a stale count in it shows that ops itself resets it
    w.fill_(5)
    with pytest.raises(_lib.OthelloCallError, match="OTH_EINVAL"):
        bad(*args, w)
    assert w.item() == 0
    same(good(*args, w), want)
    assert w.item() == 0


@pytest.mark.parametrize("entry", list(ENTRY))
def test_a_capture_without_a_word_is_refused_before_any_launch(entry):
    good, bad = ENTRY[entry]
    sb, st, mb, mt = inputs()
    want = ops.search(mb, mt, 1)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="explicit work word"):
            good(sb, st, mb, mt, None)
        with pytest.raises(RuntimeError, match="explicit work word"):
            bad(sb, st, mb, mt, None)
        r = ops.search(mb, mt, 1, work=w)  # the one launch the graph holds
    g.replay()
    torch.cuda.synchronize()
    same(r, want)
    assert w.item() == 0
