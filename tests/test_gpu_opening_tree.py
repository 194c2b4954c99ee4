"""The random rollout's opening walk (subproc_amd/csrc/opening_tree.hpp,
DESIGN.md §3.2): the first plies of a game from the standard opening are looked
up in the device's opening tree by the game's own draws, so nothing a game
computes may change.  Bit-exact on final boards, diff, plies and the 133-bin
histogram: against the same library computing every ply (a caller-supplied
start bypasses the tree; OTH_OPENING_DEPTH=0 turns it off) and against the
OpenMP oracle.

The depth is read per launch from the environment, but the tree is built once
per process, and "first use" is part of what is checked, so the cases that
depend on either run in a fresh child process each (CHILD below)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

from subproc_amd import ops  # noqa: E402
from subproc_amd._lib import BLACK  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
U = ops.to_numpy_u64
OPEN_BLACK, OPEN_WHITE = 0x0000000810000000, 0x0000001008000000
N = 4129  # 64 full batches and one ragged batch of 33
WRAP_ID0 = 2**64 - 2000  # game ids wrap 2^64 inside the launch
CASES = [(0x5EED, 0), (77, 123456789), (5, WRAP_ID0)]  # (seed, game_id0)
FIELDS = ("final_boards", "diff", "plies", "hist")


def as_numpy(r):
    return dict(final_boards=U(r.final_boards), diff=r.diff.cpu().numpy(), plies=r.plies.cpu().numpy(),
                hist=r.hist.cpu().numpy())


def same(a, b, what):
    for f in FIELDS:
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), (what, f)


@pytest.fixture(scope="module")
def oracle_cases():
    """The oracle's games of CASES, computed once and left unchanged."""
    out = []
    for seed, g0 in CASES:
        o = oracle.rollout(N, seed, g0)
        out.append({f: o[f] for f in FIELDS})
    return out


# one child process: argv = mode, output .npz; the environment carries the knobs
CHILD = r"""
import sys, threading
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from subproc_amd import ops

mode, out = sys.argv[2], sys.argv[3]
N = int(sys.argv[4])
CASES = [(int(s), int(g)) for s, g in (c.split(":") for c in sys.argv[5:])]
DEV = "cuda"
res = {}
def put(tag, r):
    res[tag + "final_boards"] = ops.to_numpy_u64(r.final_boards)
    res[tag + "diff"] = r.diff.cpu().numpy()
    res[tag + "plies"] = r.plies.cpu().numpy()
    res[tag + "hist"] = r.hist.cpu().numpy()
if mode == "depth":
    for k, (seed, g0) in enumerate(CASES):
        put("c%d_" % k, ops.rollout(N, seed, g0, device=DEV))
elif mode == "capture":
    # the first rollout of the process is captured: the tree is not built yet
    seed, g0 = CASES[0]
    w = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist = torch.zeros(133, dtype=torch.int64, device=DEV)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        r = ops.rollout(N, seed, g0, hist=hist, device=DEV, work=w)
    for k in range(2):
        hist.zero_()
        g.replay()
        torch.cuda.synchronize()
        put("replay%d_" % k, r)
    put("eager_", ops.rollout(N, seed, g0, device=DEV))  # builds the tree
    hist.zero_()
    g.replay()  # the captured launch still computes every ply
    torch.cuda.synchronize()
    put("replay2_", r)
    res["work"] = w.cpu().numpy()
elif mode == "threads":
    # two threads make the process's first rollouts at once
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    gate = threading.Barrier(2)
    got = [None, None]
    def run(k):
        seed, g0 = CASES[k]
        st = torch.cuda.Stream(DEV)
        with torch.cuda.stream(st):
            w = torch.zeros(1, dtype=torch.int64, device=DEV)
            st.synchronize()
            gate.wait()
            got[k] = ops.rollout(N, seed, g0, device=DEV, work=w)
            st.synchronize()
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    for k in range(2):
        put("c%d_" % k, got[k])
np.savez(out, **res)
"""


def run_child(mode, tmp_path, cases, env=None, n=N):
    out = str(tmp_path / f"{mode}.npz")
    e = dict(os.environ)
    e.pop("OTH_OPENING_DEPTH", None)
    e.update(env or {})
    subprocess.run([sys.executable, "-c", CHILD, ROOT, mode, out, str(n)] + [f"{s}:{g}" for s, g in cases],
                   check=True, env=e, cwd=ROOT, timeout=300)
    z = np.load(out)
    return lambda tag: {f: z[tag + f] for f in FIELDS}, z


@pytest.mark.parametrize("case", range(len(CASES)))
def test_tree_walk_equals_computed_plies(case, oracle_cases):
    """start=None walks the tree; the opening passed as `start` bypasses it and
    computes every ply.  Same seed and ids: the same games."""
    seed, g0 = CASES[case]
    start = ops.from_numpy_u64(np.tile(np.array([[OPEN_BLACK, OPEN_WHITE]], np.uint64), (N, 1)), DEV)
    turn = torch.full((N,), BLACK, dtype=torch.uint8, device=DEV)
    walked = as_numpy(ops.rollout(N, seed, g0, device=DEV))
    computed = as_numpy(ops.rollout(N, seed, g0, start=start, start_turn=turn, device=DEV))
    same(walked, computed, "walk vs computed")
    same(walked, oracle_cases[case], "walk vs oracle")
    assert int(walked["hist"][132]) == int(walked["plies"].astype(np.int64).sum())


@pytest.fixture(scope="module")
def depth0(tmp_path_factory):
    get, _ = run_child("depth", tmp_path_factory.mktemp("depth0"), CASES, {"OTH_OPENING_DEPTH": "0"})
    return [get(f"c{k}_") for k in range(len(CASES))]


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 5, 6, 7, 8, 99])
def test_every_depth_plays_the_same_games(depth, depth0, oracle_cases, tmp_path):
    """OTH_OPENING_DEPTH in a process of its own (99 is clamped to 8): the games
    of depth 0, which are the oracle's.  Up to 4 (the default, which the other
    tests run) the whole walk is in LDS; 5 and 6 read the leaf from memory; 7
    and 8 read the lower levels' nodes from memory too."""
    get, _ = run_child("depth", tmp_path, CASES, {"OTH_OPENING_DEPTH": str(depth)})
    for k in range(len(CASES)):
        r = get(f"c{k}_")
        same(r, depth0[k], (depth, k, "vs depth 0"))
        same(r, oracle_cases[k], (depth, k, "vs oracle"))
        assert int(r["hist"][132]) == int(r["plies"].astype(np.int64).sum())


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_edge_sizes_vs_oracle(n):
    r = as_numpy(ops.rollout(n, 31, 7, device=DEV))
    o = oracle.rollout(n, 31, 7)
    same(r, {f: o[f] for f in FIELDS}, n)


def test_handoff_does_not_walk_again(monkeypatch):
    """Parked games come back from the pool with their state: a game that walked
    a second time would change its plies.  K = 0 parks nothing."""
    n = 16384
    with_k = as_numpy(ops.rollout(n, 9, 50, device=DEV))
    monkeypatch.setenv("OTH_HANDOFF_K", "0")
    without = as_numpy(ops.rollout(n, 9, 50, device=DEV))
    same(with_k, without, "default K vs K=0")
    assert int(with_k["hist"][132]) == int(with_k["plies"].astype(np.int64).sum())


def test_first_use_under_capture(oracle_cases, tmp_path):
    """The process's first rollout is captured: the tree is not built during
    the capture (that launch computes every ply), the eager launch after the
    replays builds it, and everything equals the oracle."""
    get, z = run_child("capture", tmp_path, CASES[:1])
    for tag in ("replay0_", "replay1_", "eager_", "replay2_"):
        same(get(tag), oracle_cases[0], tag)
    assert int(z["work"][0]) == 0


def test_concurrent_first_use(oracle_cases, tmp_path):
    """Two threads make their first rollout at once, on two streams with two
    work words: one of them builds the tree, both play the oracle's games."""
    get, _ = run_child("threads", tmp_path, CASES[:2])
    for k in range(2):
        same(get(f"c{k}_"), oracle_cases[k], k)
