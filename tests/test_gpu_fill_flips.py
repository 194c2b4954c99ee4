"""The rollout kernels' flips come from the Kogge-Stone fills (bitboard.hpp
run_prefix): they may carry discs of the mover's own beyond a run's far end,
which place() must leave where they are.  Games from mid-game positions whose
a/h files and rows 1/8 are full, in alternating colours (every diagonal ray
ends on an occupied edge square, the +-7 / +-9 fills meet the file wrap, and
own discs beyond the stop square are everywhere), game by game against the C
oracle: random policy, greedy by the wave's cooperative choice and by the
per-lane one (OTH_COOP_CAP=0), and the legal masks."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

from subproc_amd import ops  # noqa: E402

DEV = "cuda"
U = ops.to_numpy_u64
EDGE = np.uint64(0xFF818181818181FF)
RING = [x for x in range(8)] + [7 + 8 * y for y in range(1, 8)] + [x + 56 for x in range(6, -1, -1)] + \
       [8 * y for y in range(6, 0, -1)]
ALT = [np.uint64(sum(1 << s for k, s in enumerate(RING) if k % 2 == ph)) for ph in (0, 1)]


def edge_starts(n, seed):
    """oracle.sample_midgame positions with the edge ring filled, colours
    alternating round it (the phase alternates from game to game)"""
    s = oracle.sample_midgame(n, seed)
    b = s["boards"].copy()
    black_edge = np.where(np.arange(n) % 2 == 0, ALT[0], ALT[1])
    b[:, 0] = (b[:, 0] & ~EDGE) | black_edge
    b[:, 1] = (b[:, 1] & ~EDGE) | (EDGE & ~black_edge)
    assert not (b[:, 0] & b[:, 1]).any()
    return b, s["turn"].copy()


def dev_boards(b):
    return ops.from_numpy_u64(b, DEV)


def dev_u8(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.uint8).to(DEV)


@pytest.fixture(scope="module")
def starts():
    return edge_starts(4096, 0xF111)


@pytest.fixture(scope="module")
def greedy_ref(starts):
    b, t = starts
    return oracle.rollout(len(b), 11, 0, 1, 2, start=b, start_turn=t)


def _same_games(r, o, what):
    assert (U(r.final_boards) == o["final_boards"]).all(), what
    assert (r.diff.cpu().numpy() == o["diff"]).all(), what
    assert (r.plies.cpu().numpy() == o["plies"]).all(), what


def test_random_games_from_edge_starts(starts):
    b, t = starts
    assert np.bitwise_count(oracle.legal(b, t)).sum() > 4 * len(b)  # the starts have moves to play
    r = ops.rollout(len(b), 11, 0, "random", start=dev_boards(b), start_turn=dev_u8(t), device=DEV)
    o = oracle.rollout(len(b), 11, 0, 0, start=b, start_turn=t)
    assert o["plies"].astype(int).sum() > 8 * len(b)
    _same_games(r, o, "random")


@pytest.mark.parametrize("cap", [None, "0"])
def test_greedy_games_from_edge_starts(cap, starts, greedy_ref, monkeypatch):
    if cap is None:
        monkeypatch.delenv("OTH_COOP_CAP", raising=False)
    else:
        monkeypatch.setenv("OTH_COOP_CAP", cap)
    b, t = starts
    r = ops.rollout(len(b), 11, 0, "greedy", 2, start=dev_boards(b), start_turn=dev_u8(t), device=DEV)
    _same_games(r, greedy_ref, f"greedy, OTH_COOP_CAP={cap}")


def test_legal_on_edge_positions():
    b, t = edge_starts(65536, 0xF112)
    assert (U(ops.legal(dev_boards(b), dev_u8(t))) == oracle.legal(b, t)).all()
