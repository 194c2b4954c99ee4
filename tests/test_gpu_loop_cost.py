"""The random rollout's two-ply loop after its issue-cost cuts (DESIGN.md §3.1,
§3.2, profiles/loop_cost_notes.md): the pass flag kept as a disc count, the
pass count corrected after the loop, the k-th-bit search without its variable
shift.  Nothing a game computes may change: final boards, diff, plies and the
133-bin histogram equal the OpenMP oracle's, game for game, at the batch-edge
sizes, with the batch-tail hand-over on and off (parked games carry the pass
flag through the pool), with and without the opening walk, and from starts
where the first thing a game does is pass or end."""
import numpy as np
import pytest
import torch

import oracle
import synthetic_cases as sc

pytestmark = pytest.mark.gpu

from subproc_amd import ops  # noqa: E402

DEV = "cuda"
U = ops.to_numpy_u64
SEED, ID0 = 0x10C0, 977
SIZES = (1, 63, 64, 65, 4096)
FIELDS = ("final_boards", "diff", "plies", "hist")
N_START = 4096


def as_numpy(r):
    return dict(final_boards=U(r.final_boards), diff=r.diff.cpu().numpy(), plies=r.plies.cpu().numpy(),
                hist=r.hist.cpu().numpy())


def same(a, b, what):
    for f in FIELDS:
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), (what, f)


@pytest.fixture(scope="module")
def from_opening():
    """The oracle's games from the standard opening, once per size, read-only."""
    out = {}
    for n in SIZES:
        o = oracle.rollout(n, SEED, ID0)
        out[n] = {f: o[f] for f in FIELDS}
        for a in out[n].values():
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("depth", [0, 4])
@pytest.mark.parametrize("handoff_k", [0, 16])
@pytest.mark.parametrize("n", SIZES)
def test_games_equal_the_oracle(n, handoff_k, depth, from_opening, monkeypatch):
    monkeypatch.setenv("OTH_HANDOFF_K", str(handoff_k))
    monkeypatch.setenv("OTH_OPENING_DEPTH", str(depth))
    r = as_numpy(ops.rollout(n, SEED, ID0, device=DEV))
    same(r, from_opening[n], (n, handoff_k, depth))
    assert int(r["hist"][132]) == int(r["plies"].astype(np.int64).sum())


@pytest.fixture(scope="module")
def starts():
    """4,096 caller positions: the fixed edge list (full boards, wipe-outs, nobody
    ever moves, a pass and then the last move) and the seeded families near the
    end of the game, where passes and early ends are common; tiled."""
    parts = [sc.edges()[:2], sc.lopsided(8), sc.lopsided(12), sc.islands(6), sc.uniform(20), sc.uniform(40)]
    boards = np.concatenate([p[0] for p in parts])
    turn = np.concatenate([p[1] for p in parts])
    reps = -(-N_START // len(turn))
    boards, turn = np.tile(boards, (reps, 1))[:N_START], np.tile(turn, reps)[:N_START]
    o = oracle.rollout(N_START, SEED, ID0, start=boards, start_turn=turn)
    ref = {f: o[f] for f in FIELDS}
    for a in (boards, turn, *ref.values()):
        a.setflags(write=False)
    return boards, turn, ref


def test_starts_hold_the_cases(starts):
    """A mover who must pass, a full board, both sides without a move."""
    boards, turn, _ = starts
    must_pass, over = sc.root_kinds(boards, turn)
    full = sc.popcount(boards[:, 0] | boards[:, 1]) == 64
    assert must_pass.sum() >= 32 and full.sum() >= 32 and (over & ~full).sum() >= 32


@pytest.mark.parametrize("handoff_k", [0, 16])
def test_games_from_starts_equal_the_oracle(handoff_k, starts, monkeypatch):
    boards, turn, ref = starts
    monkeypatch.setenv("OTH_HANDOFF_K", str(handoff_k))
    r = as_numpy(ops.rollout(N_START, SEED, ID0, start=ops.from_numpy_u64(boards, DEV),
                             start_turn=torch.from_numpy(turn.copy()).to(DEV), device=DEV))
    same(r, ref, ("starts", handoff_k))
    assert int(r["hist"][132]) == int(r["plies"].astype(np.int64).sum())
