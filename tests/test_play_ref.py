"""The self-play checker (tests/play_ref.py) is right: with a 1-ply chooser it
plays the C oracle's GameRunner games draw for draw, and the turns that need no
chooser are right on cases worked out by hand (CPU only)."""
import numpy as np

import oracle
import play_ref
import search_ref
from subproc_amd import params

DEFAULT = np.asarray(params.DEFAULT_WEIGHTS, np.int8)
FULL = (1 << 64) - 1


def no_chooser(boards, turn, player):
    raise AssertionError("no turn of this game asks the chooser")


def test_one_ply_chooser_reproduces_the_oracles_runner_games():
    """The schedule and the draws are the oracle's: colour draw, budgets 3 and
    12 (capped at 10), coins on passes, random moves."""
    o = oracle.rollout_runner(48, 77, game_id0=5, policy=2, weights_a=DEFAULT, weights_b=search_ref.WEIGHTS_B,
                              n_rand_a=3, n_rand_b=12, swap=True, record_moves=True)
    r = play_ref.play(48, 77, play_ref.one_ply_chooser(DEFAULT, search_ref.WEIGHTS_B), game_id0=5, n_rand_a=3,
                      n_rand_b=12, swap=True)
    assert (r["a_black"] == o["a_black"]).all() and 0 < int(o["a_black"].sum()) < 48
    assert (r["final_boards"] == o["final_boards"]).all()
    assert (r["plies"] == o["plies"]).all() and (r["diff"] == o["diff"]).all()
    assert (r["moves"] == o["moves"]).all()
    assert (r["hist"] == o["hist"]).all() and (r["status"] == play_ref.SEARCHED).all()
    assert (o["moves"] == play_ref.PASS).any()  # a pass was played (and its coin drawn) somewhere


def test_one_ply_chooser_from_midgame_starts_without_swap():
    pos = oracle.sample_midgame(32, 0x5EED)
    o = oracle.rollout_runner(32, 9, policy=2, weights_a=search_ref.WEIGHTS_B, weights_b=DEFAULT, n_rand_a=0,
                              n_rand_b=2, swap=False, start=pos["boards"], start_turn=pos["turn"], record_moves=True)
    r = play_ref.play(32, 9, play_ref.one_ply_chooser(search_ref.WEIGHTS_B, DEFAULT), n_rand_b=2,
                      start=pos["boards"], start_turn=pos["turn"])
    for k in ("a_black", "final_boards", "plies", "diff", "moves", "hist"):
        assert (r[k] == o[k]).all(), k


def test_a_start_that_is_over_plays_nothing():
    black = 0x00000000FFFFFFFF | (1 << 40)  # a full board: 33 black, 31 white
    r = play_ref.play(2, 1, no_chooser, n_rand_a=5, n_rand_b=5, swap=True,
                      start=np.array([[black, FULL ^ black]] * 2, np.uint64), start_turn=np.array([1, 2], np.uint8))
    assert r["plies"].tolist() == [0, 0] and r["diff"].tolist() == [2, 2]
    assert (r["moves"] == 255).all() and r["status"].tolist() == [1, 1]
    assert r["hist"][66] == 2 and r["hist"][129] == 2 and r["hist"][132] == 0


def test_a_mover_that_must_pass_and_a_single_move():
    """a1 empty, b1 white, the rest black, White to move: White passes (ply 0),
    Black's only move a1 (ply 1) takes the last white disc: 64 - 0 in 2 plies.
    No turn asks the chooser, with or without budgets."""
    white = 1 << 1
    black = FULL ^ white ^ 1
    for budgets in ((0, 0), (4, 7)):
        r = play_ref.play(1, 3, no_chooser, n_rand_a=budgets[0], n_rand_b=budgets[1],
                          start=np.array([[black, white]], np.uint64), start_turn=np.array([2], np.uint8))
        assert r["moves"][0, :3].tolist() == [64, 0, 255]
        assert (r["plies"][0], r["diff"][0]) == (2, 64)
        assert r["final_boards"][0].tolist() == [FULL, 0]
    # the same position with Black to move: the single move at once
    r = play_ref.play(1, 3, no_chooser, start=np.array([[black, white]], np.uint64), start_turn=np.array([1], np.uint8))
    assert r["moves"][0, :2].tolist() == [0, 255] and r["plies"][0] == 1


def test_overlapping_start_is_invalid_and_not_in_the_histogram():
    b, t, _ = oracle.reset(1)
    start = np.array([b[0], [3, 1]], np.uint64)
    r = play_ref.play(2, 5, play_ref.one_ply_chooser(DEFAULT, DEFAULT), start=start)
    assert r["status"].tolist() == [play_ref.SEARCHED, play_ref.INVALID]
    assert (r["plies"][1], r["diff"][1], r["a_black"][1]) == (0, 0, 1)
    assert r["final_boards"][1].tolist() == [3, 1] and (r["moves"][1] == 255).all()
    assert r["hist"][129] + r["hist"][130] + r["hist"][131] == 1 and r["hist"][132] == r["plies"][0]


def test_search_chooser_at_depth_one_is_the_one_ply_chooser_away_from_the_end():
    """search_ref at depth 1 scores a child by the root mover's eval, unless the
    child ends the game (rule 1); on opening games' early plies no child does."""
    a = play_ref.play(8, 11, play_ref.search_chooser(DEFAULT, search_ref.WEIGHTS_B, 1, 1), n_rand_a=2, n_rand_b=2,
                      swap=True)
    b = play_ref.play(8, 11, play_ref.one_ply_chooser(DEFAULT, search_ref.WEIGHTS_B), n_rand_a=2, n_rand_b=2, swap=True)
    assert (a["moves"][:, :40] == b["moves"][:, :40]).all()
