"""Perft on the host (tools/diag/perft_host.cpp: perft_core.hpp's machine in plain
C++ inside a plain restatement of perft.hip's level expansion, void levels
included) against tests/perft_ref.py's level-by-level checker over the oracle
and against the published opening values.  DESIGN.md §27.

Splits 0, 1, 3 and 5 and lists of 64, 4,096 and 2**18 tasks, with and without
the rows, so that void levels occur and deep levels too: leaves, divide and
status must not depend on any of it.  The same under
-fsanitize=address,undefined, as a process of its own.  CPU only."""
import numpy as np
import pytest

import host_programs as hp
import perft_cases
import perft_ref
import synthetic_cases

SPLITS = (0, 1, 3, 5)
CAPS = (64, 4096, 1 << 18)  # (the last so that the deep levels are made, not only declared void)


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "perft_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "perft_host", hp.SANITIZED)


def run(exe, tmp, boards, turn, depth, split, max_tasks, divide=1, limit=0, depths=None):
    inp, out = str(tmp / "pin"), str(tmp / "pout")
    hp.write_positions(inp, boards, turn, depths)
    hp.run([exe, inp, out, -1 if depths is not None else depth, split, max_tasks, divide, limit, 8])
    a, meta = hp.read_rows(out, (len(turn), 67), trailer=True)
    return dict(leaves=a[:, 0], status=a[:, 1], nodes=a[:, 2], divide=a[:, 3:], levels=int(meta[1]),
                void=int(meta[3]), tasks=int(meta[5]))


def test_the_checker_reproduces_the_published_opening_values_to_depth_8():
    b, t = perft_ref.opening()
    for d in range(0, 9):
        leaves, divide, status = perft_ref.perft(b, t, d)
        assert int(leaves[0]) == (1 if d == 0 else perft_ref.OPENING[d - 1]) and status[0] == perft_ref.COUNTED, d
        assert int(divide[0].sum()) == (0 if d == 0 else int(leaves[0])), d
        if d:
            assert sorted(np.nonzero(divide[0])[0].tolist()) == [19, 26, 37, 44] and len(set(divide[0][[19, 26, 37, 44]])) == 1


def test_the_host_build_gives_the_published_opening_values_to_depth_10(binary, tmp_path):
    b, t = perft_ref.opening()
    for d in range(1, 11):
        for split, cap in ((0, 64), (5, 64), (3, 4096)) if d >= 8 else ((0, 64), (1, 64), (3, 64), (5, 4096)):
            got = run(binary, tmp_path, b, t, d, split, cap, divide=int(split > 0))
            assert int(got["leaves"][0]) == perft_ref.OPENING[d - 1], (d, split, cap)
            assert got["status"][0] == perft_ref.COUNTED
            if split:
                assert int(got["divide"][0].sum()) == perft_ref.OPENING[d - 1]
                assert (got["divide"][0][[19, 26, 37, 44]] * 4 == perft_ref.OPENING[d - 1]).all()
    # the two rules the depths 9 and 10 are there for
    assert perft_ref.OPENING[8] != 3005320 and perft_ref.OPENING[9] != 24571056


@pytest.mark.parametrize("name", ["small", "endgames", "offtree"])
def test_the_host_build_equals_the_checker_whatever_the_split_and_the_room(binary, tmp_path, name):
    b, t = perft_cases.inputs(name)
    voids, made = set(), set()
    for depth in perft_cases.DEPTHS[name]:
        want = perft_cases.reference(name, depth)
        for split in SPLITS:
            for cap in CAPS:
                # with the rows: at least one level, lists of at least 64 tasks per position
                got = run(binary, tmp_path, b, t, depth, split, cap)
                perft_cases.same(got, want, (name, depth, split, cap))
                voids.add(got["void"])
                made.add(got["levels"])
                # without: no level is forced and the lists are as small as asked (never below a task per position)
                got = run(binary, tmp_path, b, t, depth, split, cap, divide=0)
                assert (got["leaves"] == want[0]).all() and (got["status"] == want[2]).all(), (name, depth, split, cap)
                assert not got["divide"].any() and got["levels"] <= split
                voids.add(got["void"])
                made.add(got["levels"])
                if split == 0:
                    assert got["levels"] == 0 and got["tasks"] == int((want[2] == perft_ref.COUNTED).sum())
    assert len(voids - {0}) >= 1 and 0 in voids, voids  # void levels occurred, and runs without
    assert {0, 1, 3, 5} <= made or name != "small", made
    if name == "small":
        assert want[2][-1] == perft_ref.INVALID and want[0][-1] == 0 and not want[1][-1].any()


def test_per_position_depths_in_one_run_and_the_limit(binary, tmp_path):
    b, t, d, want = perft_cases.mixed()
    for split, cap in ((0, 64), (3, 4096), (5, 64)):
        perft_cases.same(run(binary, tmp_path, b, t, 0, split, cap, depths=d), want, ("mixed", split, cap))
    over = np.array(d, np.int64)
    over[:3] = 15  # beyond OTHC_MAX_DEPTH
    got = run(binary, tmp_path, b, t, 0, 1, 64, depths=over)
    assert (got["status"][:3] == perft_ref.BADDEPTH).all() and not got["leaves"][:3].any()
    assert (got["leaves"][3:] == want[0][3:]).all()
    # a task that runs into node_limit ends its position as LIMIT with counts of 0
    ob, ot = perft_ref.opening()
    got = run(binary, tmp_path, ob, ot, 6, 0, 64, divide=0, limit=16)
    assert got["status"][0] == perft_ref.LIMIT and got["leaves"][0] == 0 and got["nodes"][0] == 16
    got = run(binary, tmp_path, ob, ot, 6, 1, 64, limit=16)
    assert got["status"][0] == perft_ref.LIMIT and got["leaves"][0] == 0 and not got["divide"].any()
    got = run(binary, tmp_path, ob, ot, 6, 0, 64, divide=0, limit=1 + 4 + 12 + 56 + 244 + 1396)
    assert got["status"][0] == perft_ref.COUNTED and got["leaves"][0] == 8200  # exactly the limit is counted


def test_the_sixteen_images_of_a_root_count_the_same(binary, tmp_path):
    b, t = perft_cases.inputs("small")
    pick = np.r_[0:6, 64:70]  # midgame roots and forced-pass / game-over roots
    ib, it, perm = synthetic_cases.images(b[pick], t[pick])
    got = run(binary, tmp_path, ib, it, 4, 3, 4096)
    want = perft_cases.reference("small", 4)
    for k, i in enumerate(pick):
        for j in range(16 * k, 16 * k + 16):
            assert got["leaves"][j] == want[0][i], (i, j)
            moved = np.zeros(64, np.int64)
            moved[perm[j]] = want[1][i]
            assert (got["divide"][j] == moved).all(), (i, j)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    for name, depth in (("small", 4), ("endgames", 8), ("offtree", 3)):
        b, t = perft_cases.inputs(name)
        want = perft_cases.reference(name, depth)
        for split, cap in ((0, 64), (3, 4096), (5, 64)):
            perft_cases.same(run(binary_asan, tmp_path, b, t, depth, split, cap), want, ("asan", name, split, cap))
    b, t, d, want = perft_cases.mixed()
    perft_cases.same(run(binary_asan, tmp_path, b, t, 0, 5, 4096, depths=d), want, "asan mixed")
    ob, ot = perft_ref.opening()
    for split in (0, 5):
        got = run(binary_asan, tmp_path, ob, ot, 8, split, 64, divide=int(split > 0))
        assert int(got["leaves"][0]) == perft_ref.OPENING[7]
    got = run(binary_asan, tmp_path, ob, ot, 14, 0, 64, divide=0, limit=4096)  # the deepest stack, cut by the limit
    assert got["status"][0] == perft_ref.LIMIT
