"""The Monte Carlo search trees that persist, on the host
(tools/diag/mcts_tree_host.cpp: mcts_core.hpp's iterate(), advance() and
compact() in plain C++) against tests/mcts_tree_ref.py's checker: the rows and
the whole tree in canonical order after search(17), after an advance by the
best move and, separately, by the last legal move, and after search(23), on
tests/mcts_cases.py's `small` with M at its default and with M = 24 (trees that
are full before the re-root and have room after it); and the same under
-fsanitize=address,undefined, as a process of its own.  DESIGN.md §29.  CPU
only."""
import struct

import numpy as np
import pytest

import host_programs as hp
import mcts_cases
import mcts_ref
import mcts_tree_cases as cases
import mcts_tree_ref as ref

MS = (mcts_ref.default_nodes(40), 24)


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "mcts_tree_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "mcts_tree_host", hp.SANITIZED)


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def signed(x):
    return x - (1 << 64) if x >> 63 else x


def run(exe, tmp, boards, turn, ids, script, M, c=cases.C, seed=cases.SEED, table_last=256):
    """The program's answers, one entry per operation that prints: ("R", fields), ("A", status, moves) or
    ("T", nodes, played, canonical trees)."""
    inp, scr, out = str(tmp / "tin"), str(tmp / "tscript"), str(tmp / "tout")
    hp.write_positions(inp, boards, turn, ids)
    with open(inp, "a") as f:
        for x in cases.TABLE[:table_last + 1]:
            f.write("L %x\n" % bits(x))
    with open(scr, "w") as f:
        f.write("\n".join(script) + "\n")
    hp.run([exe, inp, scr, out, "%x" % bits(c), seed, M])
    lines = iter(open(out).read().splitlines())
    n, answers = len(turn), []
    for op in script:
        word = op.split()[0]
        if word in ("search", "rows"):
            a = []
            for _ in range(n):
                w = next(lines).split()
                assert w[0] == "R"
                a.append([int(x) for x in w[1:7]] + [signed(int(w[7], 16)), signed(int(w[8], 16))] +
                         [int(x) for x in w[9:]])
            a = np.array(a, np.int64)
            answers.append(("R", dict(status=a[:, 0], best_move=a[:, 1], nodes=a[:, 2], root_wins=a[:, 3],
                                      root_diffs=a[:, 4], ran=a[:, 5], root_boards=a[:, 6:8], root_turn=a[:, 8],
                                      visits=a[:, 9:73], wins=a[:, 73:137], diffs=a[:, 137:201])))
        elif word == "advance":
            a = np.array([[int(x) for x in next(lines).split()[1:]] for _ in range(n)], np.int64)
            answers.append(("A", a[:, 0].tolist(), a[:, 1].tolist()))
        elif word == "dump":
            counts, played, trees = [], [], []
            for _ in range(n):
                w = next(lines).split()
                assert w[0] == "T"
                counts.append(int(w[1])), played.append(int(w[2]))
                tree = []
                for _ in range(counts[-1]):
                    x = next(lines).split()
                    tree.append((int(x[0], 16), int(x[1], 16), int(x[2]), int(x[3]), int(x[4]), int(x[5])))
                trees.append(tree)
            answers.append(("T", counts, played, trees))
    assert next(lines, None) is None
    return answers


def same_trees(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, i, len(g), len(w))
        for j, (x, y) in enumerate(zip(g, w)):
            assert x == y, (what, i, j, x, y)


def check_session(exe, tmp, M, how, what):
    b, t = mcts_cases.inputs("small")
    want = cases.session(M, how)
    ids = [cases.id_base(i) for i in range(len(t))]
    script = ["init", "search %d" % cases.T1, "dump", "advance 1 %s" % how, "rows", "dump", "search %d" % cases.T2,
              "dump"]
    got = run(exe, tmp, b, t, ids, script, M)
    (r1, t1), (r2, t2), (r3, t3) = want["stages"]
    cases.same_rows(got[0][1], r1, (what, M, how, "search 17"))
    same_trees(got[1][3], t1, (what, M, how, "search 17"))
    assert got[2][1] == want["status"] and got[2][2] == want["moves"], (what, M, how)
    cases.same_rows(got[3][1], r2, (what, M, how, "advance"))
    same_trees(got[4][3], t2, (what, M, how, "advance"))
    assert got[4][1] == [len(x) for x in t2]
    cases.same_rows(got[5][1], r3, (what, M, how, "search 23"))
    same_trees(got[6][3], t3, (what, M, how, "search 23"))
    played = [cases.T1 + cases.T2 if x else 0 for x in got[6][1]]
    assert got[6][2] == played
    return want


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("how", ["best", "last"])
def test_the_host_build_equals_the_checker_on_the_rows_and_the_whole_tree(binary, tmp_path, M, how):
    check_session(binary, tmp_path, M, how, "host")


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    for M in MS:
        for how in ("best", "last"):
            check_session(binary_asan, tmp_path, M, how, "asan")


def test_the_sessions_hold_what_they_are_there_for():
    """The branches the sessions exist for occur in the checker's own answers."""
    big, tiny = MS
    for how in ("best", "last"):
        s = cases.session(big, how)
        (r1, t1), (r2, t2), (r3, t3) = s["stages"]
        assert s["status"][-1] == ref.INVALID and set(s["status"][:-1]) == {ref.READY}  # the overlap
        assert mcts_ref.PASS in s["moves"] and ref.KEEP in s["moves"][:-1]  # a root that must pass, a finished game
        kept = [len(x) for x in t2]
        assert max(kept) > 8 and 1 in kept  # subtrees of some depth, and single nodes
        assert any(len(b) > len(a) for a, b in zip(t2, t3))  # the tree grows again after the re-root
        assert all(r["root_turn"] == 3 - q["root_turn"] for r, q, st in zip(r2, r1, s["status"]) if st == ref.READY
                   and q["best_move"] != ref.KEEP)
    full = cases.session(tiny, "best")
    (r1, t1), (r2, t2), (r3, t3) = full["stages"]
    at_limit = [len(a) + 1 > tiny - 4 for a in t1]
    assert sum(at_limit) > 8  # trees with no room for another block of children before the re-root
    assert any(len(b) > len(a) and len(a) < len(c) for a, b, c in zip(t2, t3, t1))  # and room after it
    assert all(len(x) <= tiny for x in t3)


def test_a_refused_move_and_keep_zero(binary, tmp_path):
    """Moves the rule refuses leave the tree as it was; keep = 0 gives the child position alone."""
    b, t = mcts_cases.inputs("small")
    b, t = b[:4], t[:4]
    ids = [cases.id_base(i) for i in range(4)]
    occupied = [(int(x[0]) & -int(x[0])).bit_length() - 1 for x in b]  # a black disc's square
    script = ["init", "search 9", "dump", "advance 1 " + " ".join(map(str, occupied)), "advance 1 64", "advance 1 65",
              "advance 1 255", "dump", "advance 0 best", "dump", "rows"]
    got = run(binary, tmp_path, b, t, ids, script, 64)
    assert got[2][1] == [ref.BADMOVE] * 4 and got[3][1] == [ref.BADMOVE] * 4 and got[4][1] == [ref.BADMOVE] * 4
    assert got[5][1] == [ref.READY] * 4
    assert got[6] == got[1]
    trees = [ref.Tree(b[i], t[i], ids[i]) for i in range(4)]
    for tr, mv in zip(trees, got[7][2]):
        ref.search(tr, 9, cases.C, cases.SEED, 64, cases.TABLE)
        assert ref.rows(tr)["best_move"] == mv and ref.advance(tr, mv, False) == ref.READY
    assert got[8][1] == [1] * 4 and got[8][2] == [9] * 4
    same_trees(got[8][3], [ref.bfs(tr) for tr in trees], "keep 0")
    cases.same_rows(got[9][1], [ref.rows(tr) for tr in trees], "keep 0")
    # at a finished game every move is refused
    b, t = mcts_cases.inputs("small")
    s = cases.session(MS[0], "best")
    over = [i for i, (m, st) in enumerate(zip(s["moves"], s["status"])) if m == ref.KEEP and st == ref.READY]
    assert over
    got = run(binary, tmp_path, b[over], t[over], over, ["init", "search 3", "advance 1 0", "advance 0 64", "dump"], 64)
    assert got[1][1] == got[2][1] == [ref.BADMOVE] * len(over) and got[3][1] == [1] * len(over)
