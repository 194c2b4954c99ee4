"""The principal variation on the host (tools/diag/line_host.cpp: line_core.hpp's
layer in plain C++ around solve_core.hpp's, search_core.hpp's and
order_core.hpp's machines) against tests/line_ref.py's walk over the oracle.
DESIGN.md §24.

Exact: every position of solve_cases.cases() at 0..8 empties.  Search: mid3 and
special3 at depths 1..4, both tables, both orders; depth 8 at 6 empties, where
the line must be the exact line; a per-position depth array holding 0, 1, 8 and
9.  The same under -fsanitize=address,undefined, as a process of its own.
CPU only."""
import numpy as np
import pytest

import host_programs as hp
import line_ref
import solve_cases
import tree_cases

SOLVED, INVALID, LIMIT, BADDEPTH = 1, 2, 3, 6
FIELDS = ("value", "best_move", "status", "nodes", "length", "end_boards", "end_turn", "line")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "line_host")


@pytest.fixture(scope="module")
def binary_asan(tmp_path_factory):
    return hp.compiled(tmp_path_factory, "line_host", hp.SANITIZED)


def read_lines(path, n):
    rows = [ln.split() for ln in open(path)]
    assert len(rows) == n
    return dict(value=np.array([int(r[0]) for r in rows], np.int64), best_move=np.array([int(r[1]) for r in rows]),
                status=np.array([int(r[2]) for r in rows]), nodes=np.array([int(r[3]) for r in rows], np.int64),
                length=np.array([int(r[4]) for r in rows]),
                end_boards=np.array([[int(r[5], 16), int(r[6], 16)] for r in rows], np.uint64).reshape(n, 2),
                end_turn=np.array([int(r[7]) for r in rows]),
                line=np.array([list(bytes.fromhex(r[8])) for r in rows], np.uint8).reshape(n, line_ref.STRIDE))


def run_solve(exe, tmp, boards, turn, max_empties=12, limit=0):
    inp, out = str(tmp / "lin"), str(tmp / "lout")
    hp.write_positions(inp, boards, turn)
    hp.run([exe, "solve", inp, out, max_empties, limit, 8])
    return read_lines(out, len(turn))


def run_search(exe, tmp, boards, turn, depth, weights, order=0, limit=0):
    """depth: an int, or an array of n (the per-position form)."""
    inp, out, wf = str(tmp / "lin"), str(tmp / "lout"), str(tmp / "lw")
    per = not np.isscalar(depth)
    hp.write_positions(inp, boards, turn, depth if per else None)
    hp.write_weights(wf, weights)
    hp.run([exe, "search", inp, out, wf, -1 if per else depth, order, limit, 8])
    return read_lines(out, len(turn))


def same_line(got, want, what, scale=1):
    """A host or device result against line_ref's (whose value is scaled by `scale`)."""
    for k in ("line", "length", "best_move", "end_boards", "end_turn"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:4]], w[bad[:4]])
    bad = np.nonzero(np.asarray(got["value"], np.int64) != scale * np.asarray(want["value"], np.int64))[0]
    assert len(bad) == 0, (what, "value", bad[:8])


def exact_checks(exe, tmp, lo, hi):
    b, t = line_ref.exact_inputs(lo, hi)
    got = run_solve(exe, tmp, b, t)
    assert (got["status"] == SOLVED).all()
    same_line(got, line_ref.exact_cases(lo, hi), ("exact", lo, hi))
    assert (line_ref.end_score(got["end_boards"], t) == got["value"]).all()
    cs = solve_cases.cases()
    forced = np.concatenate([cs[e]["forced_pass"] for e in range(lo, hi + 1)])
    over = np.concatenate([cs[e]["over"] for e in range(lo, hi + 1)])
    assert forced.any() and over.any()
    assert (got["line"][forced, 0] == 64).all() and (got["length"][over] == 0).all()
    assert (got["best_move"][over] == 255).all() and (got["nodes"][over] == 0).all()
    return got


def search_checks(exe, tmp, names=("mid3", "special3"), depths=(1, 2, 3, 4)):
    for name in names:
        b, t = tree_cases.inputs(name)
        for table in tree_cases.BOTH:
            w = tree_cases.TABLES[table]
            for depth in depths:
                want = line_ref.search_case(name, depth, table)
                for order in (0, 1):
                    got = run_search(exe, tmp, b, t, depth, w, order)
                    assert (got["status"] == SOLVED).all()
                    same_line(got, want, (name, table, depth, order))
                    assert (line_ref.end_score(got["end_boards"], t, w) == got["value"]).all()


def deep_and_mixed_checks(exe, tmp):
    cs = solve_cases.cases()[6]
    b, t = cs["boards"][:48], cs["turn"][:48]
    lo = sum(len(solve_cases.cases()[e]["turn"]) for e in range(6))
    want = {k: v[lo:lo + 48] for k, v in line_ref.exact_cases(0, 8).items()}
    w = tree_cases.TABLES["rng7"]
    for order in (0, 1):
        same_line(run_search(exe, tmp, b, t, 8, w, order), want, ("depth 8 at 6 empties", order), scale=line_ref.T)
    # per-position depths: 0 is not searched, 9 is out of range, an overlapping board comes before either
    depths = np.array([(0, 1, 8, 9)[i % 4] for i in range(len(t) + 1)])
    b2 = np.concatenate([b, np.array([[3, 1]], np.uint64)])
    t2 = np.concatenate([t, np.array([1], np.uint8)])
    depths[-1] = 9
    got = run_search(exe, tmp, b2, t2, depths, w, 1)
    assert got["status"][-1] == INVALID
    body = {k: v[:-1] for k, v in got.items()}
    d = depths[:-1]
    assert (body["status"] == np.where(d == 0, LIMIT, np.where(d == 9, BADDEPTH, SOLVED))).all()
    off = (d == 0) | (d == 9)
    off_all = np.concatenate([off, [True]])
    assert (got["length"][off_all] == 0).all() and (got["value"][off_all] == 0).all()
    assert (got["best_move"][off_all] == 255).all() and (got["nodes"][off_all] == 0).all()
    assert (got["line"][off_all] == 255).all() and (got["end_boards"][off_all] == b2[off_all]).all()
    for depth, scale in ((1, 1), (8, line_ref.T)):
        sel = d == depth
        ref = line_ref.search(b[sel], t[sel], depth, w) if depth == 1 else {k: v[sel] for k, v in want.items()}
        same_line({k: v[sel] for k, v in body.items()}, ref, ("per-position", depth), scale=scale)


def test_exact_lines_on_the_host_are_the_walk_over_the_oracle(binary, tmp_path):
    got = exact_checks(binary, tmp_path, 0, 8)
    # max_empties is classified first
    b, t = line_ref.exact_inputs(0, 8)
    few = run_solve(binary, tmp_path, b, t, max_empties=5)
    emp = line_ref.solve_ref.empties(b)
    assert (few["status"] == np.where(emp > 5, 0, SOLVED)).all()
    skipped = emp > 5
    assert (few["length"][skipped] == 0).all() and (few["line"][skipped] == 255).all()
    for k in FIELDS:
        assert (few[k][~skipped] == got[k][~skipped]).all(), k


@pytest.mark.parametrize("name", ["mid3", "special3"])
def test_search_lines_on_the_host_are_the_walk_over_the_oracle(binary, tmp_path, name):
    search_checks(binary, tmp_path, names=(name,))


def test_depth_eight_is_the_exact_line_and_depths_per_position(binary, tmp_path):
    deep_and_mixed_checks(binary, tmp_path)


def test_a_node_limit_is_all_or_nothing_and_keeps_what_the_root_search_resolves(binary, tmp_path):
    b, t = tree_cases.inputs("mid4")
    w = tree_cases.TABLES["default"]
    free = run_search(binary, tmp_path, b, t, 4, w, 0)
    # the root search is the walk's largest (the subset argument): a limit between the smallest and the largest
    # walk's sum cuts some roots and not others
    limit = int(np.median(free["nodes"])) // 2
    got = run_search(binary, tmp_path, b, t, 4, w, 0, limit=limit)
    cut = got["status"] == LIMIT
    assert cut.any() and (~cut).any()
    assert (got["length"][cut] == 0).all() and (got["value"][cut] == 0).all() and (got["best_move"][cut] == 255).all()
    assert (got["line"][cut] == 255).all()
    for k in FIELDS:
        assert (got[k][~cut] == free[k][~cut]).all(), k


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(binary_asan, tmp_path):
    exact_checks(binary_asan, tmp_path, 0, 8)
    search_checks(binary_asan, tmp_path)
    deep_and_mixed_checks(binary_asan, tmp_path)
