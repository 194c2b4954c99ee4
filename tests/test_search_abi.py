"""The depth-limited search's C-ABI is declared, bound and exported as one set
(othm_*) beside the oth_* and oths_* sets, its kernel keeps the stack in LDS,
and the exhaustive checker the GPU tests rely on is right on cases worked out
by hand (CPU only)."""
import ctypes
import re
import subprocess

import numpy as np

import codeobj
import oracle
import search_ref
from subproc_amd import _lib, params

T = search_ref.T
FULL = (1 << 64) - 1
DEFAULT = np.asarray(params.DEFAULT_WEIGHTS, np.int8)


def search_header_functions():
    src = open(_lib.SEARCH_HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(othm_\w+)\s*\(", src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_search_header_binding_and_exports_are_one_set():
    names = search_header_functions()
    assert names == ["othm_search", "othm_search_grid"]
    assert names == sorted(_lib.SEARCH_SIGNATURES)
    assert exported("othm") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.SEARCH_SIGNATURES[name][1], name
    assert not any(n.startswith("othm_") for n in {**_lib.SIGNATURES, **_lib.SOLVE_SIGNATURES})
    assert "othm_" not in open(_lib.HEADER).read() and "othm_" not in open(_lib.SOLVE_HEADER).read()


def test_header_constants_match_the_binding():
    src = open(_lib.SEARCH_HEADER).read()

    def const(name):
        return eval(re.search(r"#define %s\s+(\(?\w+(?: << \d+\))?)" % name, src).group(1).replace("u", ""))

    assert const("OTHM_MAX_DEPTH") == _lib.SEARCH_MAX_DEPTH == 8
    assert const("OTHM_TERMINAL_SCALE") == _lib.SEARCH_TERMINAL_SCALE == T == 1 << 17
    assert (const("OTHM_SEARCHED"), const("OTHM_INVALID"), const("OTHM_LIMIT")) == (
        _lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT) == (
        _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT)
    assert const("OTHM_NO_MOVE") == _lib.SEARCH_NO_MOVE == 255
    assert const("OTHM_DEFAULT_NODE_LIMIT") == _lib.SEARCH_DEFAULT_NODE_LIMIT == 1 << 28
    # any eval stays below T: a decided game outranks it
    assert 9 * 128 * 64 < T


def test_search_kernel_is_scratch_free_and_fits_eight_blocks():
    """As the solver's: the search kernel is found by its name; no scratch (the
    stack is LDS) and an LDS footprint that lets eight one-wave blocks share a
    CU's 160 KB."""
    found = [v for name, v in codeobj.kernels().items() if "search_kernel" in name]
    assert len(found) == 1, found
    k = found[0]
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] * 8 <= 160 * 1024
    assert k["vgpr_count"] <= 128  # two waves per SIMD need no more than 256; leave room


# ---------------------------------------------------------------- the checker, by hand
def test_checker_full_board_gives_t_times_the_diff():
    black = 0x00000000FFFFFFFF | (1 << 40)  # 33 black, 31 white
    boards = np.array([[black, FULL ^ black], [black, FULL ^ black]], np.uint64)
    for depth in (1, 8):
        v, m, _ = search_ref.search(boards, np.array([1, 2], np.uint8), depth, DEFAULT)
        assert v.tolist() == [2 * T, -2 * T] and m.tolist() == [255, 255]


def test_checker_root_that_must_pass():
    """a1 empty, b1 white, every other square black: White cannot move and
    passes (no depth spent), Black's a1 takes the last white disc and ends the
    game 64 - 0, whatever the depth and the table."""
    white = 1 << 1
    black = FULL ^ white ^ 1
    boards = np.array([[black, white]], np.uint64)
    assert oracle.legal(boards, np.array([2], np.uint8))[0] == 0
    assert oracle.legal(boards, np.array([1], np.uint8))[0] == 1
    for depth in (1, 2, 8):
        for w in (DEFAULT, search_ref.WEIGHTS_B):
            v, m, _ = search_ref.search(boards, np.array([2], np.uint8), depth, w)
            assert (v.tolist(), m.tolist()) == ([-64 * T], [64])
            v, m, _ = search_ref.search(boards, np.array([1], np.uint8), depth, w)
            assert (v.tolist(), m.tolist()) == ([64 * T], [0])


def test_checker_depth_one_leaf_is_the_root_movers_eval():
    """The opening, depth 1: each child's score is oracle.evaluate(child, root
    mover), worked out here move by move; the four children are images of one
    another, so all four tie and the lowest square (d3 = 19) is kept."""
    b, t, _ = oracle.reset(1)
    own = int(oracle.legal(b, t)[0])
    sqs = [s for s in range(64) if own >> s & 1]
    assert sqs == [19, 26, 37, 44]
    for w in (DEFAULT, search_ref.WEIGHTS_B):
        ev = []
        for s in sqs:
            c = oracle.step(b, t, np.array([s], np.uint8))["boards"]
            ev.append(int(oracle.evaluate(c, t, w)[0]))
        assert len(set(ev)) == 1
        v, m, ex = search_ref.search(b, t, 1, w)
        assert (v.tolist(), m.tolist(), ex) == ([ev[0]], [19], 5)


def test_checker_two_empties_equal_maximisers_keep_the_lower_square():
    """Two-empties roots of the solver's pool at full depth: the value is T *
    the best child's disc difference, by one oracle step per move and the
    exhaustive solver below it; among equal moves the lower square is kept, and
    at least one root has such a tie."""
    import solve_cases
    import solve_ref

    p = solve_cases.pool()[2]
    b, t = p["boards"][:64], p["turn"][:64]
    v, m, _ = search_ref.search(b, t, 2, DEFAULT)
    own = oracle.legal(b, t)
    ties = 0
    for i in np.nonzero(own)[0]:
        scores = []
        for sq in range(64):
            if int(own[i]) >> sq & 1:
                c = oracle.step(b[i:i + 1], t[i:i + 1], np.array([sq], np.uint8))["boards"]
                scores.append((-int(solve_ref.solve(c, 3 - t[i:i + 1])[0][0]), sq))
        top = max(s for s, _ in scores)
        best = min(sq for s, sq in scores if s == top)
        ties += sum(s == top for s, _ in scores) > 1
        assert (int(v[i]), int(m[i])) == (T * top, best), i
    assert ties >= 1
