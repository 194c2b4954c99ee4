"""The solver's C-ABI is declared, bound and exported as one set (oths_*), the
oth_* set of include/othello.h is untouched by it, and the exhaustive checker
the GPU tests rely on is right on cases worked out by hand (CPU only)."""
import ctypes
import re
import subprocess

import numpy as np

import codeobj
import oracle
import solve_ref
from subproc_amd import _lib


def solve_header_functions():
    src = open(_lib.SOLVE_HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(oths_\w+)\s*\(", src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_solve_header_binding_and_exports_are_one_set():
    names = solve_header_functions()
    assert names == ["oths_solve", "oths_solve_grid"]
    assert names == sorted(_lib.SOLVE_SIGNATURES)
    assert exported("oths") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.SOLVE_SIGNATURES[name][1], name


def test_oth_set_is_unchanged_by_the_solver():
    assert not any(n.startswith("oths_") for n in _lib.SIGNATURES)
    assert exported("oth") == set(_lib.SIGNATURES)
    assert "oths_" not in open(_lib.HEADER).read()


def test_header_constants_match_the_binding():
    src = open(_lib.SOLVE_HEADER).read()

    def const(name):
        return eval(re.search(r"#define %s\s+(\S+(?: << \d+\))?)" % name, src).group(1).replace("u", ""))

    assert const("OTHS_MAX_EMPTIES") == _lib.SOLVE_MAX_EMPTIES >= 12
    assert (const("OTHS_SKIPPED"), const("OTHS_SOLVED"), const("OTHS_INVALID"), const("OTHS_LIMIT")) == (
        _lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT) == (0, 1, 2, 3)
    assert const("OTHS_NO_MOVE") == _lib.SOLVE_NO_MOVE == 255
    assert const("OTHS_DEFAULT_NODE_LIMIT") == _lib.SOLVE_DEFAULT_NODE_LIMIT == 1 << 28


FULL = (1 << 64) - 1


def test_checker_zero_empties_gives_the_diff():
    black = 0x00000000FFFFFFFF | (1 << 40)  # 33 black, 31 white
    boards = np.array([[black, FULL ^ black], [black, FULL ^ black]], np.uint64)
    v, m, inner = solve_ref.solve(boards, np.array([1, 2], np.uint8))
    assert v.tolist() == [2, -2] and m.tolist() == [255, 255] and inner == 0


def test_checker_one_empty_is_one_oracle_step():
    """Position 1: a1 empty, b1 and h8 white, every other square black (61
    black, 2 white).  Black's only move a1 flips b1 alone: 63 - 1 = +62.
    White at a1 flanks the six black discs b2..g7 up to h8 and nothing else:
    2 + 1 + 6 = 9 against 55.  Position 2: h8 black as well, so White cannot
    move and passes, and Black's a1 takes the last white disc: 64 - 0."""
    # position 1: White can answer at a1 through the long diagonal
    white = (1 << 1) | (1 << 63)
    black = FULL ^ white ^ 1
    boards = np.array([[black, white]], np.uint64)
    assert oracle.legal(boards, np.array([1], np.uint8))[0] == 1
    assert oracle.legal(boards, np.array([2], np.uint8))[0] == 1
    st = oracle.step(boards, np.array([1], np.uint8), np.array([0], np.uint8))
    assert st["ret"][0] == 1 and st["flips"][0] == 2  # b1
    assert int(oracle.result(st["boards"])["diff"][0]) == 62
    v, m, inner = solve_ref.solve(boards, np.array([1], np.uint8))
    assert (v.tolist(), m.tolist(), inner) == ([62], [0], 0)
    st = oracle.step(boards, np.array([2], np.uint8), np.array([0], np.uint8))
    assert st["ret"][0] == 6  # b2..g7
    v, m, inner = solve_ref.solve(boards, np.array([2], np.uint8))  # White: 2 + 1 + 6 = 9 against 55
    assert (v.tolist(), m.tolist(), inner) == ([9 - 55], [0], 0)
    # position 2: h8 black too; White cannot move, passes, Black plays a1: 64 - 0
    white = 1 << 1
    black = FULL ^ white ^ 1
    boards = np.array([[black, white]], np.uint64)
    assert oracle.legal(boards, np.array([2], np.uint8))[0] == 0
    v, m, inner = solve_ref.solve(boards, np.array([2], np.uint8))
    assert (v.tolist(), m.tolist(), inner) == ([-64], [64], 0)
    v, m, inner = solve_ref.solve(boards, np.array([1], np.uint8))
    assert (v.tolist(), m.tolist(), inner) == ([64], [0], 0)


def test_checker_lowest_maximiser_and_turn_rule():
    """Two empties with equal-valued moves keep the lower square; turn 0 and 3 read as Black."""
    p = __import__("solve_cases").pool()[2]
    b, t = p["boards"][:64], p["turn"][:64]
    v, m, _ = solve_ref.solve(b, t)
    own = oracle.legal(b, t)
    for i in np.nonzero(own)[0]:
        best = None
        for sq in range(64):
            if int(own[i]) >> sq & 1:
                c = oracle.step(b[i:i + 1], t[i:i + 1], np.array([sq], np.uint8))["boards"]
                cv = -int(solve_ref.solve(c, 3 - t[i:i + 1])[0][0])
                if best is None or cv > best[0]:
                    best = (cv, sq)
        assert (int(v[i]), int(m[i])) == best, i
    black_to_move = np.full(64, 1, np.uint8)
    for other in (0, 3):
        vo, mo, _ = solve_ref.solve(b, np.full(64, other, np.uint8))
        vb, mb, _ = solve_ref.solve(b, black_to_move)
        assert (vo == vb).all() and (mo == mb).all()


def test_solve_kernel_is_scratch_free_and_fits_eight_blocks():
    """The solver's kernel is found by its name among the library's code
    objects (tests/codeobj.py).  No scratch (the search stack is LDS), and an
    LDS footprint that lets eight one-wave blocks share a CU's 160 KB."""
    found = [v for name, v in codeobj.kernels().items() if "solve_kernel" in name]
    assert len(found) == 1, found
    k = found[0]
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] * 8 <= 160 * 1024
    assert k["vgpr_count"] <= 128  # two waves per SIMD need no more than 256; leave room
