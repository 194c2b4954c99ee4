"""The principal-variation calls' C-ABI (include/othello_line.h, othl_*) is
declared, bound and exported as one set beside the others, its constants equal
the binding's and collide with no other header's status, its argument checks
answer before anything is launched, the Python layers refuse bad arguments
before they touch a device, and its kernels use no scratch and keep the
solver's and the search's footprint (CPU only)."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb")
NAMES = ["othl_search_line", "othl_search_line_grid", "othl_solve_line", "othl_solve_line_grid"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_line_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.LINE_HEADER, "othl")
    assert names == NAMES == sorted(_lib.LINE_SIGNATURES)
    assert exported("othl") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.LINE_SIGNATURES[name][1], name
        assert fn.restype == _lib.LINE_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.LINE_HEADER, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(_lib.LINE_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.LINE_SIGNATURES[name][1]), name
    # oths_solve's arguments with line, length in front of value and end_boards, end_turn in front of work
    one = _lib.LINE_SIGNATURES["othl_solve_line"][1]
    assert one[:4] + one[6:10] + one[12:] == _lib.SOLVE_SIGNATURES["oths_solve"][1]
    # otho_search_ordered's likewise, with depth_per_position after depth and order in front of the weights
    srch = _lib.LINE_SIGNATURES["othl_search_line"][1]
    assert srch[:3] + srch[4:7] + srch[9:13] + srch[15:] == _lib.ORDER_SIGNATURES["otho_search_ordered"][1]
    # the sets that were there are what they were
    assert exported("oths") == set(_lib.SOLVE_SIGNATURES) and exported("othm") == set(_lib.SEARCH_SIGNATURES)
    assert exported("otha") == set(_lib.MOVES_SIGNATURES) and exported("othb") == set(_lib.BUDGET_SIGNATURES)
    assert "othl_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_line_constants_match_the_binding_and_no_other_status():
    src = open(_lib.LINE_HEADER).read()

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, src).group(1))

    assert define("OTHL_LINE_STRIDE") == _lib.LINE_STRIDE == 32
    assert define("OTHL_BADDEPTH") == _lib.LINE_BADDEPTH == 6
    # the longest line, a pass before every move, fits the row
    assert 2 * _lib.SOLVE_MAX_EMPTIES <= _lib.LINE_STRIDE and 2 * _lib.SEARCH_MAX_DEPTH <= _lib.LINE_STRIDE
    # a status of its own: no other header gives the value to a status
    taken = {}
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        for name, v in re.findall(r"#define (OTH\w_(?:SKIPPED|SOLVED|SEARCHED|INVALID|LIMIT|NOROOM|BADWINDOW|BAD\w+))"
                                  r"\s+(\d+)", open(path).read()):
            taken.setdefault(int(v), set()).add(name)
    assert taken[6] == {"OTHL_BADDEPTH"}, taken
    assert {0, 1, 2, 3, 4, 5} <= set(taken)


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    weights = (ctypes.c_int8 * 36)()
    mem = (ctypes.c_uint64 * 16)()
    base = (ctypes.addressof(mem) + 31) & ~31
    w, b, wt = ctypes.addressof(word), ctypes.addressof(boards), ctypes.addressof(weights)

    def solve(max_empties=12, work=w, n=0, bd=b, line=None, end=None):
        return lib.othl_solve_line(bd, None, max_empties, 0, line, None, None, None, None, None, end, None, work, n,
                                   None)

    assert solve() == _lib.OTH_OK  # n == 0: nothing launched
    assert solve(line=base, end=base) == _lib.OTH_OK
    assert solve(max_empties=13) == E and solve(max_empties=-1) == E and solve(work=None) == E and solve(n=-1) == E
    assert solve(n=1, bd=None) == E
    assert solve(line=base + 8) == E and solve(end=base + 8) == E  # rows and end boards are written 16 bytes at a time

    def search(depth=3, per=None, order=0, weights=wt, work=w, n=0, bd=b, line=None, end=None):
        return lib.othl_search_line(bd, None, depth, per, order, weights, 0, line, None, None, None, None, None, end,
                                    None, work, n, None)

    assert search() == _lib.OTH_OK
    assert search(depth=0) == E and search(depth=9) == E and search(weights=None) == E and search(work=None) == E
    assert search(depth=0, per=b) == _lib.OTH_OK and search(depth=99, per=b) == _lib.OTH_OK  # depth is not read then
    assert search(order=2) == E and search(order=-1) == E and search(n=-1) == E and search(n=1, bd=None) == E
    assert search(line=base + 4) == E and search(end=base + 8) == E
    assert lib.othl_solve_line_grid(0) == 0 and lib.othl_search_line_grid(0, 0) == 0
    assert lib.othl_solve_line_grid(-1) == E and lib.othl_search_line_grid(-1, 1) == E
    assert lib.othl_search_line_grid(0, 2) == E
    assert word.value == 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, env, ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="32 bits"):
        ops.solve_line(b, t, node_limit=1 << 32)
    with pytest.raises(ValueError, match="32 bits"):
        ops.search_line(b, t, 3, node_limit=-1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.solve_line(b, t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.search_line(b, t, 2)
    assert ops.LineResult._fields == ("line", "length", "value", "best_move", "status", "nodes", "end_boards",
                                      "end_turn")
    assert {"solve_line", "search_line", "LineResult"} <= set(ops.__all__)
    assert callable(env.VecEnv.solve_line) and callable(env.VecEnv.search_line) and callable(engine.Engine.pv)


def test_the_line_kernels_use_no_scratch_and_keep_the_solvers_and_the_searchs_footprint():
    """One-wave blocks with the frames (and the widened table) in LDS: solve.hip's
    11 x 7 x 64 words, search.hip's 7 x 9 x 64 words + 48 ints, so eight blocks
    a CU; registers for two waves per SIMD.  DESIGN.md §24 has the figures."""
    found = codeobj.named(("line_exact_walk", "line_depth_walk", "line_depth_ordered_walk", "12solve_kernel",
                           "13search_kernel"))
    new = {n: k for n, k in found.items() if "line_" in n}
    assert len(new) == 3 and len(found) == 5, sorted(found)
    assert not any("solve_kernel" in n or "search_kernel" in n for n in new)
    for name, k in new.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["vgpr_count"] <= 128, name
        model = [v for n, v in found.items() if n not in new and ("solve" in n) == ("exact" in name)][0]
        assert k["group_segment_fixed_size"] == model["group_segment_fixed_size"], name
        assert k["group_segment_fixed_size"] == (11 * 7 * 64 * 4 if "exact" in name else 7 * 9 * 64 * 4 + 48 * 4), name
    print({n: found[n] for n in sorted(found)})
