"""The windowed solvers' C-ABI (include/othello_solve_window.h, othw_*) is
declared, bound and exported as one set beside the others, its constants equal
the cores' and the binding's, its argument checks answer before anything is
launched, ops.solve refuses bad windows before it touches a device, and the
kernels it changed keep the solver's footprint (CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh")


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_window_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.SOLVE_WINDOW_HEADER, "othw")
    assert names == ["othw_solve", "othw_solve_split"] == sorted(_lib.SOLVE_WINDOW_SIGNATURES)
    assert exported("othw") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.SOLVE_WINDOW_SIGNATURES[name][1], name
        assert fn.restype == _lib.SOLVE_WINDOW_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.SOLVE_WINDOW_HEADER, prefix)
    # oths_solve's arguments with alpha, beta after turn; othh_solve_hashed's with alpha, beta in front of hash_bits
    one, split = (_lib.SOLVE_WINDOW_SIGNATURES[n][1] for n in names)
    assert one[:2] + one[4:] == _lib.SOLVE_SIGNATURES["oths_solve"][1]
    assert split[:15] + split[17:] == _lib.SOLVE_HASH_SIGNATURES["othh_solve_hashed"][1]
    # the sets that were there are what they were
    assert exported("oths") == set(_lib.SOLVE_SIGNATURES) == {"oths_solve", "oths_solve_grid"}
    assert exported("othe") == set(_lib.SOLVE_TREE_SIGNATURES)
    assert exported("othh") == set(_lib.SOLVE_HASH_SIGNATURES)


def test_window_constants_match_the_binding_and_the_cores():
    src = open(_lib.SOLVE_WINDOW_HEADER).read()
    assert int(re.search(r"#define OTHW_ALPHA_MIN\s+\((-\d+)\)", src).group(1)) == _lib.SOLVE_ALPHA_MIN == -65
    assert int(re.search(r"#define OTHW_BETA_MAX\s+(\d+)", src).group(1)) == _lib.SOLVE_BETA_MAX == 65
    solve = open(_lib.SOLVE_HEADER).read()
    assert int(re.search(r"#define OTHS_BADWINDOW\s+(\d+)", solve).group(1)) == _lib.SOLVE_BADWINDOW == 5
    taken = {_lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT, _lib.SOLVE_TREE_NOROOM}
    assert _lib.SOLVE_BADWINDOW not in taken
    core = open(os.path.join(ROOT, "subproc_amd", "csrc", "solve_core.hpp")).read()
    assert re.search(r"kBadWindow = 5;", core) and re.search(r"kInf = 65;", core)
    tree = open(os.path.join(ROOT, "subproc_amd", "csrc", "solve_tree_core.hpp")).read()
    assert re.search(r"kInf = 65;", tree)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    mem = (ctypes.c_uint64 * (4 * 16 + 4))()
    base = (ctypes.addressof(mem) + 31) & ~31
    w, b = ctypes.addressof(word), ctypes.addressof(boards)

    def one(max_empties=12, work=w, n=0, bd=b):
        return lib.othw_solve(bd, None, None, None, max_empties, 0, None, None, None, None, work, n, None)

    assert one() == _lib.OTH_OK  # n == 0: nothing launched
    assert one(max_empties=13) == E and one(max_empties=-1) == E and one(work=None) == E and one(n=-1) == E
    assert one(n=1, bd=None) == E

    def split(bits=0, gate=0, table=None, size=0, n=0, task_empties=10, max_empties=14, order=0, npp=64):
        return lib.othw_solve_split(b, None, max_empties, task_empties, order, 0, None, None, None, None, None, 0, npp,
                                    w, n, None, None, bits, gate, table, size, None)

    assert split() == _lib.OTH_OK  # no table, n == 0
    assert split(bits=4, gate=6, table=base, size=512) == _lib.OTH_OK
    # a table with hash_bits 0, or hash_bits without a table: othh_solve_hashed's checks
    assert split(table=base, size=512) == E and split(bits=4, gate=6) == E
    assert split(bits=3, gate=6, table=base, size=512) == E and split(bits=4, gate=0, table=base, size=512) == E
    assert split(bits=4, gate=6, table=base + 8, size=512) == E and split(bits=4, gate=6, table=base, size=511) == E
    # othe_solve's own checks hold
    assert split(task_empties=0) == E and split(max_empties=17) == E and split(order=2) == E and split(npp=63) == E
    assert split(n=-1) == E and split(n=1) == E  # no scratch
    assert word.value == 0


def test_ops_solve_refuses_bad_windows_before_it_touches_a_device():
    import torch

    from subproc_amd import ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the window checks would raise
    t = torch.ones(3, dtype=torch.uint8)        # ValueError too, so each message is matched
    with pytest.raises(ValueError, match="wld=True is window"):
        ops.solve(b, t, window=(-1, 1), wld=True)
    for window in ((-66, 0), (0, 66), (-100, 100)):
        with pytest.raises(ValueError, match="must lie in -65..65"):
            ops.solve(b, t, window=window)
    for window in ((3, 3), (5, -5)):
        with pytest.raises(ValueError, match="alpha < beta"):
            ops.solve(b, t, window=window)
    for window in ((0,), (0, 1, 2), 7):
        with pytest.raises(ValueError, match="pair"):
            ops.solve(b, t, window=window)
    for window in ((0.5, 1), (True, 2), ("a", 1)):
        with pytest.raises(ValueError, match="must be an int"):
            ops.solve(b, t, window=window)
    with pytest.raises(ValueError, match="wld=True is window"):
        ops.solve(b, t, task_empties=6, window=(0, 1), wld=True)


def test_engine_checks_solve_wld_empties():
    from subproc_amd import engine

    for bad in (dict(solve_wld_empties=13), dict(solve_wld_empties=17, solve_task_empties=8),
                dict(solve_wld_empties=-1), dict(solve_empties=10, solve_wld_empties=10),
                dict(solve_empties=12, solve_wld_empties=11)):
        with pytest.raises(ValueError):
            engine.Engine(**bad)
    e = engine.Engine(solve_empties=10, solve_wld_empties=16, solve_task_empties=8)
    assert e.solve_wld_empties == 16 and e.solve_empties == 10
    assert engine.Engine().solve_wld_empties == 0


def test_the_windowed_kernels_keep_the_solvers_footprint():
    """One-wave blocks with the frames in LDS ([depth][field][lane], 19.25 KB),
    no scratch, and registers for two waves per SIMD: eight blocks share a CU,
    as before the window (DESIGN.md §20 has the figures beside the parent's)."""
    found = codeobj.named(("solve_windowed", "split_window_tasks"))
    # the one-lane kernel and the task kernel plain or hashed, in either move order
    assert len(found) == 5 and sum("solve_windowed" in k for k in found) == 1, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 11 * 7 * 64 * 4 == 19712, name
        assert k["vgpr_count"] <= 128, name
