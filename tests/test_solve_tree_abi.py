"""The split solver's C-ABI is declared, bound and exported as one set (othe_*)
beside the oth_*, oths_*, othm_*, othp_*, otht_* and otho_* sets, its constants
match the binding, its argument checks answer before anything is launched, and
its task kernels keep the stack in LDS at the solver's own footprint (CPU only;
resources, not instructions)."""
import ctypes
import os
import re
import subprocess

import codeobj
from subproc_amd import _lib

OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho")


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_solve_tree_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.SOLVE_TREE_HEADER, "othe")
    assert names == ["othe_scratch_bytes", "othe_solve", "othe_solve_grid"]
    assert names == sorted(_lib.SOLVE_TREE_SIGNATURES)
    assert exported("othe") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.SOLVE_TREE_SIGNATURES[name][1], name
        assert fn.restype == _lib.SOLVE_TREE_SIGNATURES[name][0], name
    # disjoint from the six other sets, in the bindings and in the headers
    others = {**_lib.SIGNATURES, **_lib.SOLVE_SIGNATURES, **_lib.SEARCH_SIGNATURES, **_lib.PLAY_SIGNATURES,
              **_lib.TREE_SIGNATURES, **_lib.ORDER_SIGNATURES}
    assert not any(n.startswith("othe_") for n in others)
    for h in (_lib.HEADER, _lib.SOLVE_HEADER, _lib.SEARCH_HEADER, _lib.PLAY_HEADER, _lib.TREE_HEADER,
              _lib.ORDER_HEADER):
        assert "othe_" not in open(h).read(), h
    for prefix in OTHERS:
        assert not header_functions(_lib.SOLVE_TREE_HEADER, prefix)
    # the other sets are what they were
    assert exported("oths") == set(_lib.SOLVE_SIGNATURES) == {"oths_solve", "oths_solve_grid"}
    assert exported("otht") == set(_lib.TREE_SIGNATURES)
    assert exported("otho") == set(_lib.ORDER_SIGNATURES)
    assert exported("oth") == set(_lib.SIGNATURES)


def test_header_constants_match_the_binding():
    src = open(_lib.SOLVE_TREE_HEADER).read()

    def const(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, src).group(1))

    assert const("OTHE_MAX_EMPTIES") == _lib.SOLVE_TREE_MAX_EMPTIES == 16 == _lib.SOLVE_MAX_EMPTIES + 4
    assert const("OTHE_NOROOM") == _lib.SOLVE_TREE_NOROOM == 4
    assert const("OTHE_MIN_NODES") == _lib.SOLVE_TREE_MIN_NODES == 64
    # a status of its own, beside the solver's four
    assert _lib.SOLVE_TREE_NOROOM not in (_lib.SOLVE_SKIPPED, _lib.SOLVE_SOLVED, _lib.SOLVE_INVALID, _lib.SOLVE_LIMIT)
    # the root's children always fit the smallest slab
    assert 1 + 33 <= _lib.SOLVE_TREE_MIN_NODES <= _lib.SOLVE_TREE_DEFAULT_NODES
    # the cores say the same
    here = os.path.dirname(_lib.LIB_PATH)
    core = open(os.path.join(here, "..", "csrc", "solve_tree_core.hpp")).read()
    assert re.search(r"kMaxEmpties = 16;", core) and re.search(r"kNoRoom = 4;", core) and re.search(
        r"kMinNodes = 64;", core)
    order = open(os.path.join(here, "..", "csrc", "solve_order_core.hpp")).read()
    k = int(re.search(r"#define OTHS_MOBILITY_EMPTIES (\d+)", order).group(1))
    assert 3 <= k <= 6
    assert int(re.search(r"at least (\d+)\s+\*?\s*empty squares", src).group(1)) == k  # the header states the rule


def test_bad_arguments_are_refused_before_any_launch():
    """Every check below answers from the host side of the call: no device is
    needed, and none of the pointers is touched."""
    lib = _lib.load()
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    w, b = ctypes.addressof(word), ctypes.addressof(boards)

    def call(max_empties=14, task_empties=10, order=0, npp=64, work=w, n=1, brd=b, scratch=None, size=0):
        return lib.othe_solve(brd, None, max_empties, task_empties, order, 0, None, None, None, None, scratch, size, npp,
                              work, n, None)

    E = _lib.OTH_EINVAL
    assert call(max_empties=-1) == E and call(max_empties=17) == E
    assert call(task_empties=0) == E and call(task_empties=13) == E and call(task_empties=-1) == E
    assert call(order=2) == E and call(order=-1) == E
    assert call(npp=63) == E and call(work=None) == E and call(n=-1) == E and call(brd=None) == E
    assert call(scratch=None, size=1 << 30) == E  # valid arguments, no scratch
    assert call(n=0) == _lib.OTH_OK               # nothing launched
    assert call(n=0, max_empties=17) == E and call(n=0, task_empties=0) == E and call(n=0, order=2) == E
    assert word.value == 0


def test_scratch_bytes_and_grid_edges_need_no_device():
    lib = _lib.load()
    assert lib.othe_scratch_bytes(0, 64) >= 0
    one = lib.othe_scratch_bytes(1, 64)
    assert one >= 64 * 48 + 64 * 4
    assert lib.othe_scratch_bytes(2, 64) > one
    assert lib.othe_scratch_bytes(1, _lib.SOLVE_TREE_DEFAULT_NODES) >= _lib.SOLVE_TREE_DEFAULT_NODES * 52
    assert lib.othe_scratch_bytes(1, 63) == _lib.OTH_EINVAL
    assert lib.othe_scratch_bytes(-1, 64) == _lib.OTH_EINVAL
    assert lib.othe_scratch_bytes(1 << 40, 1 << 30) == _lib.OTH_EINVAL
    assert lib.othe_solve_grid(0) == 0 and lib.othe_solve_grid(-1) == _lib.OTH_EINVAL


def test_task_kernels_are_scratch_free_at_the_solvers_lds_and_occupancy():
    """No scratch in any of the four kernels; the two task kernels take no more
    LDS than solve_kernel (11 frames of 7 words, 19.25 KB: eight one-wave
    blocks in a CU's 160 KB) and stay in its occupancy class (two waves per
    SIMD: at most 256 VGPRs; they are held to 128)."""
    wanted = ("solve_kernel", "split_solve_tasks", "split_solve_tasks_ordered", "split_solve_expand",
              "split_solve_prefix")
    found = codeobj.grouped(wanted, r"\d+%sE")  # the mangled name ends the identifier there
    assert {k: len(v) for k, v in found.items()} == {k: 1 for k in wanted}, found
    for name, (k,) in found.items():
        assert k["private_segment_fixed_size"] == 0, name
    ref = found["solve_kernel"][0]
    assert ref["group_segment_fixed_size"] == 11 * 7 * 64 * 4
    for name in ("split_solve_tasks", "split_solve_tasks_ordered"):
        k = found[name][0]
        assert k["group_segment_fixed_size"] <= ref["group_segment_fixed_size"], name
        assert k["vgpr_count"] <= 128, (name, k)
