"""The per-move calls' C-ABI (include/othello_moves.h, otha_*) is declared,
bound and exported as one set beside the others, its constants equal the
binding's, its argument checks answer before anything is launched, the Python
layers refuse bad arguments before they touch a device, and its kernels use no
scratch and keep the search's footprint (CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw")
NAMES = ["otha_search_moves", "otha_search_moves_scratch_bytes", "otha_solve_moves", "otha_solve_moves_scratch_bytes",
         "otha_solve_moves_split", "otha_solve_moves_split_scratch_bytes"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_moves_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.MOVES_HEADER, "otha")
    assert names == NAMES == sorted(_lib.MOVES_SIGNATURES)
    assert exported("otha") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.MOVES_SIGNATURES[name][1], name
        assert fn.restype == _lib.MOVES_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.MOVES_HEADER, prefix)
    # the argument counts of the header's declarations are the binding's
    src = re.sub(r"/\*.*?\*/", "", open(_lib.MOVES_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.MOVES_SIGNATURES[name][1]), name
    # oths_solve's / othm_search's arguments with move_value in front of value and scratch, scratch_bytes in
    # front of work
    one = _lib.MOVES_SIGNATURES["otha_solve_moves"][1]
    assert one[:4] + one[5:9] + one[11:] == _lib.SOLVE_SIGNATURES["oths_solve"][1]
    srch = _lib.MOVES_SIGNATURES["otha_search_moves"][1]
    assert srch[:5] + srch[6:10] + srch[12:] == _lib.SEARCH_SIGNATURES["othm_search"][1]
    # the sets that were there are what they were
    assert exported("oths") == set(_lib.SOLVE_SIGNATURES) and exported("othm") == set(_lib.SEARCH_SIGNATURES)
    assert exported("othe") == set(_lib.SOLVE_TREE_SIGNATURES) and exported("othh") == set(_lib.SOLVE_HASH_SIGNATURES)
    assert exported("othw") == set(_lib.SOLVE_WINDOW_SIGNATURES)
    assert "otha_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_moves_constants_match_the_binding():
    src = open(_lib.MOVES_HEADER).read()

    def define(name):
        return eval(re.search(r"#define %s\s+(\(?[-\d ()]+?\)?)\s*(?:/\*|$)" % name, src, re.M).group(1))

    assert define("OTHA_NOT_A_MOVE") == _lib.MOVES_NOT_A_MOVE == -128
    assert define("OTHA_UNKNOWN") == _lib.MOVES_UNKNOWN == -127
    assert define("OTHA_NOT_A_MOVE32") == _lib.MOVES_NOT_A_MOVE32 == -2**31
    assert define("OTHA_UNKNOWN32") == _lib.MOVES_UNKNOWN32 == -2**31 + 1
    assert define("OTHA_SEARCH_SLOTS") == _lib.MOVES_SEARCH_SLOTS == 64
    # neither marker is a value: exact values lie in -64..64, search values within 64 * 2**17
    assert _lib.MOVES_UNKNOWN < -64 and _lib.MOVES_UNKNOWN32 < -64 * _lib.SEARCH_TERMINAL_SCALE


def test_scratch_sizes_and_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    one, split, srch = (lib.otha_solve_moves_scratch_bytes, lib.otha_solve_moves_split_scratch_bytes,
                        lib.otha_search_moves_scratch_bytes)
    assert one(0, 12) == 0 and one(-1, 12) == E and one(1, 13) == E and one(1, -1) == E
    # a board, a count, a value, a status, a turn and a square per slot; a kind and a count per position
    assert one(1000, 12) == 24 * 12 * 1000 + 2 * 1000 and one(1000, 0) == one(1000, 1) == 24 * 1000 + 2 * 1000
    assert one(3, 5) % 8 == 0
    assert srch(0) == 16 and srch(-1) == E and srch(1 << 60) == E
    assert srch(1000) == 16 + 1000 * (8 + 2 + 64 * 26)
    inner = lib.othe_scratch_bytes
    for n, e, npp in ((1, 16, 65536), (64, 14, 256), (5, 0, 64)):
        slots = n * max(e, 1)
        assert split(n, e, npp) == (24 * slots + 2 * n + 7) // 8 * 8 + inner(slots, npp)  # every slot costs a slab
    assert split(1, 17, 64) == E and split(1, 16, 63) == E and split(-1, 16, 64) == E
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    weights = (ctypes.c_int8 * 36)()
    mem = (ctypes.c_uint64 * 64)()
    base = (ctypes.addressof(mem) + 31) & ~31
    w, b, wt = ctypes.addressof(word), ctypes.addressof(boards), ctypes.addressof(weights)

    def solve(max_empties=12, work=w, n=0, bd=b, scratch=None, size=0):
        return lib.otha_solve_moves(bd, None, max_empties, 0, None, None, None, None, None, scratch, size, work, n, None)

    assert solve() == _lib.OTH_OK  # n == 0: nothing launched
    assert solve(max_empties=13) == E and solve(max_empties=-1) == E and solve(work=None) == E and solve(n=-1) == E
    assert solve(n=1, bd=None, scratch=base, size=512) == E and solve(n=1) == E  # no boards; no scratch
    assert solve(n=1, scratch=base, size=one(1, 12) - 1) == E and solve(n=1, scratch=base + 8, size=512) == E

    def spl(bits=0, gate=0, table=None, size=0, n=0, task_empties=10, max_empties=14, order=0, npp=64, work=w):
        return lib.otha_solve_moves_split(b, None, max_empties, task_empties, order, 0, npp, bits, gate, table, size,
                                          None, None, None, None, None, None, 0, work, n, None)

    assert spl() == _lib.OTH_OK and spl(bits=4, gate=6, table=base, size=512) == _lib.OTH_OK
    assert spl(bits=3, gate=6, table=base, size=512) == E and spl(bits=4, gate=0, table=base, size=512) == E
    assert spl(bits=4, gate=6, table=base + 8, size=512) == E and spl(bits=4, gate=6, table=base, size=511) == E
    assert spl(task_empties=0) == E and spl(task_empties=13) == E and spl(max_empties=17) == E
    assert spl(order=2) == E and spl(npp=63) == E and spl(n=-1) == E and spl(n=1) == E and spl(work=None) == E

    def search(depth=3, weights=wt, work=w, n=0, bd=b, scratch=None, size=0):
        return lib.otha_search_moves(bd, None, depth, weights, 0, None, None, None, None, None, scratch, size, work, n,
                                     None)

    assert search() == _lib.OTH_OK
    assert search(depth=0) == E and search(depth=9) == E and search(weights=None) == E and search(work=None) == E
    assert search(n=-1) == E and search(n=1) == E and search(n=1, bd=None, scratch=base, size=4096) == E
    assert search(n=1, scratch=base, size=srch(1) - 1) == E
    assert word.value == 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="32 bits"):
        ops.solve_moves(b, t, node_limit=1 << 32)
    with pytest.raises(ValueError, match="32 bits"):
        ops.search_moves(b, t, 3, node_limit=-1)
    with pytest.raises(ValueError, match="order needs task_empties"):
        ops.solve_moves(b, t, order=1)
    with pytest.raises(ValueError, match="table needs task_empties"):
        ops.solve_moves(b, t, table=object())
    with pytest.raises(TypeError, match="SolveTable"):
        ops.solve_moves(b, t, task_empties=4, table=object())
    with pytest.raises(ValueError, match="no CPU path"):
        ops.solve_moves(b, t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.search_moves(b, t, 2)
    assert ops.MovesResult._fields == ("move_value", "value", "best_move", "status", "nodes")
    assert {"solve_moves", "search_moves", "MovesResult"} <= set(ops.__all__)
    assert callable(engine.Engine.hint)


def test_the_new_kernels_use_no_scratch_and_keep_the_searchs_footprint():
    """search_moves_kernel is search.hip's loop: one-wave blocks, the frames
    and the widened table in LDS (7 x 9 x 64 words + 48 ints), registers for
    two waves per SIMD.  The expand and finish kernels use neither LDS nor
    scratch.  DESIGN.md §21 has the figures."""
    found = codeobj.named(("moves_expand", "moves_finish", "search_moves_kernel"))
    assert len(found) == 5, sorted(found)  # two expands, the finish for int8 and int32 rows, the search
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        if "search_moves_kernel" in name:
            assert k["group_segment_fixed_size"] == 7 * 9 * 64 * 4 + 48 * 4 == 16320, name
            assert k["vgpr_count"] <= 128, name
        else:
            assert k["group_segment_fixed_size"] == 0, name
    print({n: found[n] for n in sorted(found)})
