"""The Monte Carlo tree search's C-ABI (include/othello_mcts.h, othu_*) is
declared, bound and exported as one set beside the others, its argument checks
answer before anything is launched, the Python layers refuse bad arguments
before they touch a device, and its kernel uses no scratch, at most 128 VGPRs
and the LDS the header states (CPU only)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb", "othl", "othx", "othc")
NAMES = ["othu_mcts", "othu_mcts_grid", "othu_mcts_scratch_bytes"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def header_constant(name):
    src = open(_lib.MCTS_HEADER).read()
    return eval(re.search(r"^#define %s\s+(\(?[^/\n]+?\)?)\s*(?:/\*.*)?$" % name, src, re.M).group(1).replace("u", ""))


def test_mcts_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.MCTS_HEADER, "othu")
    assert names == NAMES == sorted(_lib.MCTS_SIGNATURES)
    assert exported("othu") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.MCTS_SIGNATURES[name][1], name
        assert fn.restype == _lib.MCTS_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.MCTS_HEADER, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(_lib.MCTS_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.MCTS_SIGNATURES[name][1]), name
    # the sets that were there are what they were
    assert exported("othm") == set(_lib.SEARCH_SIGNATURES) and exported("otha") == set(_lib.MOVES_SIGNATURES)
    assert exported("othx") == set(_lib.PLAY_SOLVE_SIGNATURES) and exported("othl") == set(_lib.LINE_SIGNATURES)
    assert exported("othc") == set(_lib.PERFT_SIGNATURES) and exported("oths") == set(_lib.SOLVE_SIGNATURES)
    assert exported("oth") == set(_lib.SIGNATURES)
    assert "othu_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_the_constants_are_the_headers():
    for mine, name in ((_lib.MCTS_MAX_ITERATIONS, "OTHU_MAX_ITERATIONS"), (_lib.MCTS_MAX_NODES, "OTHU_MAX_NODES"),
                       (_lib.MCTS_MAX_BLOCKS, "OTHU_MAX_BLOCKS"), (_lib.MCTS_NODE_BYTES, "OTHU_NODE_BYTES"),
                       (_lib.MCTS_PATH_ENTRIES, "OTHU_PATH_ENTRIES"), (_lib.MCTS_LDS_BYTES, "OTHU_LDS_BYTES"),
                       (_lib.MCTS_SEARCHED, "OTHU_SEARCHED"), (_lib.MCTS_INVALID, "OTHU_INVALID"),
                       (_lib.MCTS_NO_MOVE, "OTHU_NO_MOVE")):
        assert mine == header_constant(name), name
    # the limits the rule rests on: 128 T exact in float32, |d| <= 4096 T in int32
    assert 128 * _lib.MCTS_MAX_ITERATIONS == 2**23 and 4096 * _lib.MCTS_MAX_ITERATIONS < 2**31
    assert _lib.MCTS_LDS_BYTES == 8 * 64 * 8 + 256 * 8 + 4 * _lib.MCTS_PATH_ENTRIES
    assert _lib.MCTS_PATH_ENTRIES >= 2 * 64 + 2


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    table = (ctypes.c_float * 8)()
    tp = ctypes.addressof(table)
    M = 1 << 20

    def mcts(T=5, nodes=64, log_table=tp, scratch=None, scratch_bytes=0, n=0, boards=None):
        return lib.othu_mcts(boards, None, T, 0.5, log_table, 0, 0, nodes, None, None, None, None, None, None, None,
                             None, scratch, scratch_bytes, n, None)

    assert mcts() == _lib.OTH_OK  # n == 0: nothing launched
    assert mcts(T=0) == E and mcts(T=65537) == E and mcts(T=-1) == E and mcts(T=65536) == _lib.OTH_OK
    assert mcts(nodes=0) == E and mcts(nodes=M + 1) == E and mcts(nodes=M) == _lib.OTH_OK and mcts(nodes=1) == 0
    assert mcts(log_table=None) == E and mcts(n=-1) == E
    assert mcts(n=1) == E  # no boards, no scratch
    fake = (ctypes.c_uint64 * 8)()
    fp = ctypes.addressof(fake) & ~15
    assert mcts(n=1, boards=fp, scratch=None, scratch_bytes=1 << 30) == E  # NULL scratch with n > 0
    assert mcts(n=1, boards=fp, scratch=fp, scratch_bytes=64 * 32 - 1) == E  # too few bytes
    assert mcts(n=3, boards=fp, scratch=fp, scratch_bytes=2 * 64 * 32) == E
    assert mcts(n=1, boards=fp, scratch=fp + 8, scratch_bytes=1 << 30) == E  # not 16-byte aligned
    sb = lib.othu_mcts_scratch_bytes
    assert sb(1, 64) == 64 * 32 and sb(3, 64) == 3 * 64 * 32 and sb(0, 64) == 16 and sb(1, M) == 32 * M
    assert sb(4096, 7) == sb(100000, 7) == 4096 * 7 * 32  # a slab per block, never more than OTHU_MAX_BLOCKS
    assert sb(-1, 64) == E and sb(1, 0) == E and sb(1, M + 1) == E
    assert lib.othu_mcts_grid(0) == 0 and lib.othu_mcts_grid(-1) == E


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, env, ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mcts(b, t, 5)
    for T in (0, -1, 65537):
        with pytest.raises(ValueError, match="iterations must lie"):
            ops.mcts(b, t, T)
        with pytest.raises(ValueError, match="iterations must lie"):
            ops.mcts_log_table(T)
    for M in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_nodes must lie"):
            ops.mcts(b, t, 5, max_nodes=M)
    with pytest.raises(ValueError, match="finite"):
        ops.mcts(b, t, 5, explore=float("nan"))
    assert ops.MctsResult._fields == ("visits", "wins", "diffs", "root_wins", "root_diffs", "best_move", "status",
                                      "nodes")
    assert {"mcts", "mcts_log_table", "MctsResult"} <= set(ops.__all__) and callable(env.VecEnv.mcts)
    table = ops.mcts_log_table(6)
    assert table.dtype == np.float32 and table.shape == (7,) and table[0] == 0 and table[1] == 0
    assert (table == np.log(np.arange(7, dtype=np.float64).clip(1)).astype(np.float32)).all()
    with pytest.raises(ValueError, match="needs iterations"):
        engine.Engine(policy="mcts")
    with pytest.raises(ValueError, match="needs iterations"):
        engine.Engine(policy="mcts", iterations=65537)
    with pytest.raises(ValueError, match="applies to policy mcts"):
        engine.Engine(policy="greedy", iterations=8)
    eng = engine.Engine(policy="mcts", iterations=8, explore=0.25)
    out = []
    assert eng.handle("verbose p", out.append) and out == ["GPU policy=mcts iterations=8 explore=0.25"]


def test_the_mcts_kernel_uses_no_scratch_and_the_lds_the_header_states():
    """One one-wave kernel: the ray and k-th bit tables and the path in LDS,
    6,672 B, at most 128 VGPRs (four waves a SIMD).  DESIGN.md §28 has the
    figures."""
    found = codeobj.named(("mcts_kernel",))
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == _lib.MCTS_LDS_BYTES, name
        assert k["vgpr_count"] <= 128, name
    print(found)
