"""The wide Monte Carlo tree search's C-ABI (include/othello_mcts_wide.h,
othv_*) is declared, bound and exported as one set beside the others, its
constants are the binding's, its argument checks answer before anything is
launched, the Python layers refuse bad arguments before they touch a device,
and its kernel uses no scratch and the LDS the header states (CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb", "othl", "othx", "othc",
          "othu", "othr")
NAMES = ["othv_mcts_wide", "othv_mcts_wide_grid", "othv_mcts_wide_scratch_bytes"]


def header_functions(path, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_the_header_the_binding_and_the_exports_are_one_set():
    names = header_functions(_lib.MCTS_WIDE_HEADER, "othv")
    assert names == NAMES == sorted(_lib.MCTS_WIDE_SIGNATURES)
    assert exported("othv") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.MCTS_WIDE_SIGNATURES[name][1] and fn.restype == _lib.MCTS_WIDE_SIGNATURES[name][0]
    for prefix in OTHERS:  # the new prefix is nobody else's, and this header declares nothing of theirs
        assert not header_functions(_lib.MCTS_WIDE_HEADER, prefix)
    inc = os.path.join(ROOT, "include")
    for other in os.listdir(inc):
        if other != "othello_mcts_wide.h":
            assert not header_functions(os.path.join(inc, other), "othv"), other
    src = re.sub(r"/\*.*?\*/", "", open(_lib.MCTS_WIDE_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.MCTS_WIDE_SIGNATURES[name][1]), name
    # the sets that were there are what they were
    assert exported("othu") == set(_lib.MCTS_SIGNATURES) and exported("othr") == set(_lib.MCTS_TREE_SIGNATURES)
    assert "othv_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()
    # the call is othu_mcts's with `leaves` after `iterations`
    one = _lib.MCTS_SIGNATURES["othu_mcts"][1]
    assert _lib.MCTS_WIDE_SIGNATURES["othv_mcts_wide"][1] == one[:3] + [ctypes.c_int] + one[3:]


def test_the_constants_are_the_headers():
    src = open(_lib.MCTS_WIDE_HEADER).read()
    for mine, name in ((_lib.MCTS_WIDE_MAX_LEAVES, "OTHV_MAX_LEAVES"), (_lib.MCTS_WIDE_MAX_BLOCKS, "OTHV_MAX_BLOCKS"),
                       (_lib.MCTS_WIDE_LDS_BYTES, "OTHV_LDS_BYTES")):
        assert mine == int(re.search(r"^#define %s\s+(\d+)" % name, src, re.M).group(1)), name
    assert _lib.MCTS_WIDE_LDS_BYTES == 8 * 64 * 8 + 256 * 8 + _lib.MCTS_WIDE_MAX_LEAVES * (
        4 * _lib.MCTS_PATH_ENTRIES + 16 + 4)
    assert 64 * _lib.MCTS_WIDE_MAX_LEAVES == 1024  # the largest block a kernel may have
    # the node, the limits and the statuses are othello_mcts.h's: this header restates none of them
    assert not re.findall(r"^#define OTHU_", src, re.M) and '#include "othello_mcts.h"' in src


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E, OK = _lib.OTH_EINVAL, _lib.OTH_OK
    table = (ctypes.c_float * 8)()
    tp = ctypes.addressof(table)
    M = 1 << 20

    def wide(R=5, L=4, nodes=64, log_table=tp, scratch=None, scratch_bytes=0, n=0, boards=None):
        return lib.othv_mcts_wide(boards, None, R, L, 0.5, log_table, 0, 0, nodes, None, None, None, None, None, None,
                                  None, None, scratch, scratch_bytes, n, None)

    assert wide() == OK  # n == 0: nothing launched
    assert wide(L=0) == E and wide(L=17) == E and wide(L=-1) == E and wide(L=16) == OK and wide(L=1) == OK
    assert wide(R=0) == E and wide(R=-1) == E
    assert wide(R=65536, L=1) == OK and wide(R=65537, L=1) == E  # R L = 65,537
    assert wide(R=4096, L=16) == OK and wide(R=4097, L=16) == E and wide(R=2**31 - 1, L=16) == E
    assert wide(nodes=0) == E and wide(nodes=M + 1) == E and wide(nodes=M) == OK
    assert wide(log_table=None) == E and wide(n=-1) == E
    assert wide(n=1) == E  # no boards, no scratch
    fake = (ctypes.c_uint64 * 8)()
    fp = ctypes.addressof(fake) & ~15
    assert wide(n=1, boards=fp, scratch=None, scratch_bytes=1 << 30) == E
    assert wide(n=1, boards=fp, scratch=fp, scratch_bytes=64 * 32 - 1) == E  # too few bytes
    assert wide(n=1, boards=fp, scratch=fp + 8, scratch_bytes=1 << 30) == E  # not 16-byte aligned
    sb = lib.othv_mcts_wide_scratch_bytes
    assert sb(1, 64, 4) == 64 * 32 and sb(3, 64, 16) == 3 * 64 * 32 and sb(0, 64, 1) == 16
    assert sb(1024, 7, 4) == sb(100000, 7, 4) == 1024 * 7 * 32  # a slab per block, never more than OTHV_MAX_BLOCKS
    assert sb(-1, 64, 4) == E and sb(1, 0, 4) == E and sb(1, M + 1, 4) == E and sb(1, 64, 0) == E and sb(1, 64, 17) == E
    g = lib.othv_mcts_wide_grid
    assert g(0, 4) == 0 and g(-1, 4) == E and g(5, 0) == E and g(5, 17) == E


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mcts(b, t, 5, leaves=4)
    for L in (0, 17, -1):
        with pytest.raises(ValueError, match="leaves must lie"):
            ops.mcts(b, t, 5, leaves=L)
    for R, L in ((0, 4), (65537, 1), (4097, 16)):
        with pytest.raises(ValueError, match="iterations must lie"):
            ops.mcts(b, t, R, leaves=L)
    with pytest.raises(ValueError, match="leaves must lie"):
        engine.Engine(policy="mcts", iterations=8, leaves=17)
    with pytest.raises(ValueError, match="leaves must lie"):
        engine.Engine(policy="mcts", iterations=4097, leaves=16)
    with pytest.raises(ValueError, match="not with reuse"):
        engine.Engine(policy="mcts", iterations=8, leaves=4, reuse=1)
    with pytest.raises(ValueError, match="applies to policy mcts"):
        engine.Engine(policy="greedy", leaves=4)
    eng = engine.Engine(policy="mcts", iterations=8, leaves=4)
    out = []
    assert eng.handle("verbose p", out.append) and out == ["GPU policy=mcts iterations=8 explore=0.5 leaves=4"]


def test_the_kernel_uses_no_scratch_and_the_lds_the_header_states():
    """One kernel of up to sixteen waves a block: the tables, sixteen paths and
    sixteen leaves in LDS, at most 128 VGPRs (four waves a SIMD)."""
    found = codeobj.named(("mcts_wide_rounds",))
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == _lib.MCTS_WIDE_LDS_BYTES, name
        assert k["vgpr_count"] <= 128, name
    print(found)
