"""Perft's C-ABI (include/othello_perft.h, othc_*) is declared, bound and
exported as one set beside the others, its argument checks answer before
anything is launched, the Python layers refuse bad arguments before they touch
a device, and its kernels use no scratch and the LDS the header states (CPU
only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb", "othl", "othx")
NAMES = ["othc_perft", "othc_perft_grid", "othc_perft_scratch_bytes"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def header_constant(name):
    src = open(_lib.PERFT_HEADER).read()
    return eval(re.search(r"^#define %s\s+(\(?[^/\n]+?\)?)\s*(?:/\*.*)?$" % name, src, re.M).group(1).replace("u", ""))


def test_perft_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.PERFT_HEADER, "othc")
    assert names == NAMES == sorted(_lib.PERFT_SIGNATURES)
    assert exported("othc") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.PERFT_SIGNATURES[name][1], name
        assert fn.restype == _lib.PERFT_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.PERFT_HEADER, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(_lib.PERFT_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.PERFT_SIGNATURES[name][1]), name
    # the sets that were there are what they were
    assert exported("othm") == set(_lib.SEARCH_SIGNATURES) and exported("otha") == set(_lib.MOVES_SIGNATURES)
    assert exported("othx") == set(_lib.PLAY_SOLVE_SIGNATURES) and exported("othl") == set(_lib.LINE_SIGNATURES)
    assert "othc_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_the_constants_are_the_headers():
    for mine, name in ((_lib.PERFT_MAX_DEPTH, "OTHC_MAX_DEPTH"), (_lib.PERFT_MAX_SPLIT, "OTHC_MAX_SPLIT"),
                       (_lib.PERFT_MAX_TASKS, "OTHC_MAX_TASKS"), (_lib.PERFT_ROOT_SLOTS, "OTHC_ROOT_SLOTS"),
                       (_lib.PERFT_COUNTED, "OTHC_COUNTED"), (_lib.PERFT_INVALID, "OTHC_INVALID"),
                       (_lib.PERFT_LIMIT, "OTHC_LIMIT"), (_lib.PERFT_BADDEPTH, "OTHC_BADDEPTH"),
                       (_lib.PERFT_COUNT_LDS_BYTES, "OTHC_COUNT_LDS_BYTES"),
                       (_lib.SOLVE_DEFAULT_NODE_LIMIT, "OTHC_DEFAULT_NODE_LIMIT")):
        assert mine == header_constant(name), name
    assert _lib.PERFT_COUNT_LDS_BYTES == (_lib.PERFT_MAX_DEPTH - 1) * 6 * 64 * 4


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    word = ctypes.c_uint64(0)
    w = ctypes.addressof(word)

    def perft(depth=5, split=0, work=w, n=0):
        return lib.othc_perft(None, None, depth, None, split, 0, None, None, None, None, None, 0, work, n, None)

    assert perft() == _lib.OTH_OK  # n == 0: nothing launched
    assert perft(depth=-1) == E and perft(depth=15) == E and perft(depth=14) == _lib.OTH_OK and perft(depth=0) == 0
    assert perft(split=-1) == E and perft(split=9) == E and perft(split=8) == _lib.OTH_OK
    assert perft(work=None) == E and perft(n=-1) == E and perft(n=(1 << 24) + 1) == E
    assert perft(n=1) == E  # no boards, no scratch
    sizes = [lib.othc_perft_scratch_bytes(n, m) for n, m in ((0, 0), (1, 0), (1, 64), (100, 64), (100, 4096),
                                                             (1 << 24, 1 << 24))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[2] - sizes[1] == 63 * 48  # two lists of 24-byte tasks, never below a task per position
    assert sizes[3] == lib.othc_perft_scratch_bytes(100, 100)
    assert lib.othc_perft_scratch_bytes(-1, 0) == E and lib.othc_perft_scratch_bytes(0, -1) == E
    assert lib.othc_perft_scratch_bytes((1 << 24) + 1, 0) == E and lib.othc_perft_scratch_bytes(1, (1 << 24) + 1) == E
    assert lib.othc_perft_grid(0) == 0 and lib.othc_perft_grid(-1) == E
    assert word.value == 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, env, ops

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.perft(b, t, 5)
    assert ops.PerftResult._fields == ("leaves", "divide", "status", "nodes")
    assert {"perft", "PerftResult"} <= set(ops.__all__) and callable(env.VecEnv.perft)
    out = []
    eng = engine.Engine()
    for cmd in ("perft", "perft x", "perft -1", "perft 15", "perft 3 4"):
        assert eng.handle(cmd, out.append)
    assert out == ["perft unavailable"] * 5


def test_the_perft_kernels_use_no_scratch_and_the_count_kernel_the_lds_the_header_states():
    """The count kernel is a one-wave block with 13 frames of 6 words per lane
    in LDS, 19,968 B: eight blocks a CU, as the search kernels.  DESIGN.md §27
    has the figures."""
    found = codeobj.named(("perft_roots", "perft_expand", "perft_count_kernel", "perft_finish"))
    assert len(found) == 4, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == (_lib.PERFT_COUNT_LDS_BYTES if "count" in name else 0), name
        assert k["vgpr_count"] <= 128, name
    assert 8 * _lib.PERFT_COUNT_LDS_BYTES <= 160 * 1024
    print({n: found[n] for n in sorted(found)})
