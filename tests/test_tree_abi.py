"""The split search's C-ABI is declared, bound and exported as one set (otht_*)
beside the oth_*, oths_*, othm_* and othp_* sets, its constants match the
binding, and its task kernel keeps the stack in LDS at the search's own
occupancy (CPU only; resources, not instructions)."""
import ctypes
import re
import subprocess

import codeobj
from subproc_amd import _lib


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_tree_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.TREE_HEADER, "otht")
    assert names == ["otht_scratch_bytes", "otht_search", "otht_search_grid"]
    assert names == sorted(_lib.TREE_SIGNATURES)
    assert exported("otht") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.TREE_SIGNATURES[name][1], name
        assert fn.restype == _lib.TREE_SIGNATURES[name][0], name
    # disjoint from the four other sets, in the bindings and in the headers
    others = {**_lib.SIGNATURES, **_lib.SOLVE_SIGNATURES, **_lib.SEARCH_SIGNATURES, **_lib.PLAY_SIGNATURES}
    assert not any(n.startswith("otht_") for n in others)
    for h in (_lib.HEADER, _lib.SOLVE_HEADER, _lib.SEARCH_HEADER, _lib.PLAY_HEADER):
        assert "otht_" not in open(h).read(), h
    for prefix in ("oth", "oths", "othm", "othp"):
        assert not header_functions(_lib.TREE_HEADER, prefix)
    # the search's own set is what it was
    assert exported("othm") == {"othm_search", "othm_search_grid"}


def test_header_constants_match_the_binding():
    src = open(_lib.TREE_HEADER).read()

    def const(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, src).group(1))

    assert const("OTHT_MAX_SPLIT") == _lib.TREE_MAX_SPLIT == 4
    assert const("OTHT_NOROOM") == _lib.TREE_NOROOM == 4
    assert const("OTHT_MIN_NODES") == _lib.TREE_MIN_NODES == 64
    # a status of its own, beside the search's three
    assert _lib.TREE_NOROOM not in (_lib.SEARCH_SEARCHED, _lib.SEARCH_INVALID, _lib.SEARCH_LIMIT)
    # the root's children always fit the smallest slab
    assert 1 + 33 <= _lib.TREE_MIN_NODES <= _lib.TREE_DEFAULT_NODES


def test_scratch_bytes_needs_no_device():
    lib = _lib.load()
    assert lib.otht_scratch_bytes(0, 64) >= 0
    one = lib.otht_scratch_bytes(1, 64)
    assert one >= 64 * 48 + 64 * 4
    assert lib.otht_scratch_bytes(2, 64) > one
    assert lib.otht_scratch_bytes(1, 32768) >= 32768 * 52
    assert lib.otht_scratch_bytes(1, 63) == _lib.OTH_EINVAL
    assert lib.otht_scratch_bytes(-1, 64) == _lib.OTH_EINVAL
    assert lib.otht_search_grid(0) == 0 and lib.otht_search_grid(-1) == _lib.OTH_EINVAL


def test_tree_kernels_are_scratch_free_and_the_task_kernel_fits_eight_blocks():
    """As the search's: no scratch in any of the three kernels, and a task
    kernel whose LDS lets eight one-wave blocks share a CU's 160 KB."""
    found = codeobj.grouped(("task_kernel", "expand_kernel", "prefix_kernel"))
    assert {k: len(v) for k, v in found.items()} == {"task_kernel": 1, "expand_kernel": 1, "prefix_kernel": 1}, found
    for name, (k,) in found.items():
        assert k["private_segment_fixed_size"] == 0, name
    k = found["task_kernel"][0]
    assert k["group_segment_fixed_size"] * 8 <= 160 * 1024
    assert k["vgpr_count"] <= 128  # two waves per SIMD need no more than 256; leave room
