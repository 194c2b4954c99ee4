"""The search self-play's C-ABI is declared, bound and exported as one set
(othp_*) beside the oth_*, oths_* and othm_* sets, and its kernel keeps the
search's resource budget: no scratch, eight one-wave blocks per CU, at most 128
VGPRs (host only)."""
import ctypes
import re
import subprocess

import codeobj
from subproc_amd import _lib


def play_header_functions():
    src = open(_lib.PLAY_HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(othp_\w+)\s*\(", src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_play_header_binding_and_exports_are_one_set():
    names = play_header_functions()
    assert names == ["othp_play", "othp_play_grid"]
    assert names == sorted(_lib.PLAY_SIGNATURES)
    assert exported("othp") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.PLAY_SIGNATURES[name][1], name
    others = {**_lib.SIGNATURES, **_lib.SOLVE_SIGNATURES, **_lib.SEARCH_SIGNATURES}
    assert not any(n.startswith("othp_") for n in others)
    for header in (_lib.HEADER, _lib.SOLVE_HEADER, _lib.SEARCH_HEADER):
        assert "othp_" not in open(header).read()


def test_play_signature_matches_the_header_argument_for_argument():
    """Each parameter of the header's othp_play, by its C type, is the ctypes
    type the binding passes."""
    src = open(_lib.PLAY_HEADER).read()
    params = re.search(r"^int othp_play\((.*?)\);", src, re.M | re.S).group(1)
    ctype = {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}
    want = []
    for p in params.split(","):
        p = " ".join(p.split())
        want.append(ctypes.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]])
    assert want == _lib.PLAY_SIGNATURES["othp_play"][1]
    assert _lib.PLAY_SIGNATURES["othp_play"][0] is ctypes.c_int


def test_header_constants_match_the_binding():
    src = open(_lib.PLAY_HEADER).read()

    def const(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, src).group(1))

    assert const("OTHP_MAX_RANDOM") == _lib.PLAY_MAX_RANDOM == 10
    assert const("OTHP_MAX_PLIES") == _lib.PLAY_MAX_PLIES == 255
    # a game's statuses are the search's, its move record the rollouts'
    assert "OTHM_SEARCHED" in src and "OTHM_INVALID" in src and "OTHM_LIMIT" in src and "OTH_MOVES_STRIDE" in src


def test_play_kernel_is_scratch_free_and_fits_eight_blocks():
    """As the search's: the play kernel is found by its name, once; no scratch
    (the stack is LDS, the game's state registers), an LDS footprint that lets
    eight one-wave blocks share a CU's 160 KB, and at most 128 VGPRs."""
    # the mangled name's length prefix tells play_kernel from replay_kernel
    found = {name: v for name, v in codeobj.kernels().items() if "11play_kernel" in name}
    assert len(found) == 1, found
    # and the names the earlier code-object tests look for do not find it
    assert not any(s in name for name in found for s in ("search_kernel", "solve_kernel", "rollout_kernel"))
    k = next(iter(found.values()))
    print(k)
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] * 8 <= 160 * 1024
    assert k["vgpr_count"] <= 128
