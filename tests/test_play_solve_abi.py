"""The C-ABI of the search self-play with the exact solver's endgame
(include/othello_play_solve.h, othx_*) is declared, bound and exported as one
set beside the others, its argument checks answer before anything is launched
(for n == 0 too), the Python layers refuse bad arguments before they touch a
device, and its kernels use no scratch and have the LDS DESIGN.md §25 states
(CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb", "othl")
NAMES = ["othx_play", "othx_play_grid", "othx_scratch_bytes"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.PLAY_SOLVE_HEADER, "othx")
    assert names == NAMES == sorted(_lib.PLAY_SOLVE_SIGNATURES)
    assert exported("othx") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.PLAY_SOLVE_SIGNATURES[name][1], name
        assert fn.restype == _lib.PLAY_SOLVE_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.PLAY_SOLVE_HEADER, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(_lib.PLAY_SOLVE_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.PLAY_SOLVE_SIGNATURES[name][1]), name
    # othb_play's arguments with scratch, scratch_bytes in front of work
    play, budget = _lib.PLAY_SOLVE_SIGNATURES["othx_play"][1], _lib.BUDGET_SIGNATURES["othb_play"][1]
    assert play[:24] + play[26:] == budget and play[24:26] == [ctypes.c_void_p, ctypes.c_int64]
    # the sets that were there are what they were
    assert exported("othp") == set(_lib.PLAY_SIGNATURES) == {"othp_play", "othp_play_grid"}
    assert exported("otho") == set(_lib.ORDER_SIGNATURES) and exported("othb") == set(_lib.BUDGET_SIGNATURES)
    assert exported("oths") == set(_lib.SOLVE_SIGNATURES) and exported("othl") == set(_lib.LINE_SIGNATURES)
    assert exported("othm") == set(_lib.SEARCH_SIGNATURES) and exported("otha") == set(_lib.MOVES_SIGNATURES)
    assert "othx_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_scratch_bytes_are_the_documented_ones():
    lib = _lib.load()
    head = open(_lib.PLAY_SOLVE_HEADER).read()
    counter = int(re.search(r"#define OTHX_COUNTER_BYTES (\d+)", head).group(1))
    parked = int(re.search(r"#define OTHX_PARKED_BYTES (\d+)", head).group(1))
    assert (counter, parked) == (_lib.PLAY_SOLVE_COUNTER_BYTES, _lib.PLAY_SOLVE_PARKED_BYTES) == (16, 48)
    sizes = [lib.othx_scratch_bytes(n) for n in (0, 1, 2, 63, 64, 65, 4133, 1 << 20, 1 << 40)]
    assert sizes == [counter + parked * n for n in (0, 1, 2, 63, 64, 65, 4133, 1 << 20, 1 << 40)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert lib.othx_scratch_bytes(-1) == _lib.OTH_EINVAL and lib.othx_scratch_bytes(2**63 - 1) == _lib.OTH_EINVAL


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    word = ctypes.c_uint64(0)
    weights = (ctypes.c_int8 * 36)()
    room = (ctypes.c_uint64 * 16)()  # 128 bytes, 16-byte aligned below
    w, wt = ctypes.addressof(word), ctypes.addressof(weights)
    sc = (ctypes.addressof(room) + 15) & ~15

    def play(da=3, db=3, ba=0, bb=0, zone=10, order=0, ra=0, rb=0, wa=wt, wb=wt, scratch=sc, size=64, work=w, n=0):
        return lib.othx_play(None, None, 1, 0, wa, wb, da, db, ba, bb, zone, order, ra, rb, 0, 0, None, None, None,
                             None, None, None, None, None, scratch, size, work, n, None)

    assert play() == _lib.OTH_OK and play(ba=5, bb=7) == _lib.OTH_OK  # n == 0: nothing launched
    assert play(zone=1) == _lib.OTH_OK and play(zone=12) == _lib.OTH_OK and play(size=16) == _lib.OTH_OK
    assert play(da=0) == E and play(db=9) == E and play(order=2) == E and play(order=-1) == E
    assert play(zone=0) == E and play(zone=13) == E and play(zone=-1) == E
    assert play(ba=5, bb=0) == E and play(ba=0, bb=5) == E  # one budget zero, the other not
    assert play(ra=-1) == E and play(rb=-1) == E and play(wa=None) == E and play(wb=None) == E
    assert play(work=None) == E and play(n=-1) == E
    # the scratch: NULL, misaligned, too small -- for n == 0 too, and before any launch for n > 0
    assert play(scratch=None) == E and play(scratch=sc + 8) == E and play(size=15) == E
    assert play(n=1, size=63) == E and play(n=1, scratch=None) == E and play(n=2, size=64) == E
    assert lib.othx_play_grid(0, 0, 0) == 0 and lib.othx_play_grid(0, 1, 1) == 0
    assert lib.othx_play_grid(-1, 0, 0) == E and lib.othx_play_grid(4, 2, 0) == E and lib.othx_play_grid(4, 0, 2) == E
    assert lib.othx_play_grid(4, -1, 0) == E and lib.othx_play_grid(4, 0, -1) == E
    assert word.value == 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import inspect

    from subproc_amd import ops, runner

    assert inspect.signature(ops.play).parameters["solve_empties"].default == 0
    assert inspect.signature(runner.do_matches).parameters["solve_empties"].default == 0
    for bad in (-1, 13, 100):
        with pytest.raises(ValueError, match="solve_empties must lie in 0..12"):
            ops.play(4, 1, depth_a=3, solve_empties=bad, device="not a device")
    with pytest.raises(ValueError, match="only one of the two"):
        ops.play(4, 1, depth_a=3, exact_empties=4, solve_empties=9, device="not a device")
    with pytest.raises(ValueError, match="budget must be"):
        ops.play(4, 1, depth_a=3, budget=0, solve_empties=9, device="not a device")
    with pytest.raises(ValueError, match="policy 'search' only"):
        runner.do_matches({}, n=1, policy="eval", solve_empties=9)
    with pytest.raises(ValueError, match="solve_empties must lie"):
        runner.do_matches({}, n=1, policy="search", depth=2, solve_empties=13, device="not a device")
    # the parameter line: the default text unchanged, E after the budget and the weights as the engine's
    w = list(range(36))
    assert runner.hamlet_param_line("H", "search", w, 3) == "H policy=search depth=3 weights=%s" % w
    assert (runner.hamlet_param_line("H", "search", w, 6, 11, 512)
            == "H policy=search depth=6 nodes=512 weights=%s solve_empties=11" % w)


def test_the_kernels_use_no_scratch_and_have_the_stated_lds():
    """One-wave blocks.  The first phase's four kernels keep play.hip's footprint (7 x 9 x 64 words of search
    frames + the two widened tables): eight blocks a CU.  The second phase's has the solver's frames and
    nothing else (11 x 7 x 64 words = 19,712 B): eight blocks in a CU's 160 KB, two waves per SIMD, for which
    128 VGPRs would already do.  DESIGN.md §25 has the figures."""
    found = codeobj.named(("park_fixed_games", "park_ordered_games", "park_budget_games",
                           "park_budget_ordered_games", "finish_parked_games", "11play_kernel", "line_exact_walk"))
    assert len(found) == 7, sorted(found)
    model = [v for n, v in found.items() if "11play_kernel" in n][0]
    walk = [v for n, v in found.items() if "line_exact_walk" in n][0]
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["vgpr_count"] <= 128, name
        if "park_" in name:
            assert k["group_segment_fixed_size"] == model["group_segment_fixed_size"] == (7 * 9 * 64 + 96) * 4, name
        if "finish_parked" in name:
            assert k["group_segment_fixed_size"] == walk["group_segment_fixed_size"] == 11 * 7 * 64 * 4, name
            assert 8 * k["group_segment_fixed_size"] <= 160 * 1024 < 9 * k["group_segment_fixed_size"]
    print({n: found[n] for n in sorted(found)})
