"""The budget searches' C-ABI (include/othello_budget.h, othb_*) is declared,
bound and exported as one set beside the others, its argument checks answer
before anything is launched, the Python layers refuse bad arguments before they
touch a device, and its kernels use no scratch and keep the footprint of
search.hip's and play.hip's (CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha")
NAMES = ["othb_play", "othb_play_grid", "othb_search", "othb_search_grid"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_budget_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.BUDGET_HEADER, "othb")
    assert names == NAMES == sorted(_lib.BUDGET_SIGNATURES)
    assert exported("othb") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.BUDGET_SIGNATURES[name][1], name
        assert fn.restype == _lib.BUDGET_SIGNATURES[name][0], name
    for prefix in OTHERS:
        assert not header_functions(_lib.BUDGET_HEADER, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(_lib.BUDGET_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.BUDGET_SIGNATURES[name][1]), name
    # othm_search's arguments with (budget, budgets, order) where node_limit was and depth in front of status
    srch, fixed = _lib.BUDGET_SIGNATURES["othb_search"][1], _lib.SEARCH_SIGNATURES["othm_search"][1]
    assert srch[:4] + srch[7:9] + srch[10:] == fixed[:4] + fixed[5:]
    # otho_play_ordered's with the two budgets after the depths
    play = _lib.BUDGET_SIGNATURES["othb_play"][1]
    assert play[:8] + play[10:] == _lib.ORDER_SIGNATURES["otho_play_ordered"][1]
    # the sets that were there are what they were
    assert exported("othm") == set(_lib.SEARCH_SIGNATURES) and exported("othp") == set(_lib.PLAY_SIGNATURES)
    assert exported("otho") == set(_lib.ORDER_SIGNATURES) and exported("otha") == set(_lib.MOVES_SIGNATURES)
    assert "othb_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E = _lib.OTH_EINVAL
    word = ctypes.c_uint64(0)
    boards = (ctypes.c_uint64 * 2)(0, 0)
    weights = (ctypes.c_int8 * 36)()
    w, b, wt = ctypes.addressof(word), ctypes.addressof(boards), ctypes.addressof(weights)

    def search(max_depth=6, weights=wt, budget=100, budgets=None, order=0, work=w, n=0, bd=b):
        return lib.othb_search(bd, None, max_depth, weights, budget, budgets, order, None, None, None, None, None, work,
                               n, None)

    assert search() == _lib.OTH_OK  # n == 0: nothing launched
    assert search(max_depth=0) == E and search(max_depth=9) == E and search(weights=None) == E
    assert search(budget=0) == E and search(budget=0, budgets=b) == _lib.OTH_OK  # per-position budgets may hold 0
    assert search(order=2) == E and search(order=-1) == E and search(work=None) == E and search(n=-1) == E
    assert search(n=1, bd=None) == E

    def play(da=3, db=3, ba=100, bb=100, exact=0, order=0, ra=0, rb=0, wa=wt, wb=wt, work=w, n=0):
        return lib.othb_play(None, None, 1, 0, wa, wb, da, db, ba, bb, exact, order, ra, rb, 0, 0, None, None, None,
                             None, None, None, None, None, work, n, None)

    assert play() == _lib.OTH_OK
    assert play(da=0) == E and play(db=9) == E and play(ba=0) == E and play(bb=0) == E and play(exact=9) == E
    assert play(order=2) == E and play(ra=-1) == E and play(wa=None) == E and play(work=None) == E and play(n=-1) == E
    assert lib.othb_search_grid(0) == 0 and lib.othb_play_grid(0) == 0
    assert lib.othb_search_grid(-1) == E and lib.othb_play_grid(-1) == E
    assert word.value == 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, env, ops, runner

    b = torch.zeros((3, 2), dtype=torch.int64)  # host tensors: a call that got past the checks would raise otherwise
    t = torch.ones(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.search_budget(b, t, 100)
    with pytest.raises(ValueError, match="budget must be"):
        ops.play(4, 1, depth_a=3, budget=0)
    with pytest.raises(ValueError, match="budget must be"):
        ops.play(4, 1, depth_a=3, budget=(5, 6, 7))
    with pytest.raises(ValueError, match="policy 'search' only"):
        runner.do_matches({}, n=1, policy="eval", budget=100)
    with pytest.raises(ValueError, match="policy search"):
        engine.Engine(policy="eval", nodes=100)
    with pytest.raises(ValueError, match="policy search"):
        engine.Engine(policy="search", depth=6, split=2, nodes=100)
    with pytest.raises(ValueError, match="nodes must lie"):
        engine.Engine(policy="search", depth=6, nodes=0)
    assert ops.BudgetResult._fields == ("value", "best_move", "status", "depth", "nodes")
    assert {"search_budget", "BudgetResult"} <= set(ops.__all__) and callable(env.VecEnv.search_budget)
    # the parameter line: unchanged without a budget, the budget after the depth with one
    w = list(range(36))
    assert runner.hamlet_param_line("H", "search", w, 3, 2) == "H policy=search depth=3 weights=%s solve_empties=2" % w
    assert runner.hamlet_param_line("H", "search", w, 6, 0, 512) == "H policy=search depth=6 nodes=512 weights=%s" % w
    out = []
    engine.Engine(name="H", policy="search", depth=6, nodes=512, weights=w).handle("verbose p", out.append)
    assert out == [runner.hamlet_param_line("H", "search", w, 6, 0, 512)]


def test_the_budget_kernels_use_no_scratch_and_keep_the_searchs_and_the_games_footprint():
    """One-wave blocks with the frames and the widened table(s) in LDS
    (7 x 9 x 64 words + 48 ints, or + 96): search.hip's and play.hip's
    footprint, so eight blocks a CU; registers for two waves per SIMD.
    DESIGN.md §22 has the figures."""
    found = codeobj.named(("budget_deepen", "budget_play", "13search_kernel", "11play_kernel"))
    new = {n: k for n, k in found.items() if "budget_" in n}
    assert len(new) == 4 and len(found) == 6, sorted(found)  # search and games, unordered and ordered; the two models
    for name, k in new.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["vgpr_count"] <= 128, name
        model = [v for n, v in found.items() if n not in new and ("play" in n) == ("play" in name)][0]
        assert k["group_segment_fixed_size"] == model["group_segment_fixed_size"], name
        assert k["group_segment_fixed_size"] == 7 * 9 * 64 * 4 + (96 if "play" in name else 48) * 4, name
    print({n: found[n] for n in sorted(found)})
