"""The C-ABI of the Monte Carlo search trees that persist
(include/othello_mcts_tree.h, othr_*) is declared, bound and exported as one
set beside the others, its constants are the binding's, its argument checks
answer before anything is launched, the Python layers refuse bad arguments
before they touch a device, and its kernels use no scratch and the LDS the
header states (CPU only)."""
import ctypes
import os
import re
import subprocess

import pytest

import codeobj
from subproc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("oth", "oths", "othm", "othp", "otht", "otho", "othe", "othh", "othw", "otha", "othb", "othl", "othx", "othc",
          "othu")
NAMES = ["othr_advance", "othr_init", "othr_rows", "othr_search", "othr_trees_grid", "othr_trees_record_bytes",
         "othr_trees_slab_bytes"]


def header_functions(path, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def header_constant(name, path=None):
    src = open(path or _lib.MCTS_TREE_HEADER).read()
    return eval(re.search(r"^#define %s\s+(\(?[^/\n]+?\)?)\s*(?:/\*.*)?$" % name, src, re.M).group(1).replace("u", ""))


def test_the_header_the_binding_and_the_exports_are_one_set():
    names = header_functions(_lib.MCTS_TREE_HEADER, "othr")
    assert names == NAMES == sorted(_lib.MCTS_TREE_SIGNATURES)
    assert exported("othr") == set(names)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.MCTS_TREE_SIGNATURES[name][1], name
        assert fn.restype == _lib.MCTS_TREE_SIGNATURES[name][0], name
    for prefix in OTHERS:  # the new prefix is nobody else's, and this header declares nothing of theirs
        assert not header_functions(_lib.MCTS_TREE_HEADER, prefix)
    inc = os.path.join(ROOT, "include")
    for other in os.listdir(inc):
        if other != "othello_mcts_tree.h":
            assert not header_functions(os.path.join(inc, other), "othr"), other
    src = re.sub(r"/\*.*?\*/", "", open(_lib.MCTS_TREE_HEADER).read(), flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.MCTS_TREE_SIGNATURES[name][1]), name
    # the sets that were there are what they were
    assert exported("othu") == set(_lib.MCTS_SIGNATURES) and exported("othc") == set(_lib.PERFT_SIGNATURES)
    assert exported("oth") == set(_lib.SIGNATURES)
    assert "othr_*" in open(os.path.join(ROOT, "subproc_amd", "csrc", "exports.map")).read()


def test_the_constants_are_the_headers():
    for mine, name in ((_lib.MCTS_TREE_RECORD_BYTES, "OTHR_RECORD_BYTES"), (_lib.MCTS_TREE_LDS_BYTES, "OTHR_LDS_BYTES"),
                       (_lib.MCTS_TREE_READY, "OTHR_READY"), (_lib.MCTS_TREE_INVALID, "OTHR_INVALID"),
                       (_lib.MCTS_TREE_BADMOVE, "OTHR_BADMOVE"), (_lib.MCTS_TREE_KEEP, "OTHR_KEEP")):
        assert mine == header_constant(name), name
    assert _lib.MCTS_TREE_READY == _lib.MCTS_SEARCHED and _lib.MCTS_TREE_INVALID == _lib.MCTS_INVALID
    assert _lib.MCTS_TREE_KEEP == _lib.MCTS_NO_MOVE and _lib.MCTS_TREE_LDS_BYTES == _lib.MCTS_LDS_BYTES
    # no other header's status shares BADMOVE's value
    assert _lib.MCTS_TREE_BADMOVE not in (_lib.SEARCH_LIMIT, _lib.TREE_NOROOM, _lib.SOLVE_BADWINDOW, _lib.LINE_BADDEPTH,
                                          _lib.PERFT_BADDEPTH)
    # the node the slab is made of is othello_mcts.h's, and this header restates none of its constants
    assert _lib.MCTS_NODE_BYTES == header_constant("OTHU_NODE_BYTES", _lib.MCTS_HEADER) == 32
    assert "OTHU_" not in "".join(re.findall(r"^#define (\w+)", open(_lib.MCTS_TREE_HEADER).read(), re.M))


def test_bad_arguments_are_answered_without_a_launch():
    lib = _lib.load()
    E, OK = _lib.OTH_EINVAL, _lib.OTH_OK
    M = 1 << 20
    table = (ctypes.c_float * 8)()
    tp = ctypes.addressof(table)
    fake = (ctypes.c_uint64 * 8)()
    fp = ctypes.addressof(fake) & ~15
    sb, rb = lib.othr_trees_slab_bytes, lib.othr_trees_record_bytes
    assert sb(1, 64) == 2 * 64 * 32 and sb(3, 7) == 3 * 2 * 7 * 32 and sb(0, 64) == 16 and sb(2, M) == 2 * 2 * 32 * M
    assert sb(100000, 7) == 100000 * 2 * 7 * 32  # a slab per tree, however many
    assert sb(-1, 64) == E and sb(1, 0) == E and sb(1, M + 1) == E
    assert rb(0) == 16 and rb(1) == 32 and rb(1000) == 32000 and rb(-1) == E
    assert lib.othr_trees_grid(0) == 0 and lib.othr_trees_grid(-1) == E

    def trees(n=1, nodes=64, slabs=fp, slab_bytes=1 << 30, records=fp, record_bytes=1 << 30):
        return dict(nodes=nodes, tail=(slabs, slab_bytes, records, record_bytes, n, None))

    def calls(t, boards=fp, move=fp, T=5, log_table=tp):
        rows = (None,) * 11
        return (lib.othr_init(boards, None, None, 0, 0, t["nodes"], *t["tail"]),
                lib.othr_search(T, None, 0.5, log_table, 0, t["nodes"], *rows, *t["tail"]),
                lib.othr_rows(t["nodes"], *rows, *t["tail"]),
                lib.othr_advance(move, 1, t["nodes"], None, *t["tail"]))

    assert calls(trees(n=0)) == (OK,) * 4  # nothing launched
    assert calls(trees(n=0, slabs=None, records=None)) == (OK,) * 4
    for bad in (trees(n=-1), trees(nodes=0), trees(nodes=M + 1), trees(slabs=None), trees(records=None),
                trees(slabs=fp + 8), trees(records=fp + 4), trees(slab_bytes=2 * 64 * 32 - 1),
                trees(record_bytes=31), trees(n=3, slab_bytes=5 * 64 * 32), trees(n=3, record_bytes=95)):
        assert calls(bad) == (E,) * 4, bad
    assert calls(trees(n=0), T=-1)[1] == E and calls(trees(n=0), T=65537)[1] == E
    assert calls(trees(n=0), T=0)[1] == OK and calls(trees(n=0), T=65536)[1] == OK
    assert calls(trees(n=0), log_table=None)[1] == E
    assert lib.othr_init(None, None, None, 0, 0, 64, *trees()["tail"]) == E  # no boards with n > 0
    assert lib.othr_advance(None, 1, 64, None, *trees()["tail"]) == E  # no moves with n > 0


def test_python_layers_refuse_bad_arguments_before_they_touch_a_device():
    import torch

    from subproc_amd import engine, env, ops, runner

    assert ops.MctsTreesResult._fields == ops.MctsResult._fields + ("ran", "root_boards", "root_turn")
    assert ops.MctsPlayResult._fields[:6] == ops.RunnerResult._fields == ops.PlayResult._fields[:6]
    assert ops.MctsPlayResult._fields[6:] == ("status", "root_visits")
    assert {"MctsTrees", "MctsTreesResult", "mcts_play", "MctsPlayResult"} <= set(ops.__all__)
    assert callable(env.VecEnv.mcts_trees)
    for kw in (dict(n=-1, max_nodes=8), dict(n=1, max_nodes=0), dict(n=1, max_nodes=(1 << 20) + 1)):
        with pytest.raises(ValueError, match="must"):
            ops.MctsTrees(**kw)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.MctsTrees(1, 8, device="cpu")
    # mcts_play: every check comes before the first device call (the arguments here are host tensors or none)
    for bad in (0, 65537, (1, 2, 3), (0, 5), (5, 65537)):
        with pytest.raises(ValueError, match="iterations must"):
            ops.mcts_play(2, 0, iterations=bad)
    for bad in (float("nan"), (0.5, float("inf")), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="explore must"):
            ops.mcts_play(2, 0, iterations=4, explore=bad)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_nodes must lie"):
            ops.mcts_play(2, 0, iterations=4, max_nodes=bad)
    with pytest.raises(ValueError, match="n must be"):
        ops.mcts_play(-1, 0, iterations=4)
    with pytest.raises(ValueError, match="poll"):
        ops.mcts_play(2, 0, iterations=4, poll=0)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.mcts_play(2, 0, iterations=4, device="cpu")
    b = torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="start must have n rows"):
        ops.mcts_play(2, 0, iterations=4, start=b)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mcts_play(3, 0, iterations=4, start=b)
    with pytest.raises(ValueError, match="start_turn needs start"):
        ops.mcts_play(3, 0, iterations=4, start_turn=torch.ones(3, dtype=torch.uint8), device="cpu")
    # runner: the keywords of the eval searches do not belong to policy mcts, nor mcts's to the others
    with pytest.raises(ValueError, match="needs iterations"):
        runner.do_matches({}, policy="mcts")
    for kw in (dict(depth=2), dict(exact_empties=4), dict(order=1), dict(budget=100), dict(solve_empties=8),
               dict(weights_a=[0] * 36), dict(weights_b=[0] * 36)):
        with pytest.raises(ValueError, match="belong to the eval searches"):
            runner.do_matches({}, policy="mcts", iterations=8, **kw)
    with pytest.raises(ValueError, match="no random plies"):
        runner.do_matches({"proc_n_rand_hands_for_a": 2}, policy="mcts", iterations=8)
    with pytest.raises(ValueError, match="no random plies"):
        runner.do_matches({"proc_randomize_black_white": 1}, policy="mcts", iterations=8)
    with pytest.raises(ValueError, match="apply to policy 'mcts' only"):
        runner.do_matches({}, policy="eval", iterations=8)
    # the engine
    with pytest.raises(ValueError, match="reuse applies to policy mcts"):
        engine.Engine(policy="greedy", reuse=1)
    with pytest.raises(ValueError, match="reuse must be"):
        engine.Engine(policy="mcts", iterations=8, reuse=2)
    out = []
    assert engine.Engine(policy="mcts", iterations=8, reuse=1).handle("verbose p", out.append)
    assert engine.Engine(policy="mcts", iterations=8).handle("verbose p", out.append)
    assert out == ["GPU policy=mcts iterations=8 explore=0.5 reuse=1", "GPU policy=mcts iterations=8 explore=0.5"]


def test_the_kernels_use_no_scratch_and_the_lds_the_header_states():
    """Four kernels: the search (the tables and the path in LDS, as mcts.hip's:
    6,672 B, at most 128 VGPRs), the rows, the advance and the init (no LDS).  DESIGN.md §29 has the figures."""
    found = codeobj.named(("tree_walk_kernel", "tree_advance_kernel", "tree_init_kernel"))
    assert len(found) == 4, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0, name
        assert k["vgpr_count"] <= 128, name
        if "tree_walk_kernelILb1E" in name:
            assert k["group_segment_fixed_size"] == _lib.MCTS_TREE_LDS_BYTES, name
        else:
            assert k["group_segment_fixed_size"] == 0, name
    assert sum("tree_walk_kernelILb1E" in name for name in found) == 1
    assert len(codeobj.named(("mcts_kernel",))) == 1  # and mcts.hip's is still the only one of its name
    print(found)
