"""The ordered searches' C-ABI (otho_*, include/othello_order.h) is declared,
bound and exported as one set beside the five others, rejects what the
unordered calls reject and every order but 0 and 1 before it touches a device,
its kernels keep the stack in LDS at the unordered kernels' footprint, and the
tie cases the GPU tests rely on do exercise the root tie rule (CPU only)."""
import ctypes
import re
import subprocess

import numpy as np

import codeobj
import order_cases
from subproc_amd import _lib, params

EINVAL = _lib.OTH_EINVAL
NAMES = ["otho_play_ordered", "otho_play_ordered_grid", "otho_search_ordered", "otho_search_ordered_grid",
         "otho_tree_ordered", "otho_tree_ordered_grid"]


def header_functions(path, prefix):
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(%s_\w+)\s*\(" % prefix, src, re.M)))


def exported(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return set(re.findall(r" T (%s_\w+)$" % prefix, out, re.M))


def test_order_header_binding_and_exports_are_one_set():
    names = header_functions(_lib.ORDER_HEADER, "otho")
    assert names == NAMES
    assert names == sorted(_lib.ORDER_SIGNATURES)
    assert exported("otho") == set(names)
    lib = _lib.load()
    for name in names:  # the three *_ordered symbols, and their grids, resolve
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and fn.argtypes == _lib.ORDER_SIGNATURES[name][1], name
        assert fn.restype == _lib.ORDER_SIGNATURES[name][0], name
    # disjoint from the five other sets, in the bindings and in the headers
    others = {**_lib.SIGNATURES, **_lib.SOLVE_SIGNATURES, **_lib.SEARCH_SIGNATURES, **_lib.PLAY_SIGNATURES,
              **_lib.TREE_SIGNATURES}
    assert not any(n.startswith("otho_") for n in others)
    for h in (_lib.HEADER, _lib.SOLVE_HEADER, _lib.SEARCH_HEADER, _lib.PLAY_HEADER, _lib.TREE_HEADER):
        assert "otho_" not in open(h).read(), h
    for prefix in ("oth", "oths", "othm", "othp", "otht"):
        assert not header_functions(_lib.ORDER_HEADER, prefix)
    # an ordered call is the unordered one with `order` inserted
    sig = _lib.ORDER_SIGNATURES
    for ordered, plain, at in (("otho_search_ordered", _lib.SEARCH_SIGNATURES["othm_search"], 3),
                               ("otho_play_ordered", _lib.PLAY_SIGNATURES["othp_play"], 9),
                               ("otho_tree_ordered", _lib.TREE_SIGNATURES["otht_search"], 4)):
        args = list(sig[ordered][1])
        assert args.pop(at) is ctypes.c_int and args == plain[1] and sig[ordered][0] is plain[0]
    src = open(_lib.ORDER_HEADER).read()
    assert int(re.search(r"#define OTHO_MAX_ORDER\s+(\d+)", src).group(1)) == _lib.ORDER_MAX == 1


W8 = np.ascontiguousarray(np.asarray(params.DEFAULT_WEIGHTS, np.int8))
WP = W8.ctypes.data_as(ctypes.c_void_p)
FAKE = ctypes.c_void_p(0x1000)  # a non-NULL pointer no rejected call may follow


def search_call(lib, order=1, depth=3, weights=WP, work=FAKE, boards=FAKE, n=4):
    return lib.otho_search_ordered(boards, None, depth, order, weights, 0, None, None, None, None, work, n, None)


def play_call(lib, order=1, da=2, db=2, exact=0, ra=0, rb=0, wa=WP, wb=WP, work=FAKE, n=4):
    return lib.otho_play_ordered(None, None, 1, 0, wa, wb, da, db, exact, order, ra, rb, 0, 0, None, None, None, None,
                                 None, None, None, None, work, n, None)


def tree_call(lib, order=1, depth=5, split=2, weights=WP, work=FAKE, boards=FAKE, scratch=FAKE, size=1 << 30, npp=64,
              n=4):
    return lib.otho_tree_ordered(boards, None, depth, split, order, weights, 0, None, None, None, None, scratch, size,
                                 npp, work, n, None)


def test_bad_orders_and_bad_arguments_are_einval_without_a_device():
    lib = _lib.load()
    for order in (-1, 2, 3, 255, 1 << 20):
        assert search_call(lib, order=order) == EINVAL
        assert play_call(lib, order=order) == EINVAL
        assert tree_call(lib, order=order) == EINVAL
        assert search_call(lib, order=order, n=0) == EINVAL  # even with nothing to do
        assert lib.otho_search_ordered_grid(1, order) == EINVAL
        assert lib.otho_play_ordered_grid(1, order) == EINVAL
        assert lib.otho_tree_ordered_grid(1, order) == EINVAL
    for order in (0, 1):
        # what othm_search rejects
        for kw in (dict(depth=0), dict(depth=9), dict(depth=-1), dict(weights=None), dict(work=None),
                   dict(boards=None), dict(n=-1)):
            assert search_call(lib, order=order, **kw) == EINVAL, kw
        # what othp_play rejects
        for kw in (dict(da=0), dict(da=9), dict(db=0), dict(db=9), dict(exact=-1), dict(exact=9), dict(ra=-1),
                   dict(rb=-1), dict(wa=None), dict(wb=None), dict(work=None), dict(n=-1)):
            assert play_call(lib, order=order, **kw) == EINVAL, kw
        # what otht_search rejects
        for kw in (dict(split=0), dict(split=5), dict(depth=2, split=2), dict(depth=11, split=2), dict(weights=None),
                   dict(work=None), dict(boards=None), dict(n=-1), dict(npp=63), dict(scratch=None), dict(size=64),
                   dict(scratch=ctypes.c_void_p(0x1004))):
            assert tree_call(lib, order=order, **kw) == EINVAL, kw
        # n == 0: OTH_OK, nothing launched (no pointer is followed)
        assert search_call(lib, order=order, n=0, boards=None) == _lib.OTH_OK
        assert play_call(lib, order=order, n=0) == _lib.OTH_OK
        assert tree_call(lib, order=order, n=0, boards=None, scratch=None, size=0) == _lib.OTH_OK
        assert lib.otho_search_ordered_grid(0, order) == 0 and lib.otho_search_ordered_grid(-1, order) == EINVAL
        assert lib.otho_play_ordered_grid(0, order) == 0 and lib.otho_play_ordered_grid(-1, order) == EINVAL
        assert lib.otho_tree_ordered_grid(0, order) == 0 and lib.otho_tree_ordered_grid(-1, order) == EINVAL


def test_ordered_kernels_keep_the_unordered_kernels_lds_and_use_no_scratch():
    """Only the current frame scores, in registers: the frames keep their 9
    words, so the LDS per block is the unordered kernels' (16,320 B for search
    and tree, 16,512 B for play), none of the searches' eight kernels has
    scratch, and eight one-wave blocks still share a CU."""
    k = codeobj.kernels()

    def one(sub):
        hit = [n for n in k if sub in n]
        assert len(hit) == 1, (sub, hit)
        return k[hit[0]]

    pairs = (("13search_kernel", "21search_ordered_kernel", 16320), ("11play_kernel", "19play_ordered_kernel", 16512),
             ("11task_kernel", "19task_ordered_kernel", 16320))
    for plain, ordered, lds in pairs:
        p, o = one(plain), one(ordered)
        assert p["group_segment_fixed_size"] == o["group_segment_fixed_size"] == lds, (plain, p, o)
        assert o["private_segment_fixed_size"] == 0 and p["private_segment_fixed_size"] == 0
        assert o["group_segment_fixed_size"] * 8 <= 160 * 1024 and o["vgpr_count"] <= 128, (ordered, o)
    family = [n for n in k if re.search(r"\d+(search|play|task|expand|prefix)(_ordered)?_kernelE", n)]
    assert len(family) == 8 and not any(k[n]["private_segment_fixed_size"] for n in family), family


def test_the_tie_cases_exercise_the_root_tie_rule():
    """The root tie rule matters only where the lowest maximiser is in a later
    class than another maximiser (an ordered root meets that one first)."""
    assert order_cases.CLASS_OF[[0, 7, 56, 63]].tolist() == [0] * 4
    assert order_cases.CLASS_OF[[9, 14, 49, 54]].tolist() == [7] * 4
    b, t, v, m, later = order_cases.two_empties()
    assert len(t) == 64 and later.sum() >= 1
    for table, ties in (("default", 167), ("rng7", None)):
        b, t, v, m, later = order_cases.depth1_ties(table)
        assert later.sum() >= 5 and (ties is None or len(t) == ties)
    # and roots where the MOBILITY order (depth 3) meets a higher-square maximiser first
    assert len(order_cases.mobility_ties(3, 1024)[1]) >= 20
