"""ctypes binding of the HIP C-ABI (include/othello.h -> lib/libsubproc_amd_hip.so).

There is no CPU fallback: if the library is missing or fails to load, every
product entry point raises :class:`OthelloLibraryError`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsubproc_amd_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello.h")
SOLVE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_solve.h")
SEARCH_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_search.h")
PLAY_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_play.h")
TREE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_tree.h")
ORDER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_order.h")
SOLVE_TREE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_solve_tree.h")
SOLVE_HASH_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_solve_hash.h")
SOLVE_WINDOW_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_solve_window.h")
MOVES_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_moves.h")
BUDGET_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_budget.h")
LINE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_line.h")
PLAY_SOLVE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_play_solve.h")
PERFT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_perft.h")
MCTS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_mcts.h")
MCTS_TREE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_mcts_tree.h")
MCTS_WIDE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "othello_mcts_wide.h")

OTH_OK = 0
OTH_EINVAL = -1000
BLACK, WHITE, PASS = 1, 2, 64
HIST_BINS = 133
MOVES_STRIDE = 128
POS_STRIDE = 129
BOOK_LINE = 67
N_FEATURES = 10
POLICY_RANDOM, POLICY_GREEDY, POLICY_EVAL = 0, 1, 2
EVAL_PHASES, EVAL_FEATURES, EVAL_WEIGHTS = 4, 9, 36
TD_KEY_BITS = 43
TD_SKEY_BITS = 36         # include/othello.h packed update words: the sort key's bits
TD_PACK_TURN_SHIFT = 36
TD_PACK_VALUE_SHIFT = 56
TD_FIT_BLOCKS, TD_FIT_COLS = 1024, 64
SOLVE_MAX_EMPTIES = 12    # include/othello_solve.h
SOLVE_SKIPPED, SOLVE_SOLVED, SOLVE_INVALID, SOLVE_LIMIT = 0, 1, 2, 3
SOLVE_NO_MOVE = 255
SOLVE_DEFAULT_NODE_LIMIT = 1 << 28
SEARCH_MAX_DEPTH = 8      # include/othello_search.h
SEARCH_TERMINAL_SCALE = 1 << 17
SEARCH_SEARCHED, SEARCH_INVALID, SEARCH_LIMIT = 1, 2, 3
SEARCH_NO_MOVE = 255
SEARCH_DEFAULT_NODE_LIMIT = 1 << 28
PLAY_MAX_RANDOM = 10      # include/othello_play.h
PLAY_MAX_PLIES = 255
TREE_MAX_SPLIT = 4        # include/othello_tree.h
TREE_NOROOM = 4
TREE_MIN_NODES = 64
TREE_DEFAULT_NODES = 32768
ORDER_MAX = 1             # include/othello_order.h
SOLVE_TREE_MAX_EMPTIES = 16  # include/othello_solve_tree.h
SOLVE_TREE_NOROOM = 4
SOLVE_TREE_MIN_NODES = 64
SOLVE_TREE_DEFAULT_NODES = 65536
SOLVE_HASH_MIN_BITS, SOLVE_HASH_MAX_BITS = 4, 26  # include/othello_solve_hash.h
SOLVE_HASH_ENTRY_BYTES = 32
SOLVE_HASH_MIN_EMPTIES_LO, SOLVE_HASH_MIN_EMPTIES_HI = 1, 12
SOLVE_HASH_DEFAULT_MIN_EMPTIES = 8
SOLVE_BADWINDOW = 5          # include/othello_solve.h, set by the calls of include/othello_solve_window.h
SOLVE_ALPHA_MIN, SOLVE_BETA_MAX = -65, 65
MOVES_NOT_A_MOVE, MOVES_UNKNOWN = -128, -127  # include/othello_moves.h: the exact calls' int8 rows
MOVES_NOT_A_MOVE32, MOVES_UNKNOWN32 = -2**31, -2**31 + 1  # the search's int32 rows
MOVES_SEARCH_SLOTS = 64
LINE_STRIDE = 32             # include/othello_line.h
LINE_BADDEPTH = 6
PLAY_SOLVE_COUNTER_BYTES, PLAY_SOLVE_PARKED_BYTES = 16, 48  # include/othello_play_solve.h
PERFT_MAX_DEPTH, PERFT_MAX_SPLIT = 14, 8  # include/othello_perft.h
PERFT_MAX_TASKS, PERFT_ROOT_SLOTS = 1 << 24, 64
PERFT_COUNTED, PERFT_INVALID, PERFT_LIMIT, PERFT_BADDEPTH = 1, 2, 3, 7
PERFT_COUNT_LDS_BYTES = 19968
MCTS_MAX_ITERATIONS, MCTS_MAX_NODES = 65536, 1 << 20  # include/othello_mcts.h
MCTS_MAX_BLOCKS, MCTS_NODE_BYTES, MCTS_PATH_ENTRIES, MCTS_LDS_BYTES = 4096, 32, 132, 6672
MCTS_SEARCHED, MCTS_INVALID, MCTS_NO_MOVE = 1, 2, 255
MCTS_TREE_RECORD_BYTES, MCTS_TREE_LDS_BYTES = 32, 6672  # include/othello_mcts_tree.h
MCTS_TREE_READY, MCTS_TREE_INVALID, MCTS_TREE_BADMOVE, MCTS_TREE_KEEP = 1, 2, 8, 255
MCTS_WIDE_MAX_LEAVES, MCTS_WIDE_MAX_BLOCKS, MCTS_WIDE_LDS_BYTES = 16, 1024, 14912  # include/othello_mcts_wide.h

# name -> (restype, argtypes); must match include/othello.h exactly
_P, _I64, _U64, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int
SIGNATURES = {
    "oth_version": (ctypes.c_char_p, []),
    "oth_reset": (_I, [_P, _P, _P, _I64, _P]),
    "oth_legal": (_I, [_P, _P, _P, _I64, _P]),
    "oth_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_result": (_I, [_P, _P, _P, _P, _P, _I64, _P]),
    "oth_hands": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_rollout": (_I, [_P, _P, _U64, _U64, _I, _I, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_sample_midgame": (_I, [_U64, _U64, _P, _P, _P, _P, _I64, _P]),
    "oth_replay": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_replay_rows": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_book_text": (_I, [_P, _P, _I64, _P, _P]),
    "oth_book_parse": (_I, [_P, _I64, _P, _P, _I64, _P]),
    "oth_features": (_I, [_P, _P, _P, _I64, _P]),
    "oth_rollout_eval": (_I, [_P, _P, _U64, _U64, _I, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_rollout_match": (_I, [_P, _P, _U64, _U64, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_rollout_runner": (_I, [_P, _P, _U64, _U64, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_eval": (_I, [_P, _P, _P, _P, _I64, _P]),
    "oth_td_updates": (_I, [_P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_td_updates_rows": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_td_updates_records": (_I, [_P, _P, _P, _P, _P, _P, _I64, _P]),
    "oth_td_ema": (_I, [_P, _P, _P, ctypes.c_double, ctypes.c_double, _P, _I64, _P]),
    "oth_td_new_before": (_I, [_P, _I64, _P, _P, _P, _P]),
    "oth_td_segments": (_I, [_P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P]),
    "oth_td_segments_words": (_I, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "oth_td_ema_split": (_I, [_P, _P, _P, ctypes.c_double, ctypes.c_double, _P, _I64, _I64, _P, _I64, _I64, _P, _P,
                              _P]),
    "oth_td_sort_pairs": (_I, [_P, _P, _P, _P, _I64, _P, _P, _P]),
    "oth_rollout_grid": (_I, [_I, _I64]),
    "oth_td_updates_packed": (_I, [_P, _P, _P, _P, _P, _I64, _P]),
    "oth_td_sort_packed": (_I, [_P, _P, _I64, _P, _P, _P]),
    "oth_td_sort_unpack": (_I, [_P, _P, _P, _P, _I64, _P, _P, _P]),
    "oth_td_unpack": (_I, [_P, _P, _P, _P, _I64, _P]),
    "oth_td_word_errors": (_I, [_P, _I, _P]),
    "oth_td_merge": (_I, [_P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "oth_td_lookup": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "oth_td_lookup_dev": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "oth_td_merge_after_lookup": (_I, [_P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P]),
    "oth_td_fit_moments": (_I, [_P, _P, _I64, _P, _P, _P]),
}

# the endgame solver, include/othello_solve.h (no host twin: its own prefix)
SOLVE_SIGNATURES = {
    "oths_solve": (_I, [_P, _P, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, _P]),
    "oths_solve_grid": (_I, [_I64]),
}

# the depth-limited search, include/othello_search.h (its own prefix likewise)
SEARCH_SIGNATURES = {
    "othm_search": (_I, [_P, _P, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, _P]),
    "othm_search_grid": (_I, [_I64]),
}

# search self-play, include/othello_play.h (its own prefix likewise)
PLAY_SIGNATURES = {
    "othp_play": (_I, [_P, _P, _U64, _U64, _P, _P, _I, _I, _I, _I, _I, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P,
                       _P, _P, _I64, _P]),
    "othp_play_grid": (_I, [_I64]),
}

# the split search, include/othello_tree.h (its own prefix likewise)
TREE_SIGNATURES = {
    "otht_search": (_I, [_P, _P, _I, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, ctypes.c_int32, _P, _I64, _P]),
    "otht_scratch_bytes": (_I64, [_I64, ctypes.c_int32]),
    "otht_search_grid": (_I, [_I64]),
}

# the ordered searches, include/othello_order.h (its own prefix likewise): the
# three calls above with `order` after depth / split / exact_empties
ORDER_SIGNATURES = {
    "otho_search_ordered": (_I, [_P, _P, _I, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, _P]),
    "otho_play_ordered": (_I, [_P, _P, _U64, _U64, _P, _P, _I, _I, _I, _I, _I, _I, _I, ctypes.c_uint32, _P, _P, _P, _P,
                               _P, _P, _P, _P, _P, _I64, _P]),
    "otho_tree_ordered": (_I, [_P, _P, _I, _I, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, ctypes.c_int32, _P,
                               _I64, _P]),
    "otho_search_ordered_grid": (_I, [_I64, _I]),
    "otho_play_ordered_grid": (_I, [_I64, _I]),
    "otho_tree_ordered_grid": (_I, [_I64, _I]),
}

# the split endgame solver, include/othello_solve_tree.h (its own prefix likewise)
SOLVE_TREE_SIGNATURES = {
    "othe_solve": (_I, [_P, _P, _I, _I, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, ctypes.c_int32, _P, _I64, _P]),
    "othe_scratch_bytes": (_I64, [_I64, ctypes.c_int32]),
    "othe_solve_grid": (_I, [_I64]),
}

# the split solver with a transposition table, include/othello_solve_hash.h (its own prefix likewise):
# othe_solve's arguments with hash_bits, hash_min_empties, table, table_bytes in front of the stream
SOLVE_HASH_SIGNATURES = {
    "othh_solve_hashed": (_I, [_P, _P, _I, _I, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, ctypes.c_int32, _P, _I64,
                               _I, _I, _P, _I64, _P]),
    "othh_hash_bytes": (_I64, [_I]),
}

# the exact solvers with a root window, include/othello_solve_window.h (its own prefix likewise): oths_solve's
# arguments with alpha, beta after turn; othh_solve_hashed's with alpha, beta in front of hash_bits
SOLVE_WINDOW_SIGNATURES = {
    "othw_solve": (_I, [_P, _P, _P, _P, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, _P]),
    "othw_solve_split": (_I, [_P, _P, _I, _I, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, ctypes.c_int32, _P, _I64,
                              _P, _P, _I, _I, _P, _I64, _P]),
}

# the value of every root move, include/othello_moves.h (its own prefix likewise)
MOVES_SIGNATURES = {
    "otha_solve_moves": (_I, [_P, _P, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "otha_solve_moves_scratch_bytes": (_I64, [_I64, _I]),
    "otha_solve_moves_split": (_I, [_P, _P, _I, _I, _I, ctypes.c_uint32, ctypes.c_int32, _I, _I, _P, _I64, _P, _P, _P,
                                    _P, _P, _P, _I64, _P, _I64, _P]),
    "otha_solve_moves_split_scratch_bytes": (_I64, [_I64, _I, ctypes.c_int32]),
    "otha_search_moves": (_I, [_P, _P, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "otha_search_moves_scratch_bytes": (_I64, [_I64]),
}

# the searches by node budget, include/othello_budget.h (its own prefix likewise): othm_search's arguments with
# budget, budgets, order in place of node_limit and depth in front of status; otho_play_ordered's with budget_a,
# budget_b after the depths
BUDGET_SIGNATURES = {
    "othb_search": (_I, [_P, _P, _I, _P, ctypes.c_uint32, _P, _I, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "othb_play": (_I, [_P, _P, _U64, _U64, _P, _P, _I, _I, ctypes.c_uint32, ctypes.c_uint32, _I, _I, _I, _I, _I,
                       ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "othb_search_grid": (_I, [_I64]),
    "othb_play_grid": (_I, [_I64]),
}

# the principal variation, include/othello_line.h (its own prefix likewise): oths_solve's / otho_search_ordered's
# arguments with line, length in front of value and end_boards, end_turn in front of work; the search's with
# depth_per_position after depth
LINE_SIGNATURES = {
    "othl_solve_line": (_I, [_P, _P, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "othl_search_line": (_I, [_P, _P, _I, _P, _I, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "othl_solve_line_grid": (_I, [_I64]),
    "othl_search_line_grid": (_I, [_I64, _I]),
}

# search self-play with the exact solver's endgame, include/othello_play_solve.h (its own prefix likewise):
# othb_play's arguments with solve_empties where exact_empties stands and scratch, scratch_bytes in front of work
PLAY_SOLVE_SIGNATURES = {
    "othx_play": (_I, [_P, _P, _U64, _U64, _P, _P, _I, _I, ctypes.c_uint32, ctypes.c_uint32, _I, _I, _I, _I, _I,
                       ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "othx_scratch_bytes": (_I64, [_I64]),
    "othx_play_grid": (_I, [_I64, _I, _I]),
}

# perft, include/othello_perft.h (its own prefix likewise)
PERFT_SIGNATURES = {
    "othc_perft": (_I, [_P, _P, _I, _P, _I, ctypes.c_uint32, _P, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "othc_perft_scratch_bytes": (_I64, [_I64, _I64]),
    "othc_perft_grid": (_I, [_I64]),
}

# the Monte Carlo tree search, include/othello_mcts.h (its own prefix likewise)
MCTS_SIGNATURES = {
    "othu_mcts": (_I, [_P, _P, _I, ctypes.c_float, _P, _U64, _U64, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64,
                       _P]),
    "othu_mcts_scratch_bytes": (_I64, [_I64, _I]),
    "othu_mcts_grid": (_I, [_I64]),
}

# the Monte Carlo search trees that persist, include/othello_mcts_tree.h (its own prefix likewise): every call ends
# in slabs, slab_bytes, records, record_bytes, n, stream
_TREES = [_P, _I64, _P, _I64, _I64, _P]
_TREE_ROWS = [_P] * 11
MCTS_TREE_SIGNATURES = {
    "othr_trees_slab_bytes": (_I64, [_I64, _I]),
    "othr_trees_record_bytes": (_I64, [_I64]),
    "othr_trees_grid": (_I, [_I64]),
    "othr_init": (_I, [_P, _P, _P, _U64, _U64, _I, *_TREES]),
    "othr_search": (_I, [_I, _P, ctypes.c_float, _P, _U64, _I, *_TREE_ROWS, *_TREES]),
    "othr_rows": (_I, [_I, *_TREE_ROWS, *_TREES]),
    "othr_advance": (_I, [_P, _I, _I, _P, *_TREES]),
}

# the wide Monte Carlo tree search, include/othello_mcts_wide.h (its own prefix likewise): othu_mcts's arguments with
# `leaves` after `iterations`
MCTS_WIDE_SIGNATURES = {
    "othv_mcts_wide": (_I, [_P, _P, _I, _I, ctypes.c_float, _P, _U64, _U64, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                            _I64, _I64, _P]),
    "othv_mcts_wide_scratch_bytes": (_I64, [_I64, _I, _I]),
    "othv_mcts_wide_grid": (_I, [_I64, _I]),
}


class OthelloLibraryError(RuntimeError):
    pass


class OthelloCallError(RuntimeError):
    pass


_lib = None


def load():
    """Load the HIP library (once).  torch is imported first so that the HIP
    runtime the library binds to (soname libamdhip64.so.7) is the one torch
    already loaded: device pointers and hipStream_t handles from torch are then
    valid in the library."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (runtime sharing, see docstring)

    if not os.path.exists(LIB_PATH):
        raise OthelloLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise OthelloLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in {**SIGNATURES, **SOLVE_SIGNATURES, **SEARCH_SIGNATURES, **PLAY_SIGNATURES,
                              **TREE_SIGNATURES, **ORDER_SIGNATURES, **SOLVE_TREE_SIGNATURES,
                              **SOLVE_HASH_SIGNATURES, **SOLVE_WINDOW_SIGNATURES, **MOVES_SIGNATURES,
                              **BUDGET_SIGNATURES, **LINE_SIGNATURES, **PLAY_SOLVE_SIGNATURES,
                              **PERFT_SIGNATURES, **MCTS_SIGNATURES, **MCTS_TREE_SIGNATURES,
                              **MCTS_WIDE_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status != OTH_OK:
        if status == OTH_EINVAL:
            raise OthelloCallError(f"{what}: invalid argument (OTH_EINVAL)")
        raise OthelloCallError(f"{what}: HIP error {-status}")


def version():
    return load().oth_version().decode()


def library_sha16(path=None):
    """First 16 hex digits of the SHA-256 of the HIP library file: the build
    identity that bench lines and profile digests are stamped with (the build
    is deterministic: the same sources and flags give the same file)."""
    import hashlib

    with open(path or LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]
