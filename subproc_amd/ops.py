"""Tensor-level batched Othello ops on the MI355X (one call = one HIP launch).

Every function takes/returns torch tensors resident on a ROCm device and calls
the C-ABI of include/othello.h on torch's current stream.  Bitboards are
``(n, 2)`` ``torch.int64`` tensors holding the uint64 bit patterns
``[black, white]`` (torch has no general uint64 arithmetic; the bits are what
matter, see :func:`to_numpy_u64`).  There is no CPU fallback: CPU tensors or a
missing library raise.

Reference mapping (board.py line numbers):
  reset   -> Board.__init__            22-27
  legal   -> Board.puttables           46-52   (n_puttable_for = popcount)
  step    -> Board.put_s / put         161-209
  result  -> n_black / n_white / is_game_over 37-58 + game_runner.py:194-199
  hands   -> Board.hands_for_direc     124-139 (any origin, all 8 directions)
  rollout -> GameRunner.play_a_game loop   game_runner.py:165-201
  evaluate -> linear eval of the learner's counts() features
  search  -> fixed-depth alpha-beta over that eval (what the Edax-protocol engines do)
  play    -> GameRunner matches between two such engines, whole games in one launch
"""
import ctypes
import numbers
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import (BLACK, BOOK_LINE, HIST_BINS, MOVES_STRIDE, N_FEATURES, PASS, POLICY_EVAL, POLICY_GREEDY,
                   POLICY_RANDOM, POS_STRIDE, WHITE, check)
from .params import DEFAULT_WEIGHTS, as_weights

StepResult = namedtuple("StepResult", "boards turn flips legal_next ret")
Result = namedtuple("Result", "n_black n_white diff terminal")
RolloutResult = namedtuple("RolloutResult", "final_boards diff plies moves hist")
Positions = namedtuple("Positions", "boards turn nturn move")
Replay = namedtuple("Replay", "boards turn end")
ReplayRows = namedtuple("ReplayRows", "boards turn end row_off")

_POLICIES = {"random": POLICY_RANDOM, "greedy": POLICY_GREEDY, "eval": POLICY_EVAL, POLICY_RANDOM: POLICY_RANDOM,
             POLICY_GREEDY: POLICY_GREEDY, POLICY_EVAL: POLICY_EVAL}


def _weights_ptr(weights):
    """Host int8[36] buffer for oth_eval / oth_rollout_eval (copied into the launch)."""
    w = as_weights(DEFAULT_WEIGHTS if weights is None else weights)
    return (ctypes.c_int8 * w.size).from_buffer_copy(w.tobytes())


def _stream():
    return ctypes_stream(torch.cuda.current_stream())


def ctypes_stream(s):
    return s.cuda_stream  # hipStream_t as an integer handle


def _dev(t, name, dtype, shape=None, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name}: tensor must be on a ROCm device (got {t.device}); there is no CPU path")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: tensor is on {t.device}, expected {device} (all arguments on one device)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def _opt(t, name, dtype, shape, device=None):
    return None if t is None else _dev(t, name, dtype, shape, device)


def _n(boards):
    if boards.dim() != 2 or boards.shape[1] != 2:
        raise ValueError(f"boards: expected shape (n, 2), got {tuple(boards.shape)}")
    return boards.shape[0]


def _device(device):
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"device must be a ROCm device, got {d}")
    if d.index is None:  # "cuda" -> the current device, so it compares equal to tensors' devices
        d = torch.device("cuda", torch.cuda.current_device())
    return d


# ---------------------------------------------------------------------------
def reset(n, device="cuda"):
    """n games at the opening position: (boards (n,2) int64, turn (n,) uint8, nturn (n,) uint8)."""
    d = _device(device)
    boards = torch.empty((n, 2), dtype=torch.int64, device=d)
    turn = torch.empty(n, dtype=torch.uint8, device=d)
    nturn = torch.empty(n, dtype=torch.uint8, device=d)
    with torch.cuda.device(d):
        check(_lib.load().oth_reset(boards.data_ptr(), turn.data_ptr(), nturn.data_ptr(), n, _stream()), "oth_reset")
    return boards, turn, nturn


def legal(boards, turn, out=None):
    """Legal-move bitboard of the side to move (Board.puttables as a mask)."""
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), boards.device)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=boards.device)
    po = _dev(out, "out", torch.int64, (n,), boards.device)
    with torch.cuda.device(boards.device):
        check(_lib.load().oth_legal(pb, pt, po, n, _stream()), "oth_legal")
    return out


def step(boards, turn, move, nturn=None, inplace=False, want_flips=True, want_legal=True):
    """One Board.put_s per game on integer move codes (0..63 square, 64 pass).

    Returns StepResult(boards, turn, flips, legal_next, ret) with ret exactly as
    board.py: -1 illegal (state unchanged), 0 pass, n >= 1 discs flipped.
    ``nturn`` (uint8, optional) is incremented in place where ret >= 0.
    ``inplace=True`` writes the new boards/turn into the input tensors.
    """
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), boards.device)
    pm = _dev(move, "move", torch.uint8, (n,), boards.device)
    pn = _opt(nturn, "nturn", torch.uint8, (n,), boards.device)
    dev = boards.device
    bo = boards if inplace else torch.empty_like(boards)
    to = turn if inplace else torch.empty_like(turn)
    fl = torch.empty(n, dtype=torch.int64, device=dev) if want_flips else None
    ln = torch.empty(n, dtype=torch.int64, device=dev) if want_legal else None
    ret = torch.empty(n, dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().oth_step(pb, pt, pm, bo.data_ptr(), to.data_ptr(), None if fl is None else fl.data_ptr(),
                                   None if ln is None else ln.data_ptr(), ret.data_ptr(), pn, n, _stream()),
              "oth_step")
    return StepResult(bo, to, fl, ln, ret)


def result(boards):
    """Result(n_black, n_white, diff = n_black - n_white, terminal = is_game_over())."""
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    dev = boards.device
    nb = torch.empty(n, dtype=torch.uint8, device=dev)
    nw = torch.empty(n, dtype=torch.uint8, device=dev)
    df = torch.empty(n, dtype=torch.int8, device=dev)
    te = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().oth_result(pb, nb.data_ptr(), nw.data_ptr(), df.data_ptr(), te.data_ptr(), n, _stream()),
              "oth_result")
    return Result(nb, nw, df, te)


def hands(own, hostile, x, y, dx, dy):
    """len(Board.hands_for_direc((dx, dy), piece, x, y)) (board.py:124-139) per
    item, for any origin and direction (int64: off-board origins included);
    own[i] / hostile[i] = squares holding the piece / hostile(piece).  The
    returned squares are (x + k*dx, y + k*dy), k = 1..count: (n,) uint8."""
    n = own.shape[0]
    po = _dev(own, "own", torch.int64, (n,))
    ph = _dev(hostile, "hostile", torch.int64, (n,), own.device)
    pc = [_dev(v, nm, torch.int64, (n,), own.device) for v, nm in ((x, "x"), (y, "y"), (dx, "dx"), (dy, "dy"))]
    out = torch.empty(n, dtype=torch.uint8, device=own.device)
    with torch.cuda.device(own.device):
        check(_lib.load().oth_hands(po, ph, *pc, out.data_ptr(), n, _stream()), "oth_hands")
    return out


_WORK = {}


def work_word(device=None):
    """The rollout work word of torch's current stream on `device` (one zeroed
    device uint64 per (device, stream), include/othello.h oth_rollout): a
    launch finds it at 0 and leaves it at 0, so launches ordered on one stream
    share it and launches on different streams never do."""
    d = _device("cuda" if device is None else device)
    with torch.cuda.device(d):
        key = (d.index, torch.cuda.current_stream().cuda_stream)
        w = _WORK.get(key)
        if w is None:
            w = torch.zeros(1, dtype=torch.int64, device=d)  # zeroed on this stream, before any launch on it
            _WORK[key] = w
    return w


# The work-word launch protocol, stated once for every entry point that takes
# ``work``: _capturing refuses a missing word under capture, _work_ptr chooses
# the word, _launch makes the call and cleans up after a failed one.
def _capturing(name, work):
    """Whether the current stream is capturing; a capture without ``work`` raises."""
    capturing = torch.cuda.is_current_stream_capturing()
    if work is None and capturing:
        raise RuntimeError(f"ops.{name} under graph capture needs an explicit work word: an int64 (1,) device "
                           "tensor zeroed before the capture, one per captured launch")
    return capturing


def _work_ptr(work, d):
    """Address of the launch's work word: the caller's, else the current stream's."""
    return _dev(work_word(d) if work is None else work, "work", torch.int64, (1,), d)


def _drop_word(d, stream):
    """Forget the cached word of (d, stream): the next work_word makes a fresh zeroed one."""
    _WORK.pop((d.index, stream), None)


def _launch(what, fn, args, w, d):
    """``fn(*args, stream)`` on torch's current stream of device ``d``, then
    check(); ``w`` is the caller's ``work`` (None: the stream's word).  A failed
    launch leaves the counter unknown (include/othello.h): the stream's default
    word is dropped; a caller's word is reset eagerly, never as a captured node."""
    with torch.cuda.device(d):
        rc = fn(*args, _stream())
        if rc != _lib.OTH_OK:
            if w is None:
                _drop_word(d, _stream())
            elif not torch.cuda.is_current_stream_capturing():
                w.zero_()
        check(rc, what)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _outputs(n, dtype, want_nodes, d):
    """The value / best_move / status / nodes tensors of the solves and searches."""
    return (torch.empty(n, dtype=dtype, device=d), torch.empty(n, dtype=torch.uint8, device=d),
            torch.empty(n, dtype=torch.uint8, device=d),
            torch.empty(n, dtype=torch.int32, device=d) if want_nodes else None)


def _check32(name, x, lo=0):
    if not lo <= x < lo + 2**32:
        raise ValueError(f"{name} must fit 32 bits")


def rollout(n, seed, game_id0=0, policy="random", n_random=10, start=None, start_turn=None, record_moves=False,
            hist=None, device="cuda", want_boards=True, want_diff=True, want_plies=True, weights=None,
            weights_white=None, work=None):
    """Play n games to terminal on the GPU (one lane per game).

    Game i uses the RNG stream of global id game_id0 + i, so results do not
    depend on how games are split over launches or GPUs.  ``hist`` (int64[133])
    is accumulated into if given (zero it yourself), else a fresh zeroed one is
    returned: [0..128] diff+64, 129 black wins, 130 white wins, 131 draws,
    132 total plies (= env-steps).

    Policies: "random"; "greedy" (minimise the opponent's mobility) and "eval"
    (maximise the mover's linear eval under ``weights``, int8 [4, 9], default
    params.DEFAULT_WEIGHTS) after ``n_random`` random plies.  With
    ``weights_white`` the eval policy is a match: Black plays ``weights``,
    White plays ``weights_white`` (oth_rollout_match).

    ``work`` (int64 (1,) device tensor, 0 at the launch) is the launch's batch
    counter; default: the current stream's :func:`work_word`.  Under graph
    capture ``work`` is required: a replay runs on the replaying stream, so
    every captured launch needs a word of its own, zeroed before the capture
    (graphs replayed concurrently must not share one).
    """
    if policy not in _POLICIES:
        raise ValueError(f"policy must be 'random', 'greedy' or 'eval', got {policy!r}")
    _capturing("rollout", work)
    d = _device(device) if start is None else start.device
    ps = pst = None
    if start is not None:
        if _n(start) != n:
            raise ValueError("start must have n rows")
        ps = _dev(start, "start", torch.int64)
        pst = _opt(start_turn, "start_turn", torch.uint8, (n,), start.device)
    fb = torch.empty((n, 2), dtype=torch.int64, device=d) if want_boards else None
    df = torch.empty(n, dtype=torch.int8, device=d) if want_diff else None
    pl = torch.empty(n, dtype=torch.uint8, device=d) if want_plies else None
    mv = torch.empty((n, MOVES_STRIDE), dtype=torch.uint8, device=d) if record_moves else None
    if hist is None:
        hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=d)
    ph = _dev(hist, "hist", torch.int64, (HIST_BINS,), d)
    if _POLICIES[policy] != POLICY_EVAL and (weights is not None or weights_white is not None):
        raise ValueError("weights apply to policy 'eval' only")
    pw = _work_ptr(work, d)
    lib = _lib.load()
    if _POLICIES[policy] == POLICY_EVAL and weights_white is not None:
        fn, what, how = lib.oth_rollout_match, "oth_rollout_match", (n_random, _weights_ptr(weights),
                                                                     _weights_ptr(weights_white))
    elif _POLICIES[policy] == POLICY_EVAL:
        fn, what, how = lib.oth_rollout_eval, "oth_rollout_eval", (n_random, _weights_ptr(weights))
    else:
        fn, what, how = lib.oth_rollout, "oth_rollout", (_POLICIES[policy], n_random)
    _launch(what, fn, (ps, pst, seed & (2**64 - 1), game_id0, *how, _ptr(fb), _ptr(df), _ptr(pl), _ptr(mv), ph, pw, n),
            work, d)
    return RolloutResult(fb, df, pl, mv, hist)


_SIDE = {}


def _side_streams(d, k):
    """k side streams of device d, created once and reused (rollout_batches)."""
    have = _SIDE.setdefault(d.index, [])
    while len(have) < k:
        have.append(torch.cuda.Stream(d))
    return have[:k]


ROLLOUT_MERGE_GAMES = 1 << 24  # rollout_batches merges batches into launches of up to this many games


def rollout_batches(n, steps, seed, game_id0=0, policy="random", n_random=10, hist=None, device="cuda", streams=2,
                    want_boards=False, want_diff=False, want_plies=False, weights=None, merge=True):
    """`steps` batches of `n` games each, pipelined: batch s plays global ids
    [game_id0 + s*n, +n).  Consecutive batches are merged into launches of up
    to max(n, ROLLOUT_MERGE_GAMES) games (merge=False: one launch per batch),
    and the launches are issued round-robin on `streams` HIP streams (torch's
    current stream and streams - 1 side streams, each with its own work
    word), so the last batches of one launch share the CUs with the first
    batches of the next instead of leaving them idle (batch
    tail): ten batches of 1M games run as one launch of 10M, with one launch
    tail where ten launches had ten.  The result equals ``rollout(n * steps, seed, game_id0,
    ...)`` game for game whatever the launches: every game keeps the RNG
    stream of its global id, and the launches add into one histogram (device
    atomics).  Outputs, if asked for, are (n * steps, ...) in game-id order.
    On return the current stream is ordered after every launch; nothing is
    synchronised with the host.
    """
    if policy not in _POLICIES:
        raise ValueError(f"policy must be 'random', 'greedy' or 'eval', got {policy!r}")
    if steps < 1 or n < 0 or streams < 1:
        raise ValueError("rollout_batches: steps >= 1, n >= 0 and streams >= 1")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("rollout_batches issues on side streams: capture ops.rollout launches instead")
    d = _device(device)
    pid = _POLICIES[policy]
    if pid != POLICY_EVAL and weights is not None:
        raise ValueError("weights apply to policy 'eval' only")
    total = n * steps
    fb = torch.empty((total, 2), dtype=torch.int64, device=d) if want_boards else None
    df = torch.empty(total, dtype=torch.int8, device=d) if want_diff else None
    pl = torch.empty(total, dtype=torch.uint8, device=d) if want_plies else None
    if hist is None:
        hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=d)
    ph = _dev(hist, "hist", torch.int64, (HIST_BINS,), d)
    lib = _lib.load()
    wp = _weights_ptr(weights) if pid == POLICY_EVAL else None
    with torch.cuda.device(d):
        main = torch.cuda.current_stream()
        side = _side_streams(d, streams - 1)
        sts = [main] + side
        fork = torch.cuda.Event()
        fork.record(main)
        for st in side:
            st.wait_event(fork)
        # one work word per stream (0 before and after each launch on it): the
        # streams' cached words, as ops.rollout uses them
        works = []
        for st in sts:
            with torch.cuda.stream(st):
                works.append(work_word(d))
        per = 1  # batches per launch
        if merge and n > 0:
            per = max(1, min(steps, ROLLOUT_MERGE_GAMES // n))
        for L, s0 in enumerate(range(0, steps, per)):
            i = L % len(sts)
            st, w = sts[i], works[i]
            g0 = game_id0 + s0 * n
            m = min(per, steps - s0) * n  # this launch's games

            def part(t, k=1):
                return None if t is None else t.data_ptr() + s0 * n * k * t.element_size()

            if pid == POLICY_EVAL:
                rc = lib.oth_rollout_eval(None, None, seed & (2**64 - 1), g0, n_random, wp, part(fb, 2), part(df),
                                          part(pl), None, ph, w.data_ptr(), m, st.cuda_stream)
            else:
                rc = lib.oth_rollout(None, None, seed & (2**64 - 1), g0, pid, n_random, part(fb, 2), part(df),
                                     part(pl), None, ph, w.data_ptr(), m, st.cuda_stream)
            if rc != _lib.OTH_OK:  # the failed launch's word is unknown: drop it (ops.rollout does the same)
                _drop_word(d, st.cuda_stream)
            check(rc, "oth_rollout (rollout_batches launch %d)" % L)
        for st in side:  # the caller's stream waits for every launch
            e = torch.cuda.Event()
            e.record(st)
            main.wait_event(e)
        for t in (fb, df, pl, hist):
            if t is not None:
                for st in side:
                    t.record_stream(st)
    return RolloutResult(fb, df, pl, None, hist)


RunnerResult = namedtuple("RunnerResult", "final_boards diff plies moves hist a_black")


def rollout_runner(n, seed, game_id0=0, policy="eval", weights_a=None, weights_b=None, n_rand_a=0, n_rand_b=0,
                   swap_colours=False, start=None, start_turn=None, record_moves=False, hist=None, device="cuda",
                   work=None):
    """n GameRunner matches between player A and player B on the GPU
    (oth_rollout_runner, include/othello.h): both play ``policy`` ("greedy",
    or "eval" with tables ``weights_a`` / ``weights_b``, default
    params.DEFAULT_WEIGHTS), each places min(n_rand, 10) random moves by
    go_for's coin (game_runner.py:115-150), and with ``swap_colours`` each game
    draws who plays Black (subproc.do_match's proc_randomize_black_white).
    Game i is global id game_id0 + i.  ``a_black`` (n,) uint8: 1 where A
    played Black; diff / hist / final boards are by colour."""
    if policy not in ("greedy", "eval"):
        raise ValueError(f"policy must be 'greedy' or 'eval', got {policy!r}")
    _capturing("rollout_runner", work)
    d = _device(device) if start is None else start.device
    ps = pst = None
    if start is not None:
        if _n(start) != n:
            raise ValueError("start must have n rows")
        ps = _dev(start, "start", torch.int64)
        pst = _opt(start_turn, "start_turn", torch.uint8, (n,), start.device)
    fb = torch.empty((n, 2), dtype=torch.int64, device=d)
    df = torch.empty(n, dtype=torch.int8, device=d)
    pl = torch.empty(n, dtype=torch.uint8, device=d)
    ab = torch.empty(n, dtype=torch.uint8, device=d)
    mv = torch.empty((n, MOVES_STRIDE), dtype=torch.uint8, device=d) if record_moves else None
    if hist is None:
        hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=d)
    ph = _dev(hist, "hist", torch.int64, (HIST_BINS,), d)
    pw = _work_ptr(work, d)
    _launch("oth_rollout_runner", _lib.load().oth_rollout_runner,
            (ps, pst, seed & (2**64 - 1), game_id0, _POLICIES[policy], _weights_ptr(weights_a), _weights_ptr(weights_b),
             int(n_rand_a), int(n_rand_b), int(bool(swap_colours)), ab.data_ptr(), fb.data_ptr(), df.data_ptr(),
             pl.data_ptr(), _ptr(mv), ph, pw, n), work, d)
    return RunnerResult(fb, df, pl, mv, hist, ab)


SolveResult = namedtuple("SolveResult", "value best_move status nodes")


class SolveTable:
    """The split solver's transposition table (include/othello_solve_hash.h):
    2**bits entries of 32 bytes in device memory, zeroed (all zero is empty).
    The solver never clears it: what one ``ops.solve(..., table=t)`` proved is
    there for the next, whatever its order, task_empties or batch.  ``data`` is
    the int64 tensor, ``nbytes`` its size, ``clear()`` empties it.  One table
    serves the calls of one stream, one after the other."""

    def __init__(self, bits, device="cuda"):
        bits = int(bits)
        if not _lib.SOLVE_HASH_MIN_BITS <= bits <= _lib.SOLVE_HASH_MAX_BITS:
            raise ValueError(f"bits must lie in {_lib.SOLVE_HASH_MIN_BITS}..{_lib.SOLVE_HASH_MAX_BITS}")
        self.bits = bits
        self.nbytes = _lib.SOLVE_HASH_ENTRY_BYTES << bits
        self.data = torch.zeros(self.nbytes // 8, dtype=torch.int64, device=device)

    @property
    def device(self):
        return self.data.device

    def clear(self):
        self.data.zero_()


def _check_table(whose, table, task_empties, hash_min_empties, d):
    """The ``table`` / ``hash_min_empties`` checks of :func:`solve` and :func:`solve_moves`."""
    if table is None:
        return
    if task_empties is None:
        raise ValueError(f"{whose} table serves the split solver's tasks: table needs task_empties")
    if not isinstance(table, SolveTable):
        raise TypeError("table must be an ops.SolveTable")
    if not _lib.SOLVE_HASH_MIN_EMPTIES_LO <= int(hash_min_empties) <= _lib.SOLVE_HASH_MIN_EMPTIES_HI:
        raise ValueError(f"hash_min_empties must lie in {_lib.SOLVE_HASH_MIN_EMPTIES_LO}.."
                         f"{_lib.SOLVE_HASH_MIN_EMPTIES_HI}")
    if table.device != d:
        raise ValueError(f"table is on {table.device}, boards on {d}")


def _table_args(table, hash_min_empties):
    """bits, min_empties, table, table_bytes of the C-ABI; no table is 0, 0, NULL, 0."""
    return (0, 0, None, 0) if table is None else (table.bits, hash_min_empties, table.data.data_ptr(), table.nbytes)


def _solve_window(window, wld, n, d):
    """:func:`solve`'s ``window`` / ``wld`` as (alpha, beta), each an int8 (n,)
    device tensor or None (the full window's end); None: no window was given."""
    if wld:
        if window is not None:
            raise ValueError("ops.solve: wld=True is window=(-1, 1); give one of the two")
        window = (-1, 1)
    if window is None:
        return None
    try:
        lo, hi = window
    except (TypeError, ValueError):
        raise ValueError("window must be a pair (alpha, beta)") from None
    ends = []
    for name, x, full in (("alpha", lo, _lib.SOLVE_ALPHA_MIN), ("beta", hi, _lib.SOLVE_BETA_MAX)):
        if isinstance(x, torch.Tensor):
            _dev(x, "window " + name, torch.int8, (n,), d)
            ends.append(x)
        else:
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise ValueError(f"window {name} must be an int or an int8 ({n},) device tensor")
            if not _lib.SOLVE_ALPHA_MIN <= int(x) <= _lib.SOLVE_BETA_MAX:
                raise ValueError(f"window {name} must lie in {_lib.SOLVE_ALPHA_MIN}..{_lib.SOLVE_BETA_MAX}")
            ends.append(int(x))
    if not isinstance(ends[0], torch.Tensor) and not isinstance(ends[1], torch.Tensor) and ends[0] >= ends[1]:
        raise ValueError("window needs alpha < beta")
    # an int at the full window's end is the C-ABI's NULL; any other is spread over the batch
    return tuple(x if isinstance(x, torch.Tensor) else None if x == full
                 else torch.full((n,), x, dtype=torch.int8, device=d)
                 for x, full in zip(ends, (_lib.SOLVE_ALPHA_MIN, _lib.SOLVE_BETA_MAX)))


def solve(boards, turn, max_empties=12, node_limit=0, want_nodes=False, work=None, task_empties=None, order=0,
          nodes_per_position=_lib.SOLVE_TREE_DEFAULT_NODES, table=None,
          hash_min_empties=_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES, window=None, wld=False):
    """Exact endgame solve (oths_solve, include/othello_solve.h): for every
    position with at most ``max_empties`` (0..12) empty squares, the final disc
    difference under perfect play by both sides, from the mover's side (White
    if turn == 2, else Black; no bonus for empty squares), and the move that
    achieves it.

    Returns SolveResult(value int8, best_move uint8, status uint8, nodes):
    best_move is the lowest square among the best moves, 64 for a forced pass,
    255 when the game is over; status is _lib.SOLVE_SOLVED, SOLVE_SKIPPED (more
    empties: value 0, best_move 255), SOLVE_INVALID (black & white overlap) or
    SOLVE_LIMIT (the search of this position would have passed ``node_limit``
    moves and passes; 0 = the library's default, 2**28).  ``nodes`` (uint32 as
    int32 bits, with ``want_nodes``) is each position's count, else None.

    ``work`` as in :func:`rollout`: default the current stream's
    :func:`work_word` (shared with the rollouts), required under graph capture.

    ``task_empties`` = T (1..12) is the split solver (othe_solve,
    include/othello_solve_tree.h): the top of every position's tree is
    expanded, down to nodes of at most T empties, into a tree of at most
    ``nodes_per_position`` nodes in device memory, and the nodes at its bottom
    are solved by all the device's lanes, sharing bounds.  Values, moves and
    statuses are the same; ``max_empties`` may go to 16; ``node_limit`` bounds
    each task; a position whose tree does not fit its slab far enough down (a
    task would have more than 12 empties) ends as _lib.SOLVE_TREE_NOROOM (value
    0, move 255); ``nodes`` then depends on timing.  ``order`` = 1 orders the
    moves inside the tasks (the same results from a smaller tree; only a
    position within reach of ``node_limit`` may end differently).  It pays for
    small batches, down to one position.  The default slab, 65,536 nodes
    (3.25 MiB per position), holds four full plies of every 16-empties root of
    tests/golden/solve_deep/solve_deep.npz and of tools/solve_tree_bench.py's set, so
    none of them ends as NOROOM.  The scratch (othe_scratch_bytes) is allocated
    here, so this form does not run under graph capture.  Without
    ``task_empties`` the call is oths_solve's, and ``order`` must be 0.

    ``table`` (a :class:`SolveTable`; needs ``task_empties``) gives the tasks a
    transposition table (othh_solve_hashed, include/othello_solve_hash.h):
    search frames with at least ``hash_min_empties`` (1..12) empties look their
    position up and store what they prove.  Values, moves and statuses are the
    same with any table, of any size and contents, and any ``hash_min_empties``
    (only a position within reach of ``node_limit`` may end differently): both
    are speed knobs.  Keep the table between calls to reuse what was solved.

    ``window`` = (alpha, beta), -65 <= alpha < beta <= 65 from the mover's
    side, asks a cheaper question (othw_solve / othw_solve_split,
    include/othello_solve_window.h); each member is an int or an int8 (n,)
    device tensor, one window per position.  With V the exact value: ``value``
    is clamp(V, alpha, beta); ``best_move`` is the lowest maximiser when
    alpha < V < beta, the lowest move whose own value reaches beta when
    V >= beta, and 255 when V <= alpha (no move is proved); a forced pass is 64
    and a finished game 255 whatever the window.  ``wld=True`` is
    ``window=(-1, 1)``: the value is the sign of V, the move the lowest winning
    move, the lowest drawing move, or 255 on a loss.  Ints out of range raise
    ValueError; tensors are checked on the device, and a position whose window
    is out of range or empty ends as _lib.SOLVE_BADWINDOW (value 0, move 255).
    It works with and without ``task_empties``, ``order`` and ``table``; the
    answers do not depend on them.  Without a window the calls are the ones
    above, unchanged.
    """
    n = _n(boards)
    win = _solve_window(window, bool(wld), n, boards.device)
    capturing = _capturing("solve", work)
    _check32("node_limit", int(node_limit))
    _check_table("ops.solve's", table, task_empties, hash_min_empties, boards.device)
    if task_empties is not None:
        return _solve_split(boards, turn, n, int(max_empties), int(task_empties), int(order), int(node_limit),
                            want_nodes, work, int(nodes_per_position), capturing, table, int(hash_min_empties), win)
    if int(order) != 0:
        raise ValueError("ops.solve orders moves only inside the split solver's tasks: order needs task_empties")
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    val, mv, st, nd = _outputs(n, torch.int8, want_nodes, d)
    pw = _work_ptr(work, d)
    out = (int(max_empties), int(node_limit), val.data_ptr(), mv.data_ptr(), st.data_ptr(), _ptr(nd), pw, n)
    if win is None:
        _launch("oths_solve", _lib.load().oths_solve, (pb, pt, *out), work, d)
    else:
        _launch("othw_solve", _lib.load().othw_solve, (pb, pt, *map(_ptr, win), *out), work, d)
    return SolveResult(val, mv, st, nd)


def _solve_split(boards, turn, n, max_empties, task_empties, order, node_limit, want_nodes, work, nodes_per_position,
                 capturing, table=None, hash_min_empties=_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES, win=None):
    """:func:`solve` with task_empties set: othe_solve on a scratch of its own
    (othh_solve_hashed with a table, othw_solve_split with a window)."""
    if capturing:
        raise RuntimeError("ops.solve(task_empties=...) allocates its scratch and does not run under graph capture")
    _check32("nodes_per_position", nodes_per_position, -2**31)
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    lib = _lib.load()
    size = lib.othe_scratch_bytes(n, nodes_per_position)
    if size < 0:
        check(int(size), "othe_scratch_bytes")
    val, mv, st, nd = _outputs(n, torch.int8, want_nodes, d)
    scratch = torch.empty(max(int(size), 8) // 8, dtype=torch.int64, device=d)
    args = (pb, pt, max_empties, task_empties, order, node_limit, val.data_ptr(), mv.data_ptr(), st.data_ptr(),
            _ptr(nd), scratch.data_ptr(), scratch.numel() * 8, nodes_per_position, _work_ptr(work, d), n)
    if win is not None:
        _launch("othw_solve_split", lib.othw_solve_split,
                (*args, *map(_ptr, win), *_table_args(table, hash_min_empties)), work, d)
    elif table is None:
        _launch("othe_solve", lib.othe_solve, args, work, d)
    else:
        _launch("othh_solve_hashed", lib.othh_solve_hashed, (*args, *_table_args(table, hash_min_empties)), work, d)
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return SolveResult(val, mv, st, nd)


SearchResult = namedtuple("SearchResult", "value best_move status nodes")


def search(boards, turn, depth, weights=None, node_limit=0, want_nodes=False, work=None, split=0,
           nodes_per_position=_lib.TREE_DEFAULT_NODES, order=0):
    """Depth-limited alpha-beta search (othm_search, include/othello_search.h):
    every position is searched ``depth`` (1..8) plies deep for its mover (White
    if turn == 2, else Black) with the linear eval of ``weights`` (int8 [4, 9],
    default params.DEFAULT_WEIGHTS) at the horizon, scored from the root mover's
    side; a game decided inside the horizon is worth 2**17 times its disc
    difference.  Depth 1 chooses the move of the 1-ply "eval" policy; a depth of
    at least the number of empties gives 2**17 times :func:`solve`'s value.

    Returns SearchResult(value int32, best_move uint8, status uint8, nodes):
    best_move is the lowest square among the best moves, 64 for a forced pass,
    255 when the game is over; status is _lib.SEARCH_SEARCHED, SEARCH_INVALID
    (black & white overlap) or SEARCH_LIMIT (this position's search would have
    passed ``node_limit`` moves and passes; 0 = the library's default, 2**28).
    ``nodes`` (uint32 as int32 bits, with ``want_nodes``) is each position's
    count, else None.

    ``work`` as in :func:`rollout`: default the current stream's
    :func:`work_word` (shared with the rollouts and solves), required under
    graph capture.

    ``split`` >= 1 (up to 4) is the split search (otht_search,
    include/othello_tree.h): the top ``split`` plies of every position are
    expanded into a tree of at most ``nodes_per_position`` nodes in device
    memory and the nodes at its bottom are searched by all the device's lanes,
    sharing bounds.  Values and moves are the same; ``depth`` may go to
    8 + split; ``node_limit`` bounds each task; a position whose tree does not
    fit its slab far enough down ends as _lib.TREE_NOROOM (value 0, move 255);
    ``nodes`` then depends on timing.  It pays for small batches, down to one
    position.  The scratch (otht_scratch_bytes) is allocated here, so this
    form does not run under graph capture.

    ``order`` = 1 searches with move ordering (otho_search_ordered /
    otho_tree_ordered, include/othello_order.h): value, best_move and status
    are those of ``order`` = 0, ties included, from a smaller tree; ``nodes``
    then counts the ordering's scoring placements too, and only a position
    within reach of ``node_limit`` may end differently.  With ``split`` the
    searches inside the tasks are ordered, the tree's expansion is not.
    """
    n = _n(boards)
    capturing = _capturing("search", work)
    _check32("node_limit", int(node_limit))
    if int(split) != 0:
        return _search_split(boards, turn, n, int(depth), int(split), weights, int(node_limit), want_nodes, work,
                             int(nodes_per_position), capturing, int(order))
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    val, mv, st, nd = _outputs(n, torch.int32, want_nodes, d)
    pw = _work_ptr(work, d)
    lib = _lib.load()
    fn, name, ordered = (lib.otho_search_ordered, "otho_search_ordered", (int(order),)) if int(order) != 0 else (
        lib.othm_search, "othm_search", ())
    _launch(name, fn, (pb, pt, int(depth), *ordered, _weights_ptr(weights), int(node_limit), val.data_ptr(),
                       mv.data_ptr(), st.data_ptr(), _ptr(nd), pw, n), work, d)
    return SearchResult(val, mv, st, nd)


def _search_split(boards, turn, n, depth, split, weights, node_limit, want_nodes, work, nodes_per_position, capturing,
                  order=0):
    """:func:`search` with split >= 1: otht_search (otho_tree_ordered with order != 0) on a scratch of its own."""
    if capturing:
        raise RuntimeError("ops.search(split >= 1) allocates its scratch and does not run under graph capture")
    _check32("nodes_per_position", nodes_per_position, -2**31)
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    lib = _lib.load()
    size = lib.otht_scratch_bytes(n, nodes_per_position)
    if size < 0:
        check(int(size), "otht_scratch_bytes")
    val, mv, st, nd = _outputs(n, torch.int32, want_nodes, d)
    scratch = torch.empty(max(int(size), 8) // 8, dtype=torch.int64, device=d)
    pw = _work_ptr(work, d)
    fn, name, ordered = (lib.otho_tree_ordered, "otho_tree_ordered", (order,)) if order != 0 else (
        lib.otht_search, "otht_search", ())
    _launch(name, fn, (pb, pt, depth, split, *ordered, _weights_ptr(weights), node_limit, val.data_ptr(),
                       mv.data_ptr(), st.data_ptr(), _ptr(nd), scratch.data_ptr(), scratch.numel() * 8,
                       nodes_per_position, pw, n), work, d)
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return SearchResult(val, mv, st, nd)


BudgetResult = namedtuple("BudgetResult", "value best_move status depth nodes")


def search_budget(boards, turn, budget, max_depth=8, weights=None, order=0, want_nodes=False, work=None):
    """Search by node budget (othb_search, include/othello_budget.h): every
    position is searched by iterative deepening -- :func:`search` at depth 1,
    2, ... up to ``max_depth`` (1..8) or the number of empty squares -- until the
    next iteration would take the position past its ``budget`` of nodes (an int
    >= 1 for all, or a uint32 / int64 tensor of n; a position with budget 0 is
    not searched).  The answer is that of the deepest iteration that completed;
    iteration d is exactly ``search(depth=d)``, so every field can be checked
    against it.  A lane's work is bounded by its budget, whatever the position.

    Returns BudgetResult(value int32, best_move uint8, status uint8, depth
    uint8, nodes): ``depth`` is the deepest completed iteration; status is
    _lib.SEARCH_SEARCHED, SEARCH_INVALID (black & white overlap) or SEARCH_LIMIT
    (not even depth 1 fitted the budget: value 0, move 255, depth 0).  ``nodes``
    (uint32 as int32 bits, with ``want_nodes``) sums the completed iterations,
    so it never exceeds the budget.  ``order`` = 1 deepens with the ordered
    search: the same value and move per depth, other node counts, so the depth
    reached may differ.  ``work`` as in :func:`search`."""
    n = _n(boards)
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    capturing = _capturing("search_budget", work)
    per_position = None
    if isinstance(budget, torch.Tensor):
        if budget.dtype == torch.int64:
            if capturing:
                raise RuntimeError("ops.search_budget under graph capture takes a uint32 budget tensor")
            if n and not bool(((budget >= 0) & (budget < 2**32)).all()):
                raise ValueError("budget must fit 32 bits")
            per_position = budget.to(torch.int32).view(torch.uint32)  # (the low 32 bits)
        elif budget.dtype == torch.uint32:
            per_position = budget
        else:
            raise TypeError(f"budget: expected an int or a uint32 / int64 tensor, got {budget.dtype}")
        pbud = _dev(per_position, "budget", per_position.dtype, (n,), d)
        scalar = 0
    else:
        scalar, pbud = int(budget), None
        if not 1 <= scalar < 2**32:
            raise ValueError("budget must lie in 1..2**32 - 1")
    val, mv, st, nd = _outputs(n, torch.int32, want_nodes, d)
    dp = torch.empty(n, dtype=torch.uint8, device=d)
    pw = _work_ptr(work, d)
    _launch("othb_search", _lib.load().othb_search,
            (pb, pt, int(max_depth), _weights_ptr(weights), scalar, pbud, int(order), val.data_ptr(), mv.data_ptr(),
             dp.data_ptr(), st.data_ptr(), _ptr(nd), pw, n), work, d)
    return BudgetResult(val, mv, st, dp, nd)


MovesResult = namedtuple("MovesResult", "move_value value best_move status nodes")


def _moves_call(name, fn, size, head, boards, turn, n, dtype, want_nodes, work):
    """The shared half of :func:`solve_moves` and :func:`search_moves`: the
    outputs, a scratch of ``size`` bytes, the work word, and the call
    ``fn(boards, turn, *head, move_value, value, best_move, status, nodes,
    scratch, scratch_bytes, work, n, stream)``."""
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    if size < 0:
        check(int(size), name + "_scratch_bytes")
    rows = torch.empty((n, 64), dtype=dtype, device=d)
    val, mv, st, nd = _outputs(n, dtype, want_nodes, d)
    scratch = torch.empty(max(int(size), 16) // 8, dtype=torch.int64, device=d)
    _launch(name, fn, (pb, pt, *head, rows.data_ptr(), val.data_ptr(), mv.data_ptr(), st.data_ptr(), _ptr(nd),
                       scratch.data_ptr(), scratch.numel() * 8, _work_ptr(work, d), n), work, d)
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return MovesResult(rows, val, mv, st, nd)


def solve_moves(boards, turn, max_empties=12, node_limit=0, want_nodes=False, work=None, task_empties=None, order=0,
                nodes_per_position=_lib.SOLVE_TREE_DEFAULT_NODES, table=None,
                hash_min_empties=_lib.SOLVE_HASH_DEFAULT_MIN_EMPTIES):
    """The exact value of EVERY root move (otha_solve_moves /
    otha_solve_moves_split, include/othello_moves.h): :func:`solve`'s answer
    for each position with at most ``max_empties`` empties, and beside it what
    each legal move is worth.

    Returns MovesResult(move_value int8 (n, 64), value int8, best_move uint8,
    status uint8, nodes).  ``move_value[i, s]`` is the final disc difference
    from the mover's side after playing square s, then perfect play by both
    sides; _lib.MOVES_NOT_A_MOVE (-128) where s is not a legal move,
    _lib.MOVES_UNKNOWN (-127) where the move's subtree hit ``node_limit`` (or,
    split, did not fit its slab).  ``value``, ``best_move`` are :func:`solve`'s:
    the row's maximum and its lowest maximising square; a forced pass has a row
    of -128, move 64 and the passed position's value; a finished game its disc
    difference and move 255; a row with an unknown move 0 and 255.  ``status``
    is SOLVE_SKIPPED / SOLVE_INVALID as in :func:`solve` (rows all -128), else
    the largest status among the position's moves (SOLVED < LIMIT < NOROOM).
    ``node_limit`` bounds each root move's subtree, not the position;
    ``nodes`` (with ``want_nodes``) counts the root moves and their subtrees.

    ``task_empties``, ``order``, ``nodes_per_position``, ``table`` and
    ``hash_min_empties`` are :func:`solve`'s: with ``task_empties`` every root
    move is solved by the split solver (``max_empties`` up to 16).  Every move
    slot, max(max_empties, 1) per position, then costs a slab of
    ``nodes_per_position`` nodes (52 B each): a batch wants a smaller
    ``nodes_per_position`` than the default, which suits single positions
    (16 slots x 3.25 MiB).  There is no root window here.

    Argument checks and ``work`` as in :func:`solve`.  Both forms allocate
    their scratch here (the caching allocator's memory, no synchronisation);
    the one-lane form may be captured in a graph with an explicit work word —
    the scratch then belongs to the graph's pool — the split form may not.
    """
    n = _n(boards)
    _check32("node_limit", int(node_limit))
    if task_empties is None and int(order) != 0:
        raise ValueError("ops.solve_moves orders moves only inside the split solver's tasks: order needs task_empties")
    _check_table("ops.solve_moves'", table, task_empties, hash_min_empties, boards.device)
    _dev(boards, "boards", torch.int64)  # (a host tensor is refused before anything asks the device)
    capturing = _capturing("solve_moves", work)
    lib = _lib.load()
    if task_empties is None:
        return _moves_call("otha_solve_moves", lib.otha_solve_moves,
                           lib.otha_solve_moves_scratch_bytes(n, int(max_empties)),
                           (int(max_empties), int(node_limit)), boards, turn, n, torch.int8, want_nodes, work)
    if capturing:
        raise RuntimeError("ops.solve_moves(task_empties=...) does not run under graph capture")
    npp = int(nodes_per_position)
    _check32("nodes_per_position", npp, -2**31)
    return _moves_call("otha_solve_moves_split", lib.otha_solve_moves_split,
                       lib.otha_solve_moves_split_scratch_bytes(n, int(max_empties), npp),
                       (int(max_empties), int(task_empties), int(order), int(node_limit), npp,
                        *_table_args(table, int(hash_min_empties))), boards, turn, n, torch.int8, want_nodes, work)


def search_moves(boards, turn, depth, weights=None, node_limit=0, want_nodes=False, work=None):
    """The depth-limited value of EVERY root move (otha_search_moves,
    include/othello_moves.h): :func:`search`'s answer at ``depth`` (1..8), and
    beside it what each legal move is worth to the root mover.

    Returns MovesResult(move_value int32 (n, 64), value int32, best_move uint8,
    status uint8, nodes).  ``move_value[i, s]`` is the depth - 1 search of the
    position after square s WITH THE LEAVES SCORED FROM THE ROOT MOVER'S SIDE
    (what a host loop of :func:`search` over the children cannot give: it
    scores them from the child's mover's side, and the eval is not
    antisymmetric); at depth 1 it is :func:`evaluate` of the child for the root
    mover, or 2**17 times the disc difference where the game ends there.
    _lib.MOVES_NOT_A_MOVE32 (-2**31) where s is not a legal move,
    _lib.MOVES_UNKNOWN32 where the move's subtree hit ``node_limit``.
    ``value``, ``best_move`` and ``status`` are :func:`search`'s (a row with an
    unknown move: 0, 255, SEARCH_LIMIT); ``node_limit`` bounds each root
    move's subtree.  No ``split`` and no ``order`` here.

    ``work`` as in :func:`search`.  The scratch (1.7 KB per position) is
    allocated here; the call may be captured in a graph with an explicit work
    word.
    """
    n = _n(boards)
    _check32("node_limit", int(node_limit))
    _dev(boards, "boards", torch.int64)  # (a host tensor is refused before anything asks the device)
    _capturing("search_moves", work)
    lib = _lib.load()
    return _moves_call("otha_search_moves", lib.otha_search_moves, lib.otha_search_moves_scratch_bytes(n),
                       (int(depth), _weights_ptr(weights), int(node_limit)), boards, turn, n, torch.int32, want_nodes,
                       work)


PerftResult = namedtuple("PerftResult", "leaves divide status nodes")


def perft(boards, turn, depth, split=0, want_divide=False, want_nodes=False, node_limit=0, max_tasks=1 << 20,
          work=None):
    """Perft (othc_perft, include/othello_perft.h): the number of move paths of
    length ``depth`` from every position for its mover (White if turn == 2,
    else Black).  A PASS IS A PLY and a finished game is one path whatever is
    left of the depth -- the published convention (from the opening 4, 12, 56,
    244, 1396, ...), not the searches' "a pass costs no depth".  ``depth`` is an
    int in 0..14 or a uint8 tensor with one depth per position.

    Returns PerftResult(leaves int64, divide int64 (n, 64) or None, status
    uint8, nodes int64 or None).  ``divide[i, s]`` (with ``want_divide``) is
    the count below root move s, 0 where s is no move; the row is all 0 at a
    root pass, a finished game and depth 0, else it sums to ``leaves[i]``.
    status is _lib.PERFT_COUNTED, PERFT_INVALID (black & white overlap),
    PERFT_LIMIT (a task ran into ``node_limit``; 0 = the library's default,
    2**28 positions per task) or PERFT_BADDEPTH (a per-position depth above
    14); the last three have counts of 0.  The counts stay below 2**62.
    ``nodes`` (with ``want_nodes``) is the number of positions the counting
    kernel generated moves for, a diagnostic that depends on ``split``.

    ``split`` = S (0..8) expands every position S plies, level by level on the
    device, into a list of at most ``max_tasks`` tasks (up to 2**24; 48 bytes
    of scratch each) that all the device's lanes then count: what spreads ONE
    position over the device, where split 0 gives it one lane.  A level that
    does not fit the list is skipped with those after it; leaves, divide and
    status do not depend on ``split`` or ``max_tasks``.  ``want_divide`` needs
    the root moves as tasks: it raises ``split`` to at least 1 and
    ``max_tasks`` to at least 64 per position.

    Argument checks and ``work`` as in :func:`search`.  The scratch is
    allocated here (the caching allocator's memory, no synchronisation) and
    nothing is read on the host, so the call may be captured in a graph with an
    explicit work word -- the scratch then belongs to the graph's pool.
    """
    n = _n(boards)
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    _capturing("perft", work)
    _check32("node_limit", int(node_limit))
    if isinstance(depth, torch.Tensor):
        pd, scalar = _dev(depth, "depth", torch.uint8, (n,), d), 0
    else:
        pd, scalar = None, int(depth)
        if not 0 <= scalar <= _lib.PERFT_MAX_DEPTH:
            raise ValueError(f"depth must lie in 0..{_lib.PERFT_MAX_DEPTH}")
    split, max_tasks = int(split), int(max_tasks)
    if not 0 <= split <= _lib.PERFT_MAX_SPLIT:
        raise ValueError(f"split must lie in 0..{_lib.PERFT_MAX_SPLIT}")
    if not 0 <= max_tasks <= _lib.PERFT_MAX_TASKS:
        raise ValueError(f"max_tasks must lie in 0..{_lib.PERFT_MAX_TASKS}")
    if want_divide:
        split, max_tasks = max(split, 1), max(max_tasks, _lib.PERFT_ROOT_SLOTS * n)
    lib = _lib.load()
    size = lib.othc_perft_scratch_bytes(n, max_tasks)
    if size < 0:
        check(int(size), "othc_perft_scratch_bytes")
    leaves = torch.empty(n, dtype=torch.int64, device=d)
    divide = torch.empty((n, 64), dtype=torch.int64, device=d) if want_divide else None
    status = torch.empty(n, dtype=torch.uint8, device=d)
    nodes = torch.empty(n, dtype=torch.int64, device=d) if want_nodes else None
    scratch = torch.empty(max(int(size), 16) // 8, dtype=torch.int64, device=d)
    _launch("othc_perft", lib.othc_perft, (pb, pt, scalar, pd, split, int(node_limit), leaves.data_ptr(), _ptr(divide),
                                           status.data_ptr(), _ptr(nodes), scratch.data_ptr(), scratch.numel() * 8,
                                           _work_ptr(work, d), n), work, d)
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return PerftResult(leaves, divide, status, nodes)


MctsResult = namedtuple("MctsResult", "visits wins diffs root_wins root_diffs best_move status nodes")

_LOG_TABLES = {}


def mcts_log_table(iterations):
    """The table :func:`mcts` hands the library: float32 ln(max(k, 1)) for k =
    0..iterations, computed in float64 and rounded once (numpy, host)."""
    T = int(iterations)
    if not 1 <= T <= _lib.MCTS_MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in 1..{_lib.MCTS_MAX_ITERATIONS}")
    return np.log(np.arange(T + 1, dtype=np.float64).clip(1)).astype(np.float32)


def _log_table_on(T, d):
    """mcts_log_table(T) on device d: uploaded once, cached per (T, device)."""
    key = (T, d.index)
    t = _LOG_TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ops.mcts under graph capture needs its table on the device before the capture: pass "
                               "log_table, or make one eager call with these iterations first")
        t = _LOG_TABLES[key] = torch.from_numpy(mcts_log_table(T)).to(d)
    return t


def mcts(boards, turn, iterations, explore=0.5, seed=0, game_id0=0, max_nodes=None, log_table=None, want_nodes=False,
         leaves=None):
    """Monte Carlo tree search (othu_mcts, include/othello_mcts.h): UCT over
    uniform random playouts, ``iterations`` = T (1..65536) iterations of 64
    playouts from every position for its mover (White if turn == 2, else
    Black), one wave per tree.  It needs no evaluation function.

    Returns MctsResult(visits int32 (n, 64), wins int32 (n, 64), diffs int32
    (n, 64), root_wins int32, root_diffs int32, best_move uint8, status uint8,
    nodes int32 or None).  ``visits[i, s]``, ``wins[i, s]`` and ``diffs[i, s]``
    are the iterations that went through root move s, the half-points of their
    playouts for the root mover (2 a win, 1 a draw: at most 128 per visit) and
    the sum of their final disc differences for the root mover; 0 where s is no
    move.  ``root_wins``, ``root_diffs`` are the same over all T iterations:
    ``root_wins / (128 * T)`` estimates the position's value for its mover.
    ``best_move`` is the move with the most visits (ties: more wins, then the
    lowest square), 64 where the mover must pass, 255 where the game is over;
    ``status`` _lib.MCTS_SEARCHED, or MCTS_INVALID (black & white overlap:
    everything 0, move 255).  ``nodes`` (with ``want_nodes``) counts the tree's
    nodes, at most ``max_nodes`` (1..2**20, default 1 + 16 T or 2**20): a tree that is
    full stops growing and goes on playing out from its leaves.

    ``explore`` is UCT's constant c in mean + c sqrt(ln n_parent / n_child),
    float32 with every operation rounded on its own.  Playout j of iteration t
    of position i is the game of global id ``game_id0 + (i T + t) 64 + j`` of
    ``seed`` (ops.rollout's games from the leaf), so the answer is a function
    of the arguments alone, and row i of a batch is the single call on
    position i with ``game_id0 + i T 64``.  ``log_table`` (float32 (T + 1,)
    device tensor) replaces :func:`mcts_log_table`'s values; the default table
    is uploaded once per (T, device).

    There is no work word.  The scratch (32 B per node for at most 4096 trees
    at a time) is allocated here (the caching allocator's memory, no
    synchronisation) and nothing is read on the host, so with the table on the
    device (``log_table`` passed in, or an earlier call with this T) the call
    may be captured in a graph -- the scratch then belongs to the graph's pool.

    ``leaves`` = L (1..16; None, the default: the call above and nothing else)
    runs the wide search (othv_mcts_wide, include/othello_mcts_wide.h):
    ``iterations`` = R rounds, each of L walkers that select one after another,
    every visit pending on a walker's path counting as a loss for the later
    ones, then L x 64 playouts, one wave per walker and one block of L waves
    per tree, backed up into the same tree.  The tree gets R L leaf visits
    (1..65536), so R L stands for T above: in the default ``max_nodes``, in the
    table's R L + 1 entries, in ``root_wins``.  Walker w of round r of position
    i plays the ids ``game_id0 + ((i R + r) L + w) 64 + j``; row i of a batch
    is the single call with ``game_id0 + i R L 64``.  The answer depends on L;
    with L = 1 it is the answer without ``leaves``.
    """
    R = int(iterations)
    L = None if leaves is None else int(leaves)
    if L is not None and not 1 <= L <= _lib.MCTS_WIDE_MAX_LEAVES:
        raise ValueError(f"leaves must lie in 1..{_lib.MCTS_WIDE_MAX_LEAVES}")
    T = R if L is None else R * L
    if R < 1 or not 1 <= T <= _lib.MCTS_MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in 1..{_lib.MCTS_MAX_ITERATIONS}" +
                         ("" if L is None else ", iterations x leaves too"))
    M = min(1 + 16 * T, _lib.MCTS_MAX_NODES) if max_nodes is None else int(max_nodes)
    if not 1 <= M <= _lib.MCTS_MAX_NODES:
        raise ValueError(f"max_nodes must lie in 1..{_lib.MCTS_MAX_NODES}")
    c = float(explore)
    if not abs(c) <= 3.0e38:
        raise ValueError("explore must be a finite float32")
    n = _n(boards)
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    table = _log_table_on(T, d) if log_table is None else log_table
    plt = _dev(table, "log_table", torch.float32, (T + 1,), d)
    lib = _lib.load()
    size = lib.othu_mcts_scratch_bytes(n, M) if L is None else lib.othv_mcts_wide_scratch_bytes(n, M, L)
    if size < 0:
        check(int(size), "othu_mcts_scratch_bytes" if L is None else "othv_mcts_wide_scratch_bytes")
    rows = [torch.empty((n, 64), dtype=torch.int32, device=d) for _ in range(3)]
    root = [torch.empty(n, dtype=torch.int32, device=d) for _ in range(2)]
    mv, st = (torch.empty(n, dtype=torch.uint8, device=d) for _ in range(2))
    nd = torch.empty(n, dtype=torch.int32, device=d) if want_nodes else None
    scratch = torch.empty(max(int(size), 16) // 8, dtype=torch.int64, device=d)
    tail = (c, plt, int(seed) & (2**64 - 1), int(game_id0) & (2**64 - 1), M, *(r.data_ptr() for r in rows),
            *(r.data_ptr() for r in root), mv.data_ptr(), st.data_ptr(), _ptr(nd), scratch.data_ptr(),
            scratch.numel() * 8, n)
    with torch.cuda.device(d):
        if L is None:
            check(lib.othu_mcts(pb, pt, T, *tail, _stream()), "othu_mcts")
        else:
            check(lib.othv_mcts_wide(pb, pt, R, L, *tail, _stream()), "othv_mcts_wide")
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return MctsResult(*rows, *root, mv, st, nd)


MctsTreesResult = namedtuple("MctsTreesResult", MctsResult._fields + ("ran", "root_boards", "root_turn"))
MctsPlayResult = namedtuple("MctsPlayResult", "final_boards diff plies moves hist a_black status root_visits")


def _mcts_pair(name, x, lo, hi, cast):
    """An argument that is one value for both players, or (A's, B's)."""
    pair = tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    if len(pair) != 2:
        raise ValueError(f"{name} must be one value or a pair (A's, B's)")
    pair = tuple(cast(v) for v in pair)
    if not all(lo <= v <= hi for v in pair):
        raise ValueError(f"{name} must lie in {lo}..{hi}")
    return pair


def _mcts_nodes(max_nodes, T):
    M = min(1 + 16 * T, _lib.MCTS_MAX_NODES) if max_nodes is None else int(max_nodes)
    if not 1 <= M <= _lib.MCTS_MAX_NODES:
        raise ValueError(f"max_nodes must lie in 1..{_lib.MCTS_MAX_NODES}")
    return M


class MctsTrees:
    """n Monte Carlo search trees that persist on the device (othr_*,
    include/othello_mcts_tree.h): :func:`mcts`'s trees kept between calls, so
    that a search can be resumed and a tree re-rooted on the move that was
    played, keeping the playouts below it.

    The object owns all memory: 64 B per node and tree (the tree and the room
    the re-rooting copies through) and 32 B of record per tree, the output
    tensors, and the device's table of logarithms (one per device, 65,537
    float32).  After construction every method is one asynchronous launch on
    the current stream that allocates nothing and reads nothing on the host, so
    it may be captured in a graph.  The tensors a method returns are the
    object's own: the next :meth:`search` or :meth:`rows` overwrites them
    (clone what must last).  Use one stream at a time.

    ``slabs`` (uint8 (n, 64 max_nodes); the tree is the first half of a row)
    and ``records`` (int64 (n, 4): id_base, played, nodes | turn << 32,
    status | max_nodes << 32) are the header's layout, for tests and debugging;
    :meth:`export` reads one tree into a canonical form."""

    def __init__(self, n, max_nodes, device="cuda"):
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        self.n, self.max_nodes = n, _mcts_nodes(max_nodes, 0)
        d = self.device = _device(device)
        lib = _lib.load()
        M = self.max_nodes
        self.slabs = torch.empty((n, 2 * M * _lib.MCTS_NODE_BYTES), dtype=torch.uint8, device=d)
        self.records = torch.zeros((n, _lib.MCTS_TREE_RECORD_BYTES // 8), dtype=torch.int64, device=d)
        assert lib.othr_trees_slab_bytes(n, M) == max(self.slabs.numel(), 16)
        assert lib.othr_trees_record_bytes(n) == max(self.records.numel() * 8, 16)
        self._table = _log_table_on(_lib.MCTS_MAX_ITERATIONS, d)
        i32 = dict(dtype=torch.int32, device=d)
        u8 = dict(dtype=torch.uint8, device=d)
        self._out = MctsTreesResult(torch.zeros((n, 64), **i32), torch.zeros((n, 64), **i32),
                                    torch.zeros((n, 64), **i32), torch.zeros(n, **i32), torch.zeros(n, **i32),
                                    torch.zeros(n, **u8), torch.zeros(n, **u8), torch.zeros(n, **i32),
                                    torch.zeros(n, **i32), torch.zeros((n, 2), dtype=torch.int64, device=d),
                                    torch.zeros(n, **u8))
        self._advanced = torch.zeros(n, **u8)

    def _trees(self):
        return (self.slabs.data_ptr(), self.slabs.numel(), self.records.data_ptr(), self.records.numel() * 8, self.n,
                _stream())

    def init(self, boards, turn, id_base=None, game_id0=0, stride=0):
        """Every tree becomes the root alone: position ``boards[i]`` with
        ``turn[i]`` to move, no visits, ``played`` = 0.  Its playouts' ids start
        at ``id_base[i]`` (int64 (n,) device tensor holding the uint64 bits) or
        at ``game_id0 + i * stride``.  Overlapping boards make tree i INVALID
        until the next init."""
        if _n(boards) != self.n:
            raise ValueError("boards must have n rows")
        d = self.device
        pb = _dev(boards, "boards", torch.int64, None, d)
        pt = _dev(turn, "turn", torch.uint8, (self.n,), d)
        pi = _opt(id_base, "id_base", torch.int64, (self.n,), d)
        with torch.cuda.device(d):
            check(_lib.load().othr_init(pb, pt, pi, int(game_id0) & (2**64 - 1), int(stride) & (2**64 - 1),
                                        self.max_nodes, *self._trees()), "othr_init")

    def search(self, iterations, explore=0.5, seed=0):
        """``iterations`` more iterations on every tree (an int 0..65536), or
        ``iterations[i]`` on tree i (int32 (n,) device tensor, >= 0); a tree
        never runs more than 65,536 - n_root, and one that runs none is
        untouched.  Iteration number ``played`` of a tree plays the games of
        ids ``id_base + played * 64 + lane`` of ``seed``.  Returns
        MctsTreesResult: :class:`MctsResult`'s fields (nodes always), ``ran``
        (int32: the iterations each tree ran), ``root_boards`` (n, 2) and
        ``root_turn``: the position the rows are about."""
        c = float(explore)
        if not abs(c) <= 3.0e38:
            raise ValueError("explore must be a finite float32")
        per = None
        if isinstance(iterations, torch.Tensor):
            per, T = _dev(iterations, "iterations", torch.int32, (self.n,), self.device), 0
        else:
            T = int(iterations)
            if not 0 <= T <= _lib.MCTS_MAX_ITERATIONS:
                raise ValueError(f"iterations must lie in 0..{_lib.MCTS_MAX_ITERATIONS}")
        with torch.cuda.device(self.device):
            check(_lib.load().othr_search(T, per, c, self._table.data_ptr(), int(seed) & (2**64 - 1), self.max_nodes,
                                          *(t.data_ptr() for t in self._out), *self._trees()), "othr_search")
        return self._out

    def rows(self):
        """:meth:`search`'s result with no iteration run."""
        with torch.cuda.device(self.device):
            check(_lib.load().othr_rows(self.max_nodes, *(t.data_ptr() for t in self._out), *self._trees()),
                  "othr_rows")
        return self._out

    def advance(self, moves, keep=True):
        """Play ``moves[i]`` (uint8: a square, 64 = pass, 255 = leave the tree)
        at the root of tree i.  With ``keep`` the child the move reaches becomes
        the root and keeps its visits and its whole subtree, the rest is
        dropped and its room freed; otherwise (or where the root has no
        children yet) the tree becomes the child position alone.  Returns the
        status (uint8 (n,), the object's own tensor): _lib.MCTS_TREE_READY,
        MCTS_TREE_INVALID, or MCTS_TREE_BADMOVE where the move is not one of
        the root mover's (the tree is then unchanged)."""
        pm = _dev(moves, "moves", torch.uint8, (self.n,), self.device)
        with torch.cuda.device(self.device):
            check(_lib.load().othr_advance(pm, int(bool(keep)), self.max_nodes, self._advanced.data_ptr(),
                                           *self._trees()), "othr_advance")
        return self._advanced

    def export(self, i):
        """Tree i read on the host (synchronises; for tests and debugging):
        dict(id_base, played, nodes, turn, status, tree) with ``tree`` the
        nodes in breadth-first order from the root, each (P, O, n, s, d, number
        of children): a form that does not depend on how the nodes are
        numbered in memory."""
        M = self.max_nodes
        rec = self.records[i].cpu().numpy().view(np.uint64)
        out = dict(id_base=int(rec[0]), played=int(rec[1]), nodes=int(rec[2]) & 0xFFFFFFFF, turn=int(rec[2]) >> 32,
                   status=int(rec[3]) & 0xFFFFFFFF, tree=[])
        if out["status"] != _lib.MCTS_TREE_READY or int(rec[3]) >> 32 != M:
            return out
        raw = self.slabs[i, :M * _lib.MCTS_NODE_BYTES].cpu().numpy()
        pos = raw[:16 * M].view(np.uint64).reshape(M, 2)
        ns = raw[16 * M:24 * M].view(np.uint32).reshape(M, 2)
        dl = raw[24 * M:].view(np.uint32).reshape(M, 2)
        order, q = [0], 0
        while q < len(order):
            v = order[q]
            q += 1
            first, cnt = int(dl[v, 1]) & 0xFFFFF, int(dl[v, 1]) >> 20
            out["tree"].append((int(pos[v, 0]), int(pos[v, 1]), int(ns[v, 0]), int(ns[v, 1]),
                                int(dl[v, 0].astype(np.int32)), cnt))
            order.extend(range(first, first + cnt))
            if len(order) > out["nodes"]:
                raise RuntimeError("tree %d: more nodes reachable than the record counts" % i)
        return out


def mcts_play(n, seed, game_id0=0, iterations=64, explore=0.5, reuse=True, a_black=None, start=None, start_turn=None,
              record_moves=False, max_nodes=None, hist=None, device="cuda", poll=1):
    """n whole games between two Monte Carlo tree searchers, player A and
    player B, each with trees of its own (what two engine processes have: a
    shared tree would hand one side's playouts to the other).  It needs no
    evaluation function.

    ``iterations`` = T or (Ta, Tb) iterations per move, ``explore`` = c or
    (ca, cb).  Every ply is one :meth:`MctsTrees.search` over all 2 n trees --
    the mover's T on the mover's tree, 0 on the other's (two launches where ca
    != cb) -- the mover's ``best_move``, and one :meth:`MctsTrees.advance` of
    both trees by it with ``keep = reuse``: with ``reuse`` both players keep
    the subtree below every move played, their own and the opponent's; without
    it every move is searched from a tree of one node, as a fresh :func:`mcts`
    call would.  ``reuse`` = (A's, B's) lets one side keep and the other not
    (then an advance per player).  A game ends where the move is 255.  The
    playouts' ids of player p's (0: A) tree of game i start at ``id_base =
    game_id0 + (2 i + p) * 2**32``; iteration number ``played`` of a tree
    plays ids ``id_base + played * 64 + lane`` of ``seed``, so the games are a
    function of the arguments alone.  (In memory A's n trees come first, then
    B's: the trees that search at a ply then spread evenly over the grid's
    blocks.)

    ``a_black`` (uint8 (n,) device tensor; default 1, 0, 1, ...: colours
    alternate) says where A plays Black.  ``start`` / ``start_turn`` as in
    :func:`rollout` (default: the opening, Black to move); random opening
    plies are the caller's business, through ``start``.  ``max_nodes`` per tree
    defaults to 1 + 16 max(Ta, Tb).

    Returns MctsPlayResult(final_boards, diff, plies, moves, hist, a_black,
    status, root_visits): the first six as :class:`RunnerResult`, with the
    encodings of :func:`rollout` (``moves`` 255-padded with ``record_moves``,
    else None; ``plies`` counts passes; ``hist`` is accumulated into if given
    and counts the finished games), so GameBooks.from_rollout takes it as it
    is.  ``status`` is _lib.MCTS_TREE_READY, or MCTS_TREE_INVALID where the
    start boards overlap (nothing played).  ``root_visits`` (int64) sums, over
    a game's plies, the visits the mover's root had when it chose: with reuse
    more than plies * T, the playouts kept.

    The loop is on the host, one launch per step; the only host read is the
    end test, once every ``poll`` plies (default every ply; a ply on finished
    games launches but runs no iteration)."""
    n, poll = int(n), int(poll)
    if n < 0 or poll < 1:
        raise ValueError("n must be >= 0 and poll >= 1")
    Ta, Tb = _mcts_pair("iterations", iterations, 1, _lib.MCTS_MAX_ITERATIONS, int)
    ca, cb = _mcts_pair("explore", explore, -3.0e38, 3.0e38, float)
    keep_a, keep_b = _mcts_pair("reuse", reuse, 0, 1, lambda v: int(bool(v)))
    M = _mcts_nodes(max_nodes, max(Ta, Tb))
    if start is None and start_turn is not None:
        raise ValueError("start_turn needs start")
    d = _device(device) if start is None else start.device
    if start is not None:
        if _n(start) != n:
            raise ValueError("start must have n rows")
        _dev(start, "start", torch.int64)
        _opt(start_turn, "start_turn", torch.uint8, (n,), start.device)
        boards = start
        turn = torch.ones(n, dtype=torch.uint8, device=d) if start_turn is None else start_turn.clone()
    else:
        boards, turn, _ = reset(n, d)
    if a_black is None:
        a_black = (1 - torch.arange(n, device=d) % 2).to(torch.uint8)
    _dev(a_black, "a_black", torch.uint8, (n,), d)
    if hist is None:
        hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=d)
    _dev(hist, "hist", torch.int64, (HIST_BINS,), d)
    ids = np.array([(int(game_id0) + ((2 * i + p) << 32)) & (2**64 - 1) for p in (0, 1) for i in range(n)],
                   np.uint64).view(np.int64)
    trees = MctsTrees(2 * n, M, d)  # tree p * n + i: player p's of game i
    trees.init(boards.repeat(2, 1), turn.repeat(2), torch.from_numpy(ids).to(d))
    moves = torch.full((n, MOVES_STRIDE), 255, dtype=torch.uint8, device=d) if record_moves else None
    plies = torch.zeros(n, dtype=torch.int64, device=d)
    root_visits = torch.zeros(n, dtype=torch.int64, device=d)
    alive = torch.ones(n, dtype=torch.bool, device=d)
    a_is_black = a_black != 0
    budget = torch.zeros((2, n), dtype=torch.int32, device=d)
    ply = 0
    while n:
        a_moves = (turn == BLACK) == a_is_black
        budget[0] = torch.where(alive & a_moves, Ta, 0)
        budget[1] = torch.where(alive & ~a_moves, Tb, 0)
        if ca == cb:
            r = trees.search(budget.view(-1), ca, seed)
        else:
            solo = budget.clone()
            solo[1] = 0
            trees.search(solo.view(-1), ca, seed)
            solo[0] = 0
            solo[1] = budget[1]
            r = trees.search(solo.view(-1), cb, seed)
        best, seen = r.best_move.view(2, n), r.visits.view(2, n, 64).sum(2)
        move = torch.where(a_moves, best[0], best[1])
        root_visits += torch.where(alive, torch.where(a_moves, seen[0], seen[1]), 0)
        alive = alive & (move != _lib.MCTS_NO_MOVE)
        move = torch.where(alive, move, torch.full_like(move, _lib.MCTS_NO_MOVE))
        if moves is not None and ply < MOVES_STRIDE:
            moves[:, ply] = move
        plies += alive
        if keep_a == keep_b:
            trees.advance(move.repeat(2), keep=keep_a)
        else:
            hold = torch.full_like(move, _lib.MCTS_TREE_KEEP)
            trees.advance(torch.cat((move, hold)), keep=keep_a)
            trees.advance(torch.cat((hold, move)), keep=keep_b)
        turn = torch.where(alive, 3 - turn, turn)
        ply += 1
        if ply % poll == 0 and not bool(alive.any()):
            break
    r = trees.rows()
    final = r.root_boards[:n].clone()
    status = r.status[:n].clone()
    res = result(final)
    done = status == _lib.MCTS_TREE_READY
    final = torch.where(done.unsqueeze(1), final, boards)  # (a game that could not start ends where it stood)
    diff = res.diff.to(torch.int64)
    ones = done.to(torch.int64)
    hist.index_add_(0, diff + 64, ones)
    hist.index_add_(0, torch.where(diff > 0, 129, torch.where(diff < 0, 130, 131)), ones)
    hist[HIST_BINS - 1] += (plies * ones).sum()
    return MctsPlayResult(final, res.diff.to(torch.int8), plies.to(torch.uint8), moves, hist, a_black, status,
                          root_visits)


LineResult = namedtuple("LineResult", "line length value best_move status nodes end_boards end_turn")


def _line_call(name, fn, head, boards, turn, n, dtype, want_nodes, work):
    """The shared half of :func:`solve_line` and :func:`search_line`: the
    outputs, the work word, and the call ``fn(boards, turn, *head, line,
    length, value, best_move, status, nodes, end_boards, end_turn, work, n,
    stream)``."""
    d = boards.device
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), d)
    line = torch.empty((n, _lib.LINE_STRIDE), dtype=torch.uint8, device=d)
    length = torch.empty(n, dtype=torch.uint8, device=d)
    val, mv, st, nd = _outputs(n, dtype, want_nodes, d)
    end = torch.empty((n, 2), dtype=torch.int64, device=d)
    end_turn = torch.empty(n, dtype=torch.uint8, device=d)
    _launch(name, fn, (pb, pt, *head, line.data_ptr(), length.data_ptr(), val.data_ptr(), mv.data_ptr(),
                       st.data_ptr(), _ptr(nd), end.data_ptr(), end_turn.data_ptr(), _work_ptr(work, d), n), work, d)
    return LineResult(line, length, val, mv, st, nd, end, end_turn)


def solve_line(boards, turn, max_empties=12, node_limit=0, want_nodes=False, work=None):
    """The line of perfect play (othl_solve_line, include/othello_line.h):
    :func:`solve`'s answer for each position with at most ``max_empties``
    (0..12) empties, and behind it the sequence of best moves and replies the
    value stands for, down to the end of the game.

    Returns LineResult(line uint8 (n, 32), length uint8, value int8, best_move
    uint8, status uint8, nodes, end_boards int64 (n, 2), end_turn uint8).
    ``line[i, :length[i]]`` are move codes (0..63, 64 for a pass), the rest is
    255; every entry is the lowest square among the best moves of the side to
    move there, so ``line[i, 0]`` is ``best_move[i]`` and a finished game has an
    empty line.  ``end_boards`` / ``end_turn`` are the position where the line
    ends and the side to move there: its disc difference from the root mover's
    side is ``value``.  ``value``, ``best_move`` and ``status`` are
    :func:`solve`'s.  ``node_limit`` bounds each search of the walk (one per
    entry of the line and one for the root); a position the root search
    resolves under it is resolved whole, one it does not is SOLVE_LIMIT with an
    empty line, 0 and 255.  ``nodes`` (with ``want_nodes``) sums the walk's
    searches.

    One launch; ``work`` as in :func:`solve`; the call may be captured in a
    graph with an explicit work word.  No split solver and no root window here.
    """
    n = _n(boards)
    _check32("node_limit", int(node_limit))
    _dev(boards, "boards", torch.int64)  # (a host tensor is refused before anything asks the device)
    _capturing("solve_line", work)
    return _line_call("othl_solve_line", _lib.load().othl_solve_line, (int(max_empties), int(node_limit)), boards,
                      turn, n, torch.int8, want_nodes, work)


def search_line(boards, turn, depth, weights=None, order=0, node_limit=0, want_nodes=False, work=None):
    """The line of the depth-limited search (othl_search_line,
    include/othello_line.h): :func:`search`'s answer at ``depth`` and behind it
    the sequence of best moves and replies down to the horizon (or the end of
    the game), every leaf scored from the ROOT mover's side — what a host loop
    of :func:`search` and :func:`step` cannot give, as it would score the second
    ply's leaves from the other side.

    ``depth`` is an int 1..8, or a uint8 (n,) device tensor with one depth per
    position: an entry of 0 is not searched (empty line, value 0, move 255,
    SEARCH_LIMIT — what :func:`search_budget` answers where not even depth 1
    fitted, so its ``depth`` output can be passed straight in), an entry above 8
    ends as _lib.LINE_BADDEPTH.

    Returns LineResult as :func:`solve_line` with ``value`` int32.  The end
    position's static score from the root mover's side is ``value``:
    :func:`evaluate` of it at a leaf, 2**17 times the disc difference where the
    game is over.  A line at a depth of at least the number of empties is
    :func:`solve_line`'s.  ``order`` = 1 walks with the ordered search: the same
    line from smaller trees, other ``nodes``.  ``node_limit`` as in
    :func:`solve_line` (with ``order`` = 1 a position within reach of it may end
    differently).  One launch; ``work`` as in :func:`search`; capturable with an
    explicit work word.  No split search here.
    """
    n = _n(boards)
    _check32("node_limit", int(node_limit))
    _dev(boards, "boards", torch.int64)  # (a host tensor is refused before anything asks the device)
    _capturing("search_line", work)
    if isinstance(depth, torch.Tensor):
        scalar, per = 0, _dev(depth, "depth", torch.uint8, (n,), boards.device)
    else:
        scalar, per = int(depth), None
        if not 1 <= scalar <= _lib.SEARCH_MAX_DEPTH:
            raise ValueError(f"depth must lie in 1..{_lib.SEARCH_MAX_DEPTH}")
    return _line_call("othl_search_line", _lib.load().othl_search_line,
                      (scalar, per, int(order), _weights_ptr(weights), int(node_limit)), boards, turn, n, torch.int32,
                      want_nodes, work)


PlayResult = namedtuple("PlayResult", "final_boards diff plies moves hist a_black status nodes")


def play(n, seed, game_id0=0, weights_a=None, weights_b=None, depth_a=1, depth_b=None, exact_empties=0, n_rand_a=0,
         n_rand_b=0, swap_colours=False, start=None, start_turn=None, record_moves=False, node_limit=0,
         want_nodes=False, hist=None, device="cuda", work=None, order=0, budget=None, solve_empties=0):
    """n whole games between two searching players in one launch (othp_play,
    include/othello_play.h): :func:`rollout_runner`'s match schedule -- player
    A against player B, the colour draw, the random-move budgets -- with every
    policy move chosen by :func:`search` at the mover's depth (``depth_a``,
    ``depth_b``, default ``depth_a``; 1..8) over the mover's table
    (``weights_a`` / ``weights_b``, default params.DEFAULT_WEIGHTS).  A mover
    without a move passes, a single legal move is played without a search, and
    once a position has at most ``exact_empties`` (0..8) empty squares the
    search runs to the end of the game, so the move is :func:`solve`'s.  Game i
    is global id game_id0 + i.

    Returns PlayResult(final_boards, diff, plies, moves, hist, a_black, status,
    nodes): the first six as :class:`RunnerResult` (so GameBooks.from_rollout
    takes it as it is); status is _lib.SEARCH_SEARCHED (played to its end),
    SEARCH_INVALID (the start boards overlap: nothing played) or SEARCH_LIMIT
    (a search would have passed ``node_limit`` nodes, 0 = the search's default:
    the game stops there); ``hist`` counts the finished games only.  ``nodes``
    (int64, with ``want_nodes``) is the sum of each game's search nodes.

    One lane plays one game: a launch lasts as long as its longest game.
    ``work`` as in :func:`rollout`.  ``order`` = 1: both players search with
    move ordering (otho_play_ordered, include/othello_order.h); the games are
    the same move for move, ``nodes`` is smaller.

    ``budget`` = B or (Ba, Bb), nodes per move (>= 1): every policy move is
    :func:`search_budget`'s with the mover's budget, ``depth_a`` / ``depth_b``
    being the depth caps (othb_play, include/othello_budget.h); the searches
    from ``exact_empties`` on keep ``node_limit`` and take no budget; ``nodes``
    sums the completed iterations.  A game then costs at most its plies times
    the budget, whatever its positions.  None: today's fixed-depth games.

    ``solve_empties`` = E in 1..12: once a position has at most E empty squares
    the policy move is :func:`solve`'s best move, from the exact solver's own
    machine (othx_play, include/othello_play_solve.h: the games leave the
    search's kernel for the solver's where they reach E empties).  Up to 8 the
    games are those of ``exact_empties`` = E; above it they are the ones the
    engine's ``--solve-empties`` plays.  ``node_limit`` bounds every solve too,
    ``nodes`` sums searches and solves, and a launch lasts as long as its
    hardest game's solves.  It takes the place of ``exact_empties`` (only one of
    the two may be non-zero); 0: the calls above, unchanged."""
    solve_empties = int(solve_empties)
    if not 0 <= solve_empties <= _lib.SOLVE_MAX_EMPTIES:
        raise ValueError("solve_empties must lie in 0..%d" % _lib.SOLVE_MAX_EMPTIES)
    if solve_empties and int(exact_empties):
        raise ValueError("solve_empties takes the place of exact_empties: only one of the two may be non-zero")
    budgets = ()
    if budget is not None:
        budgets = (int(budget),) * 2 if isinstance(budget, numbers.Integral) else tuple(int(b) for b in budget)
        if len(budgets) != 2 or not all(1 <= b < 2**32 for b in budgets):
            raise ValueError("budget must be an int or a pair (Ba, Bb) of ints in 1..2**32 - 1")
    _capturing("play", work)
    _check32("node_limit", int(node_limit))
    d = _device(device) if start is None else start.device
    ps = pst = None
    if start is not None:
        if _n(start) != n:
            raise ValueError("start must have n rows")
        ps = _dev(start, "start", torch.int64)
        pst = _opt(start_turn, "start_turn", torch.uint8, (n,), start.device)
    fb = torch.empty((n, 2), dtype=torch.int64, device=d)
    df = torch.empty(n, dtype=torch.int8, device=d)
    pl = torch.empty(n, dtype=torch.uint8, device=d)
    ab = torch.empty(n, dtype=torch.uint8, device=d)
    st = torch.empty(n, dtype=torch.uint8, device=d)
    mv = torch.empty((n, MOVES_STRIDE), dtype=torch.uint8, device=d) if record_moves else None
    nd = torch.empty(n, dtype=torch.int64, device=d) if want_nodes else None
    if hist is None:
        hist = torch.zeros(HIST_BINS, dtype=torch.int64, device=d)
    ph = _dev(hist, "hist", torch.int64, (HIST_BINS,), d)
    pw = _work_ptr(work, d)
    lib = _lib.load()
    fn, name, ordered = (lib.otho_play_ordered, "otho_play_ordered", (int(order),)) if int(order) != 0 else (
        lib.othp_play, "othp_play", ())
    if budgets:
        fn, name, ordered = lib.othb_play, "othb_play", (int(order),)
    zone, scratch = int(exact_empties), ()
    if solve_empties:
        fn, name, ordered, zone = lib.othx_play, "othx_play", (int(order),), solve_empties
        budgets = budgets or (0, 0)
        size = lib.othx_scratch_bytes(n)
        if size < 0:
            check(int(size), "othx_scratch_bytes")
        buf = torch.empty(int(size) // 8, dtype=torch.int64, device=d)
        scratch = (buf.data_ptr(), buf.numel() * 8)
    _launch(name, fn, (ps, pst, seed & (2**64 - 1), game_id0, _weights_ptr(weights_a), _weights_ptr(weights_b),
                       int(depth_a), int(depth_a if depth_b is None else depth_b), *budgets, zone,
                       *ordered, int(n_rand_a), int(n_rand_b), int(bool(swap_colours)), int(node_limit), ab.data_ptr(),
                       fb.data_ptr(), df.data_ptr(), pl.data_ptr(), _ptr(mv), st.data_ptr(), _ptr(nd), ph, *scratch,
                       pw, n), work, d)
    # (the caching allocator hands the scratch to later work of THIS stream only)
    return PlayResult(fb, df, pl, mv, hist, ab, st, nd)


def sample_midgame(n, seed, index0=0, device="cuda"):
    """Synthetic reachable mid-game positions + one random legal move each (config 2 inputs)."""
    d = _device(device)
    b = torch.empty((n, 2), dtype=torch.int64, device=d)
    t = torch.empty(n, dtype=torch.uint8, device=d)
    nt = torch.empty(n, dtype=torch.uint8, device=d)
    m = torch.empty(n, dtype=torch.uint8, device=d)
    with torch.cuda.device(d):
        check(_lib.load().oth_sample_midgame(seed & (2**64 - 1), index0, b.data_ptr(), t.data_ptr(), nt.data_ptr(),
                                             m.data_ptr(), n, _stream()), "oth_sample_midgame")
    return Positions(b, t, nt, m)


def replay(moves, plies, start=None, start_turn=None):
    """Every recorded position of n games (GameRunner records the board after
    Board() and after each put_s, game_runner.py:169-184).  Returns Replay with
    boards (n, 129, 2) int64, turn (n, 129) uint8, end (n, 129) uint8 =
    is_game_over(); game i's positions are rows 0..plies[i] (later rows: boards 0,
    turn 0, end 0)."""
    n = moves.shape[0]
    pm = _dev(moves, "moves", torch.uint8, (n, MOVES_STRIDE))
    pp = _dev(plies, "plies", torch.uint8, (n,), moves.device)
    ps = _opt(start, "start", torch.int64, (n, 2), moves.device)
    pst = _opt(start_turn, "start_turn", torch.uint8, (n,), moves.device)
    dev = moves.device
    # every row is written by the kernel (rows past plies as 0): no fill pass
    b = torch.empty((n, POS_STRIDE, 2), dtype=torch.int64, device=dev)
    t = torch.empty((n, POS_STRIDE), dtype=torch.uint8, device=dev)
    e = torch.empty((n, POS_STRIDE), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().oth_replay(ps, pst, pm, pp, b.data_ptr(), t.data_ptr(), e.data_ptr(), n, _stream()),
              "oth_replay")
    return Replay(b, t, e)


def row_offsets(plies):
    """Exclusive prefix sum of min(plies, 128) + 1 (int64, on plies' device):
    the first row of each game in an oth_replay_rows table; also returns the
    total row count (one host sync)."""
    cnt = plies.long().clamp(max=MOVES_STRIDE) + 1
    ends = torch.cumsum(cnt, 0)
    total = int(ends[-1]) if ends.numel() else 0
    return (ends - cnt).contiguous(), total


def replay_rows(moves, plies, start=None, start_turn=None):
    """ops.replay into packed rows (oth_replay_rows): game i's recorded
    positions are rows row_off[i] .. row_off[i] + plies[i] of boards (R, 2)
    int64, turn (R,) and end (R,) uint8, R = sum(plies + 1) -- only the rows
    GameRunner records, about half of the strided table of random games."""
    n = moves.shape[0]
    pm = _dev(moves, "moves", torch.uint8, (n, MOVES_STRIDE))
    pp = _dev(plies, "plies", torch.uint8, (n,), moves.device)
    ps = _opt(start, "start", torch.int64, (n, 2), moves.device)
    pst = _opt(start_turn, "start_turn", torch.uint8, (n,), moves.device)
    dev = moves.device
    row_off, total = row_offsets(plies)
    b = torch.empty((total, 2), dtype=torch.int64, device=dev)
    t = torch.empty(total, dtype=torch.uint8, device=dev)
    e = torch.empty(total, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().oth_replay_rows(ps, pst, pm, pp, row_off.data_ptr(), b.data_ptr(), t.data_ptr(),
                                          e.data_ptr(), n, _stream()), "oth_replay_rows")
    return ReplayRows(b, t, e, row_off)


def book_text(boards, turn):
    """serialize_str() + newline of each position (board.py:214-243), concatenated:
    a uint8 tensor of n * 67 bytes on the device."""
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    pt = _dev(turn, "turn", torch.uint8, (n,), boards.device)
    out = torch.empty(n * BOOK_LINE, dtype=torch.uint8, device=boards.device)
    with torch.cuda.device(boards.device):
        check(_lib.load().oth_book_text(pb, pt, n, out.data_ptr(), _stream()), "oth_book_text")
    return out


def book_parse(text, n, stride=64, want_turn=False):
    """Board strings back into bitboards (oth_book_parse): ``text`` a uint8
    device tensor holding n strings of 64 chars at a stride of ``stride``
    bytes (64 packed; 67 = OTH_BOOK_LINE for serialize_str lines).  Returns
    (boards (n, 2) int64, turn (n,) uint8 or None); ``want_turn`` parses the
    side after each board's space (needs stride >= 66)."""
    if not isinstance(text, torch.Tensor) or text.dtype != torch.uint8 or text.dim() != 1:
        raise TypeError("text: expected a 1-D uint8 tensor")
    if stride < 64 or (want_turn and stride < 66):
        raise ValueError("stride must be >= 64 (>= 66 to parse the side)")
    if n < 0 or (n > 0 and text.numel() < (n - 1) * stride + (66 if want_turn else 64)):
        raise ValueError(f"text holds fewer than {n} strings at stride {stride}")
    pt = _dev(text, "text", torch.uint8)
    dev = text.device
    b = torch.empty((n, 2), dtype=torch.int64, device=dev)
    t = torch.empty(n, dtype=torch.uint8, device=dev) if want_turn else None
    with torch.cuda.device(dev):
        check(_lib.load().oth_book_parse(pt, stride, b.data_ptr(), None if t is None else t.data_ptr(), n, _stream()),
              "oth_book_parse")
    return b, t


def features(boards, side):
    """counts() of parameter_progress_position_moves_learn.py:5-17 per position
    for side 1 ('O' = Black) / 2 ('X' = White): (n, 10) uint8 =
    (64 - n_empty, n_puttable_for(side), 8 region mask_counts)."""
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    ps = _dev(side, "side", torch.uint8, (n,), boards.device)
    out = torch.empty((n, N_FEATURES), dtype=torch.uint8, device=boards.device)
    with torch.cuda.device(boards.device):
        check(_lib.load().oth_features(pb, ps, out.data_ptr(), n, _stream()), "oth_features")
    return out


def evaluate(boards, side, weights=None):
    """Linear eval of each position from side 1 ('O') / 2 ('X')'s view: int32
    (n,) = sum_j W[shard(discs)][j] * counts()[1+j] (include/othello.h oth_eval;
    the model progress_position_moves_learn.py:160-184 fits)."""
    n = _n(boards)
    pb = _dev(boards, "boards", torch.int64)
    ps = _dev(side, "side", torch.uint8, (n,), boards.device)
    out = torch.empty(n, dtype=torch.int32, device=boards.device)
    with torch.cuda.device(boards.device):
        check(_lib.load().oth_eval(pb, ps, _weights_ptr(weights), out.data_ptr(), n, _stream()), "oth_eval")
    return out


# ---------------------------------------------------------------------------
# host <-> device conversion helpers (uint64 bit patterns)
# ---------------------------------------------------------------------------
def to_numpy_u64(t):
    """Device/host int64 tensor -> numpy uint64 array with the same bits."""
    return t.detach().cpu().numpy().view(np.uint64)


def from_numpy_u64(a, device="cuda"):
    """numpy uint64 array -> int64 tensor with the same bits on `device`."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).to(device)


__all__ = ["reset", "legal", "step", "result", "hands", "rollout", "work_word", "solve", "SolveTable", "search", "play",
           "search_budget", "BudgetResult",
           "solve_moves", "search_moves", "MovesResult",
           "solve_line", "search_line", "LineResult",
           "perft", "PerftResult",
           "mcts", "mcts_log_table", "MctsResult", "MctsTrees", "MctsTreesResult", "mcts_play", "MctsPlayResult",
           "sample_midgame",
           "replay",
           "book_text", "features", "evaluate", "to_numpy_u64", "from_numpy_u64",
           "StepResult", "Result", "RolloutResult", "PlayResult", "Positions", "Replay", "BLACK", "WHITE", "PASS", "HIST_BINS"]
