"""The identities behind the random loop's issue-cost changes (bitboard.hpp,
othello.hip's ply_of; profiles/loop_cost_notes.md), restated in numpy / plain
Python and checked against the plain definitions.  No GPU.

* the k-th-bit search without its variable shift: the byte is read at bit
  (b32 | s16 | s8) & 31 of the selected word;
* the pass flag as a disc count, the pass count corrected after the loop;
* the east reach read off the carry sum (the issue's 3(c)): true, and not
  taken, because it needs P << 1 on its own -- kept here so that the identity
  the notes quote stays checked."""
import importlib.util
import itertools
import os
import random

import numpy as np

import synthetic_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER = 0x7E
INNER_FILES = np.uint64(0x7E7E7E7E7E7E7E7E)
M64 = (1 << 64) - 1


def popc(x):
    return bin(x).count("1")


def kth_plain(x, k):
    for i in range(64):
        if x >> i & 1:
            if k == 0:
                return i
            k -= 1
    raise AssertionError


def kth_level(k, c, s):
    """kth_level<S>: k stays or becomes k - c by the borrow; the level's offset."""
    return (k, 0) if k < c else (k - c, s)


def kth_new(x, k):
    """kth_bit_off as shipped: w is never shifted; both byte reads take bits 4:0
    of their offset, as v_bfe_u32 does."""
    lo, hi = x & 0xFFFFFFFF, x >> 32
    k, b32 = kth_level(k, popc(lo), 32)
    w = hi if b32 else lo
    k, s16 = kth_level(k, popc(w & 0xFFFF), 16)
    k, s8 = kth_level(k, popc(w >> (s16 & 31) & 0xFF), 8)
    lvl = b32 | s16 | s8
    byte = w >> (lvl & 31) & 0xFF
    return lvl + kth_plain(byte, k)  # (the LDS byte table's entry)


def test_kth_bit_without_the_shift():
    rng = random.Random(0x10C0)
    xs = [1, 1 << 63, M64, 0x8000000080000000, 0x0001000100010001, 0xFF00FF00FF00FF00]
    xs += [rng.getrandbits(64) for _ in range(300)]
    xs += [rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64) | 1 << rng.randrange(64) for _ in range(300)]
    for x in xs:
        for k in range(popc(x)):
            assert kth_new(x, k) == kth_plain(x, k), (hex(x), k)


def old_flag(events, discs, passed, npass):
    """The parent's bookkeeping: events[i] is True when the mover has a move."""
    for has_move in events:
        if not has_move:
            if passed or discs == 64:
                if passed:
                    npass -= 1
                return discs, npass, True, None
            passed, npass = True, npass + 1
        else:
            passed, discs = False, discs + 1
    return discs, npass, False, passed  # (the flag a parked game takes along)


def new_mark(events, discs, passed, npass):
    """This build: the pass noted as the disc count; the count of a game that
    ends on a handed-over pass is corrected after the loop."""
    mark = discs if passed else 0xFFFFFFFF
    ended = False
    for has_move in events:
        if not has_move:
            if mark == discs or discs == 64:
                ended = True
                break
            mark, npass = discs, npass + 1
        else:
            discs += 1
    if ended and mark == discs:
        npass -= 1
    return discs, npass, ended, None if ended else mark == discs


def test_pass_flag_as_a_disc_count():
    """Every sequence of up to 9 plies (a move / no move each) from boards of
    0, 4, 60, 62, 63 and 64 discs, entered with and without a pass pending (a
    parked game comes back with its flag): the same end, the same counts.  A
    move on a full board cannot happen, and a full board is never passed to."""
    for discs0, passed0, n in itertools.product((0, 4, 60, 62, 63, 64), (False, True), range(1, 10)):
        if passed0 and discs0 == 64:
            continue
        for events in itertools.product((False, True), repeat=n):
            d, ok = discs0, True
            for e in events:
                ok &= not (e and d == 64)
                d += e
            if ok:
                assert old_flag(events, discs0, passed0, 3) == new_mark(events, discs0, passed0, 3), (discs0, passed0, events)


def rows3():
    """All 3^8 contents of a row as (P, O) bit masks."""
    for cells in itertools.product((0, 1, 2), repeat=8):
        yield (sum(1 << i for i, c in enumerate(cells) if c == 1), sum(1 << i for i, c in enumerate(cells) if c == 2))


def east_run_plain(P, O):
    """Opponent discs on the inner files in runs that start right east of a P disc."""
    A = 0
    for i in range(8):
        if P >> i & 1:
            j = i + 1
            while j < 8 and (O & INNER) >> j & 1:
                A |= 1 << j
                j += 1
    return A


def test_east_reach_from_the_carry_sum_rows():
    """(A0 << 1) & empty == sum & ~(P << 1) & empty with sum = Oi + (P << 1):
    every row content.  (So the shift of A0 can go only if P << 1 is at hand.)"""
    for P, O in rows3():
        Oi, Q = O & INNER, P << 1
        total = Oi + Q
        A0 = Oi & ~total
        assert A0 == east_run_plain(P, O)
        empty = ~(P | O) & 0xFF
        assert (A0 << 1) & empty == total & ~Q & empty, (P, O)


def test_east_reach_from_the_carry_sum_boards():
    """The same on whole boards (rows side by side: a carry must not cross a
    row, a disc on file h shifts onto file a of the next row)."""
    parts = [sc.edges()[:2], sc.lopsided(8), sc.lopsided(12), sc.uniform(20), sc.uniform(40)]
    b = np.concatenate([p[0] for p in parts])
    black, white = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])
    for P, O in ((black, white), (white, black)):
        Oi, Q = O & INNER_FILES, P << np.uint64(1)
        total = Oi + Q  # (uint64: wraps like the kernel's add)
        A0 = Oi & ~total
        empty = ~(P | O)
        assert ((A0 << np.uint64(1)) & empty == total & ~Q & empty).all()
        rows_P = P.view(np.uint8).reshape(-1)
        rows_O = O.view(np.uint8).reshape(-1)
        want = np.array([east_run_plain(int(p), int(o)) for p, o in zip(rows_P, rows_O)], np.uint8)
        assert (A0.view(np.uint8).reshape(-1) == want).all()


def test_tool_prices_vop3_fast_forms_as_fast():
    """tools/valu_mix.py: v_add_u32 / v_mov_b32 written in VOP3 are fast
    instructions in a VOP3 encoding, not slow ones."""
    spec = importlib.util.spec_from_file_location("valu_mix", os.path.join(ROOT, "tools", "valu_mix.py"))
    vm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vm)
    for op in ("v_add_u32_e64", "v_mov_b32_e64"):
        assert vm.cycles(op) == vm.FAST_CYC and vm.cycles_mixed(op) == vm.MIXED_FAST_VOP3
    assert vm.cycles_mixed("v_add_u32_e32") == vm.MIXED_FAST_E32
    assert vm.cycles("v_bfe_u32") > 4.0
