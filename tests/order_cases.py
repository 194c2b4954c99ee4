"""Inputs of the ordered searches' comparisons (tests/test_gpu_order.py, and the
host builds' driver tools/diag/order_host_check.py): each computed once per
process from the existing case modules and left read-only.

    mid(depth)        the checker's midgame subset of tests/test_gpu_search.py
                      (depth 1..5: 1024, 256, 64, 32, 8 roots of the 4,096)
    versus(depth)     the roots order 1 is compared with order 0 on: all 4,096
                      at every depth 1..6 (the hardest at depth 6 needs 1,239,852
                      nodes under order 0: under two seconds of one lane)
    endgame(e_max)    every position of solve_cases.cases() with <= e_max
                      empties, with the first 8 of the pool at 10 for e_max = 10
    depth1_ties()     the midgame roots whose depth-1 maximisers tie, with the
                      per-root flag "the lowest maximiser is in a LATER static
                      class than another maximiser" (what the root tie rule is for)
    two_empties()     64 roots at two empties, depth 2, with the same flag
    mobility_ties(d, k)  the roots among the first k where the MOBILITY-ordered root of a depth-d search meets a
                      higher-square maximiser first: the lower one is re-searched from alpha - 1
    PLAY              the two 128-game launches of the play comparison
"""
import functools

import numpy as np

import oracle
import play_ref
import search_ref
import solve_cases
import solve_ref
import tree_cases

TABLES, BOTH = tree_cases.TABLES, tree_cases.BOTH
MID = {1: 1024, 2: 256, 3: 64, 4: 32, 5: 8}  # tests/test_gpu_search.py's MID_CASES
VERSUS = {1: 4096, 2: 4096, 3: 4096, 4: 4096, 5: 4096, 6: 4096}
# The depth-5 node sum of the 4,096 roots, order 1 over order 0, default table:
# the host build (tools/diag/search_host, tools/diag/order_host_check.py ratio)
# counts 21,730,790 / 44,045,402 = 0.4934; the bound is that, rounded up to the
# next 0.05.  Node counts are exact functions of the position, so the GPU
# reproduces the host's.
DEPTH5_HOST_NODES = {0: 44045402, 1: 21730790}
DEPTH5_RATIO_BOUND = 0.50

# include/othello_order.h rule 3: the static classes, first to last (the eval's regions 0, 3, 4, 7, 6, 5, 1, 2)
CLASSES = (0x8100000000000081, 0x2400810000810024, 0x1800008181000018, 0x0000183C3C180000, 0x0000240000240000,
           0x003C424242423C00, 0x4281000000008142, 0x0042000000004200)
assert sum(CLASSES) == (1 << 64) - 1
CLASS_OF = np.array([[k for k, m in enumerate(CLASSES) if m >> s & 1][0] for s in range(64)])


def _frozen(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def mid(depth):
    g = tree_cases.midgame()
    return g["boards"][:MID[depth]], g["turn"][:MID[depth]]


@functools.lru_cache(maxsize=None)
def mid_reference(depth, table):
    """The checker's (value, best_move) of mid(depth)."""
    b, t = mid(depth)
    v, m, _ = search_ref.search(b, t, depth, TABLES[table])
    return _frozen(v, m)


def versus(depth):
    g = tree_cases.midgame()
    return g["boards"][:VERSUS[depth]], g["turn"][:VERSUS[depth]]


@functools.lru_cache(maxsize=None)
def endgame(e_max):
    cs = solve_cases.cases()
    bs = [cs[e]["boards"] for e in sorted(cs) if e <= e_max]
    ts = [cs[e]["turn"] for e in sorted(cs) if e <= e_max]
    if e_max >= 10:
        b, t = solve_cases.ladder(10, 8)
        bs.append(b)
        ts.append(t)
    return _frozen(np.concatenate(bs), np.concatenate(ts))


@functools.lru_cache(maxsize=None)
def special():
    """(boards, turn) of every forced-pass and game-over root of solve_cases.cases() (0..9 empties)."""
    cs = solve_cases.cases()
    sel = {e: cs[e]["forced_pass"] | cs[e]["over"] for e in cs}
    return _frozen(np.concatenate([cs[e]["boards"][sel[e]] for e in sorted(cs)]),
                   np.concatenate([cs[e]["turn"][sel[e]] for e in sorted(cs)]))


@functools.lru_cache(maxsize=None)
def special_reference(table):
    """The checker's depth-3 (value, best_move) of special()."""
    b, t = special()
    v, m, _ = search_ref.search(b, t, 3, TABLES[table])
    return _frozen(v, m)


@functools.lru_cache(maxsize=None)
def single_move_roots():
    """(boards, turn, square) of roots whose mover has exactly one move: the midgame sample's, and others of
    the solver's pool at 10..16 empties."""
    g, p = tree_cases.midgame(), solve_cases.pool()
    b = np.concatenate([g["boards"]] + [p[e]["boards"] for e in range(10, 17)])
    t = np.concatenate([g["turn"]] + [p[e]["turn"] for e in range(10, 17)])
    own = oracle.legal(b, t)
    one = np.nonzero((own != 0) & ((own & (own - np.uint64(1))) == 0))[0][:36]
    sq = np.array([int(x).bit_length() - 1 for x in own[one]], np.uint8)
    return _frozen(b[one], t[one], sq)


def _later_class(idx, sq, hit, n):
    """Per root: among the maximisers (hit), the lowest square's class comes
    after another maximiser's."""
    low = np.full(n, 255, np.int64)
    np.minimum.at(low, idx[hit], sq[hit].astype(np.int64))
    first = np.full(n, 99, np.int64)
    np.minimum.at(first, idx[hit], CLASS_OF[sq[hit]])
    has = low < 64
    out = np.zeros(n, bool)
    out[has] = CLASS_OF[low[has]] > first[has]
    return low, out


@functools.lru_cache(maxsize=None)
def depth1_ties(table="default"):
    """(boards, turn, value, best_move, later_class) of the midgame roots whose
    depth-1 maximisers tie; the values from the oracle's evaluate of the
    children (no child of these roots is a finished game)."""
    g = tree_cases.midgame()
    b, t = g["boards"], g["turn"]
    idx, sq = solve_ref._bits(oracle.legal(b, t))
    kids = oracle.step(b[idx], t[idx], sq)["boards"]
    assert (oracle.result(kids)["terminal"] == 0).all()
    ev = oracle.evaluate(kids, t[idx], TABLES[table]).astype(np.int64)
    best = np.full(len(t), -(1 << 40), np.int64)
    np.maximum.at(best, idx, ev)
    hit = ev == best[idx]
    low, later = _later_class(idx, sq, hit, len(t))
    tied = np.bincount(idx[hit], minlength=len(t)) > 1
    return _frozen(b[tied], t[tied], best[tied].astype(np.int32), low[tied].astype(np.uint8), later[tied])


@functools.lru_cache(maxsize=None)
def two_empties():
    """(boards, turn, value, best_move, later_class) of the first 64 roots of the
    solver's pool at two empties, depth 2: every move's value from the
    exhaustive solver of its child."""
    p = solve_cases.pool()[2]
    b, t = p["boards"][:64], p["turn"][:64]
    v, m, _ = search_ref.search(b, t, 2, TABLES["default"])
    idx, sq = solve_ref._bits(oracle.legal(b, t))
    kids = oracle.step(b[idx], t[idx], sq)["boards"]
    kv = -search_ref.T * solve_ref.solve(kids, (3 - t[idx]).astype(np.uint8))[0].astype(np.int64)
    hit = kv == v.astype(np.int64)[idx]
    low, later = _later_class(idx, sq, hit, len(t))
    movers = np.bincount(idx, minlength=len(t)) > 0
    assert (low[movers] == m[movers]).all()
    return _frozen(b, t, v, m, later)


def root_move_values(boards, turn, depth, table):
    """(idx, sq, value): for every legal root move of every root, -S(child, opponent, depth - 1) scored for the
    ROOT's mover, by tests/search_ref.py's own level-by-level minimax restated with the root mover carried along
    (search_ref.search scores leaves for the mover of the position it is given, so it cannot be asked about a
    child)."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = solve_ref.mover(turn)
    ridx, rsq = solve_ref._bits(oracle.legal(b, t))
    st = oracle.step(b[ridx], t[ridx], rsq)
    b, root = st["boards"], t[ridx]
    t = (3 - root).astype(np.uint8)
    d = np.full(len(b), depth - 1, np.int64)
    parent, levels = np.arange(len(b)), []
    while len(b):
        own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
        diff = oracle.result(b)["diff"].astype(np.int64) * np.where(t == 1, 1, -1)
        ev = oracle.evaluate(b, root, TABLES[table]).astype(np.int64) * np.where(t == root, 1, -1)
        over = (own == 0) & (opp == 0)
        leaf = ~over & (d == 0)
        passes, inner = ~over & ~leaf & (own == 0), ~over & ~leaf & (own != 0)
        levels.append((parent, over | leaf, np.where(over, search_ref.T * diff, np.where(leaf, ev, 0)), len(b)))
        ci, csq = solve_ref._bits(np.where(inner, own, np.uint64(0)))
        kids = oracle.step(b[ci], t[ci], csq)["boards"]
        pi = np.nonzero(passes)[0]
        b, t, root, d, parent = (np.concatenate([kids, b[pi]]), np.concatenate([3 - t[ci], 3 - t[pi]]).astype(np.uint8),
                                 np.concatenate([root[ci], root[pi]]), np.concatenate([d[ci] - 1, d[pi]]),
                                 np.concatenate([ci, pi]))
    lo, cval, cpar = -(1 << 40), None, None
    for par, final, static, n in reversed(levels):
        val = np.where(final, static, lo).astype(np.int64)
        if cval is not None and len(cval):
            np.maximum.at(val, cpar, -cval)
        cval, cpar = val, par
    return ridx, rsq, -cval


@functools.lru_cache(maxsize=None)
def mobility_ties(depth, roots):
    """(boards, turn, value, best_move) of the roots among the first `roots` midgame ones where, at `depth` >= 3,
    the mobility-ordered root (include/othello_order.h rule 2: fewest opponent moves after the move, minus 3 for a
    corner, ties to the lowest square) meets a maximiser at a HIGHER square before the lowest maximiser: the lower
    one is then searched from alpha - 1 and must take the move over on a score of exactly alpha."""
    g = tree_cases.midgame()
    b, t = g["boards"][:roots], g["turn"][:roots]
    idx, sq, val = root_move_values(b, t, depth, "default")
    best = np.full(len(t), -(1 << 40), np.int64)
    np.maximum.at(best, idx, val)
    hit = val == best[idx]
    low = np.full(len(t), 255, np.int64)
    np.minimum.at(low, idx[hit], sq[hit].astype(np.int64))
    kids = oracle.step(b[idx], t[idx], sq)["boards"]
    mob = np.array([bin(int(x)).count("1") for x in oracle.legal(kids, (3 - t[idx]).astype(np.uint8))], np.int64)
    key = (mob + np.where(CLASS_OF[sq] == 0, 0, 3)) * 64 + sq
    low_key = np.full(len(t), 1 << 30, np.int64)
    np.minimum.at(low_key, idx[hit & (sq == low[idx])], key[hit & (sq == low[idx])])
    earlier = hit & (sq > low[idx]) & (key < low_key[idx])
    pick = np.zeros(len(t), bool)
    pick[idx[earlier]] = True
    return _frozen(b[pick], t[pick], best[pick].astype(np.int32), low[pick].astype(np.uint8))


# the play comparison: 256 games in all, depths (4, 3), the last eight empties exact, moves recorded; half from
# the opening, half from midgame starts (the checker's unpruned endgames make its share of the time: about 50 s a half)
PLAY = {
    "open128": dict(n=128, seed=201, game_id0=0, tables=("default", "rng7"), depth=(4, 3), exact=8, n_rand=(4, 4),
                    swap=True, start=None),
    "mid128": dict(n=128, seed=202, game_id0=5, tables=("default", "rng7"), depth=(4, 3), exact=8, n_rand=(0, 0),
                   swap=True, start="mid"),
}


def play_starts(case):
    if PLAY[case]["start"] is None:
        return None, None
    g = tree_cases.midgame()
    return g["boards"][:PLAY[case]["n"]], g["turn"][:PLAY[case]["n"]]


@functools.lru_cache(maxsize=None)
def play_reference(case):
    """play_ref.play's games of a PLAY case."""
    c = PLAY[case]
    b, t = play_starts(case)
    wa, wb = TABLES[c["tables"][0]], TABLES[c["tables"][1]]
    r = play_ref.play(c["n"], c["seed"], play_ref.search_chooser(wa, wb, c["depth"][0], c["depth"][1], c["exact"]),
                      game_id0=c["game_id0"], n_rand_a=c["n_rand"][0], n_rand_b=c["n_rand"][1], swap=c["swap"],
                      start=b, start_turn=t)
    for v in r.values():
        v.setflags(write=False)
    return r
