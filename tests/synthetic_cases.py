"""Positions no game from the opening reaches, for the searches' tests: seeded
numpy boards classified with the C oracle (legal / step / result), each family
computed once per process and returned read-only.  No fixture file.

Every family is (boards (n, 2) uint64, turn (n,) uint8) with both movers present:

    uniform(e)   e empty squares chosen uniformly, every other square Black or White with probability 1/2
    lopsided(e)  the same with Black's share cycling through 0.03, 0.97, 0.1, 0.9
    centre(e)    the four centre squares always among the empties
    islands(e)   a 2x3 block of empties in a corner, its long side on an edge (e >= 6): the corner and the edge
                 square next to it have no occupied neighbour.  Below six empties two such squares do not exist
                 (a corner needs its three neighbours empty, and none of those has all of its own inside the
                 four), so islands(4) and islands(5) have the empty 2x2 corner block: one such square.  Black's share
                 alternates between 0.2 and 0.8, and of the boards drawn those are kept from which the oracle's walk
                 reaches a game-over with an empty square left (one in 11, 4 and 2 at 4, 6 and 8 empties; with even
                 shares one in 128, 32 and 4).  32 roots at 8 empties and above, where that walk is the cost.
    wide(k)      k roots of a hill climb on the mover's number of moves, each with at least WIDE_MIN moves
    edges()      a fixed list (empty board, full boards, wipe-outs, ...), each entry with both turns; also names
    images(b, t) the 8 symmetries of each root times the colour swap (turn swapped): 16 images per root, with
                 each image's square permutation
"""
import functools

import numpy as np

import line_ref
import moves_ref
import oracle
import play_cases
import play_ref
import search_ref
import solve_ref
import tree_cases
import window_ref
from solve_ref import _bits, empties, mover

SEED = 0x5E7C
ROOTS = 128
SHARES = (0.03, 0.97, 0.1, 0.9)
ISLAND_SHARES, ISLANDS_DEEP_ROOTS = (0.2, 0.8), 32
CENTRE = (27, 28, 35, 36)
FULL = (1 << 64) - 1
WIDE_MIN, WIDE_CHAINS, WIDE_STEPS = 28, 64, 6000
_FAMILY = {"uniform": 1, "lopsided": 2, "centre": 3, "islands": 4, "wide": 5}


def popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(len(x), 8), axis=1).sum(1).astype(np.int64)


def _mask(squares):
    v = 0
    for s in squares:
        v |= 1 << int(s)
    return v


def _freeze(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def _fill(rng, empty, share):
    """(black, white) ints: every square outside `empty` Black with probability `share`."""
    black = _mask(np.nonzero(rng.random(64) < share)[0]) & ~empty & FULL
    return black, FULL & ~empty & ~black


def _draw(rng, n, e, fixed_of, share_of, turn_of):
    boards, turn = np.zeros((n, 2), np.uint64), np.zeros(n, np.uint8)
    for i in range(n):
        fixed = fixed_of(rng)
        rest = [s for s in rng.permutation(64) if s not in fixed][:e - len(fixed)]
        boards[i] = _fill(rng, _mask(fixed) | _mask(rest), share_of(i))
        turn[i] = turn_of(i)
    return boards, turn


def _family(name, e, fixed_of, share_of, turn_of):
    return _freeze(*_draw(np.random.default_rng([SEED, _FAMILY[name], e]), ROOTS, e, fixed_of, share_of, turn_of))


@functools.lru_cache(maxsize=None)
def uniform(e):
    return _family("uniform", e, lambda rng: (), lambda i: 0.5, lambda i: 1 + i % 2)


@functools.lru_cache(maxsize=None)
def lopsided(e):
    # (the share has period 4, the mover period 8: every share meets both movers)
    return _family("lopsided", e, lambda rng: (), lambda i: SHARES[i % 4], lambda i: 1 + (i // 4) % 2)


@functools.lru_cache(maxsize=None)
def centre(e):
    assert e >= 4
    return _family("centre", e, lambda rng: CENTRE, lambda i: 0.5, lambda i: 1 + i % 2)


def _corner_block(rng, long_side):
    """A 2 x long_side block of squares in a random corner, the long side along a random edge."""
    fx, fy, tr = (int(v) for v in rng.integers(0, 2, 3))
    out = []
    for y in range(2):
        for x in range(long_side):
            xx, yy = (7 - x if fx else x), (7 - y if fy else y)
            if tr:
                xx, yy = yy, xx
            out.append(xx + 8 * yy)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def islands(e):
    assert 4 <= e <= 8  # (the walk below is the whole game tree)
    rng = np.random.default_rng([SEED, _FAMILY["islands"], e])
    n = ROOTS if e <= 6 else ISLANDS_DEEP_ROOTS
    boards, turn = np.zeros((0, 2), np.uint64), np.zeros(0, np.uint8)
    while len(turn) < n:
        b, t = _draw(rng, 64, e, lambda r: _corner_block(r, 3 if e >= 6 else 2), lambda i: ISLAND_SHARES[i % 2],
                     lambda i: 1 + (i // 2) % 2)
        keep = census(b, t, 2 * e)[2]  # (no line of play is longer: a pass is followed by a move)
        boards, turn = np.concatenate([boards, b[keep]]), np.concatenate([turn, t[keep]])
    return _freeze(boards[:n], turn[:n])


def cut_off(boards):
    """Per root: the number of empty squares none of whose neighbours is occupied."""
    b = np.ascontiguousarray(boards, np.uint64)
    occ = b[:, 0] | b[:, 1]
    not_a, not_h, all_ = np.uint64(0xFEFEFEFEFEFEFEFE), np.uint64(0x7F7F7F7F7F7F7F7F), np.uint64(FULL)
    near = np.zeros_like(occ)
    for sh, up, down in ((1, not_a, not_h), (9, not_a, not_h), (7, not_h, not_a), (8, all_, all_)):
        near |= ((occ << np.uint64(sh)) & up) | ((occ >> np.uint64(sh)) & down)
    return popcount(~occ & ~near)


@functools.lru_cache(maxsize=None)
def wide_climb():
    """(boards, turn, moves) of every chain's end: WIDE_CHAINS seeded chains from random three-valued boards,
    1 or 2 squares re-drawn per step, a step kept when the mover has no fewer moves than before."""
    rng = np.random.default_rng([SEED, _FAMILY["wide"]])
    state = rng.integers(0, 3, (WIDE_CHAINS, 64))  # 0 empty, 1 Black, 2 White
    turn = (1 + np.arange(WIDE_CHAINS) % 2).astype(np.uint8)
    weight = np.uint64(1) << np.arange(64, dtype=np.uint64)

    def pack(s):
        return np.stack([((s == 1) * weight).sum(1, dtype=np.uint64), ((s == 2) * weight).sum(1, dtype=np.uint64)], 1)

    moves = popcount(oracle.legal(pack(state), turn))
    rows = np.arange(WIDE_CHAINS)
    for _ in range(WIDE_STEPS):
        cand = state.copy()
        for k in range(2):
            on = rng.random(WIDE_CHAINS) < (1.0 if k == 0 else 0.5)
            sq = rng.integers(0, 64, WIDE_CHAINS)
            val = rng.integers(0, 3, WIDE_CHAINS)
            cand[rows[on], sq[on]] = val[on]
        got = popcount(oracle.legal(pack(cand), turn))
        keep = got >= moves
        state[keep], moves[keep] = cand[keep], got[keep]
    return _freeze(pack(state), turn, moves)


@functools.lru_cache(maxsize=None)
def wide(k=16):
    """The first k chain ends with at least WIDE_MIN moves, Black and White to move alternating while both last."""
    b, t, moves = wide_climb()
    ok = np.nonzero(moves >= WIDE_MIN)[0]
    black, white = ok[t[ok] == 1], ok[t[ok] == 2]
    order = [x for pair in zip(black, white) for x in pair]
    order += [x for x in ok if x not in order]
    idx = np.array(order[:k], np.int64)
    return _freeze(b[idx], t[idx])


def wide_max():
    return int(wide_climb()[2].max())


# name, black, white; each entry is a root with Black and with White to move
EDGES = (
    ("empty", 0, 0),
    ("one disc", 1 << 27, 0),
    ("two adjacent discs", (1 << 27) | (1 << 28), 0),
    ("full black", FULL, 0),
    ("full white", 0, FULL),
    ("full 63:1", FULL ^ 1, 1),
    ("full 32:32", 0x00000000FFFFFFFF, 0xFFFFFFFF00000000),
    # the 2x2 corner block empty, Black off every line that leaves it: nobody ever moves
    ("four unplayable empties", _mask((20, 21, 29)), FULL & ~_mask((0, 1, 8, 9)) & ~_mask((20, 21, 29))),
    # Black's only move, a1, flips White's only disc (b1); h1 stays empty for ever: 63 discs to none
    ("wipe-out", FULL & ~_mask((0, 1, 7)), 1 << 1),
    # a1 is the one empty square: Black (b1 and a few inner discs) cannot flank anything from it, White flanks b1
    ("pass then the last move", _mask((1, 12, 13, 20, 21, 22)), FULL & ~_mask((0, 1, 12, 13, 20, 21, 22))),
)


@functools.lru_cache(maxsize=None)
def edges():
    """(boards, turn, names): entry i of EDGES is rows 2i (Black to move) and 2i + 1 (White)."""
    boards = np.array([[b, w] for _, b, w in EDGES for _ in (1, 2)], np.uint64)
    turn = np.array([t for _ in EDGES for t in (1, 2)], np.uint8)
    return _freeze(boards, turn) + (tuple(n for n, _, _ in EDGES for _ in (1, 2)),)


def edge(name, turn):
    """The row of an edge entry."""
    return 2 * [n for n, _, _ in EDGES].index(name) + (turn - 1)


@functools.lru_cache(maxsize=None)
def _permutations():
    """(8, 64): where tree_cases.symmetries sends each square."""
    out = np.zeros((8, 64), np.int64)
    for s in range(64):
        for k, v in enumerate(tree_cases.symmetries(1 << s)):
            out[k, s] = v.bit_length() - 1
    return out


def images(boards, turn):
    """(boards (16 n, 2), turn (16 n,), perm (16 n, 64)): root i's images are rows 16 i .. 16 i + 15, the eight
    symmetries and then the same eight with the colours and the mover swapped; perm[j][s] is the square of
    image j that square s of its root went to."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    t = mover(turn)
    rows, turns = [], []
    for i in range(len(b)):
        bl, wh = tree_cases.symmetries(int(b[i, 0])), tree_cases.symmetries(int(b[i, 1]))
        rows += [[x, y] for x, y in zip(bl, wh)] + [[y, x] for x, y in zip(bl, wh)]
        turns += [int(t[i])] * 8 + [3 - int(t[i])] * 8
    perm = np.tile(np.concatenate([_permutations(), _permutations()]), (len(b), 1))
    return _freeze(np.array(rows, np.uint64).reshape(-1, 2), np.array(turns, np.uint8), perm)


def root_kinds(boards, turn):
    """(forced_pass, over) of the roots."""
    t = mover(turn)
    own, opp = oracle.legal(boards, t), oracle.legal(boards, (3 - t).astype(np.uint8))
    return (own == 0) & (opp != 0), (own == 0) & (opp == 0)


def census(boards, turn, plies):
    """Per root, walking the tree a level at a time as tree_cases.expected_noroom does: (passes, finals,
    ends_with_empties, nodes) = the number of nodes below the root and above level `plies` that must pass, the
    number of game-over nodes at levels 1..plies, whether one of those has an empty square left, and the number
    of nodes at levels 1..plies.  A pass is one level, as in the split trees."""
    b = np.ascontiguousarray(boards, np.uint64).reshape(-1, 2)
    n = len(b)
    t = mover(turn)
    root = np.arange(n)
    passes, finals, with_empties = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    nodes = np.zeros(n, np.int64)
    for level in range(plies + 1):
        own, opp = oracle.legal(b, t), oracle.legal(b, (3 - t).astype(np.uint8))
        over = (own == 0) & (opp == 0)
        must_pass = (own == 0) & (opp != 0)
        if level >= 1:
            np.add.at(nodes, root, 1)
            np.add.at(finals, root[over], 1)
            with_empties[root[over & (empties(b) > 0)]] = True
            if level < plies:
                np.add.at(passes, root[must_pass], 1)
        if level == plies:
            break
        idx, sq = _bits(np.where(over, np.uint64(0), own))
        kids = oracle.step(b[idx], t[idx], sq)["boards"]
        pi = np.nonzero(must_pass)[0]
        b, t, root = (np.concatenate([kids, b[pi]]), np.concatenate([3 - t[idx], 3 - t[pi]]).astype(np.uint8),
                      np.concatenate([root[idx], root[pi]]))
        if len(b) == 0:
            break
    return passes, finals, with_empties, nodes


# ---------------------------------------------------------------- the cases both test files run
# (inputs and the checkers' answers, computed once per process; tests/test_synthetic_cases.py runs the host
# drivers on them, tests/test_gpu_synthetic.py the kernels)
T = search_ref.T
TABLES = play_cases.TABLES
ALL_TABLES = ("default", "rng7", "extreme")
FAMILIES = {"uniform": uniform, "lopsided": lopsided, "centre": centre, "islands": islands}
# name -> (family, empties, roots): 128 roots at 4 and 6 empties; at 8 the checker takes 4.4 s for 128 uniform
# roots, so 32, except the lopsided ones (0.3 s for 128: most lines end early)
SOLVER = {"%s%d" % (f, e): (f, e, 32 if e == 8 and f != "lopsided" else ROOTS)
          for f in FAMILIES for e in (4, 6, 8)}
# name -> (source, depth, roots, tables, splits); a source "family:e" or "wide".  At depth 8 with 8 empties the
# horizon is never reached: the reference is T times the solver's.
SEARCH = {
    "uniform20": ("uniform:20", 3, 64, ALL_TABLES, (1, 2)),
    "uniform40": ("uniform:40", 3, 64, ALL_TABLES, (1, 2)),
    "uniform52": ("uniform:52", 3, 64, ALL_TABLES, (1, 2)),
    "wide3": ("wide", 3, 16, ALL_TABLES, (1, 2)),
    "uniform30": ("uniform:30", 4, 16, ALL_TABLES, (1, 2, 3)),
    "lopsided8": ("lopsided:8", 8, ROOTS, ALL_TABLES, (1, 2, 3)),
    "islands8": ("islands:8", 8, 32, ALL_TABLES, (1, 2, 3)),
}
# the split search alone: depth 9 with split 4 at 6 and 8 empties (passes and game-overs inside the split
# plies; the reference is T times the solver's), and depth 5 with split 4 on two wide roots (the checker
# expands 3.6 M nodes a root)
TREE = {
    "lopsided6_d9": ("lopsided:6", 9, ROOTS, ("default",), (4,)),
    "lopsided8_d9": ("lopsided:8", 9, ROOTS, ("default",), (4,)),
    "islands6_d9": ("islands:6", 9, ROOTS, ("default",), (4,)),
    "islands8_d9": ("islands:8", 9, 32, ("default",), (4,)),
    "wide5": ("wide", 5, 2, ("default",), (4,)),
}
NOROOM_DEPTH, NOROOM_SLAB, NOROOM_SPLITS = 10, 64, (2, 3)
# name -> the games: 64 starts, player A on "default", B on "rng7", colours drawn, no random moves
PLAY = {"%s_d%d%d_x%d" % (src.replace(":", ""), d[0], d[1], x): dict(start=src, depth=d, exact=x, seed=200 + k)
        for k, (src, d, x) in enumerate((s, d, x) for s in ("uniform:20", "lopsided:12") for d in ((2, 1), (3, 3))
                                        for x in (0, 6))}
PLAY_GAMES = 64
TIE_ROOTS = 8  # of each kind


def _source(src, k):
    if src == "wide":
        b, t = wide()
    else:
        f, e = src.split(":")
        b, t = FAMILIES[f](int(e))
    assert len(t) >= k
    return b[:k], t[:k]


def solver_inputs(name):
    f, e, k = SOLVER[name]
    return _source("%s:%d" % (f, e), k)


@functools.lru_cache(maxsize=None)
def _solved(src, k):
    v, m, passes = solve_ref.solve(*_source(src, k))
    return _freeze(v.astype(np.int64), m) + (passes,)


def solver_reference(name):
    """solve_ref.solve's (value int64, best_move, inner_passes) of a solver case."""
    f, e, k = SOLVER[name]
    return _solved("%s:%d" % (f, e), k)


def search_case(name):
    return SEARCH[name] if name in SEARCH else TREE[name]


def search_inputs(name):
    src, _, k, _, _ = search_case(name)
    return _source(src, k)


@functools.lru_cache(maxsize=None)
def search_reference(name, table):
    """The checker's (value int64, best_move) of a search case."""
    src, depth, k, _, _ = search_case(name)
    b, t = _source(src, k)
    if src != "wide" and depth >= int(src.split(":")[1]) <= 9:
        v, m, _ = _solved(src, k)
        return _freeze(T * v, m)
    v, m, _ = search_ref.search(b, t, depth, TABLES[table])
    return _freeze(v.astype(np.int64), m)


@functools.lru_cache(maxsize=None)
def noroom_case():
    """(boards, turn, value, best_move): the wide roots, whose second level never fits 64 nodes, mixed with 32
    roots of four empties, whose whole tree does; the answers (depth 10: T times the solver's) of the latter,
    zero and 255 for the former."""
    wb, wt = wide()
    ub, ut = _source("uniform:4", 32)
    v, m, _ = _solved("uniform:4", 32)
    order = np.random.default_rng([SEED, 6]).permutation(len(wt) + len(ut))
    return _freeze(np.concatenate([wb, ub])[order], np.concatenate([wt, ut])[order],
                   np.concatenate([np.zeros(len(wt), np.int64), T * v])[order],
                   np.concatenate([np.full(len(wt), 255, np.uint8), m])[order])


def play_starts(name):
    return _source(PLAY[name]["start"], PLAY_GAMES)


@functools.lru_cache(maxsize=None)
def play_reference(name):
    c = PLAY[name]
    b, t = play_starts(name)
    r = play_ref.play(PLAY_GAMES, c["seed"], play_ref.search_chooser(TABLES["default"], TABLES["rng7"], c["depth"][0],
                                                                     c["depth"][1], c["exact"]),
                      swap=True, start=b, start_turn=t)
    for v in r.values():
        v.setflags(write=False)
    return r


def _tied(boards, turn, answer):
    """Which roots tie, by the checker alone: `answer(boards, turn)` -> best moves, run on every root's 16
    images; a root has two maximisers or more exactly when the images' lowest maximisers, taken back to the
    root's squares, are not all one square (the half turn reverses the order of any two squares)."""
    ib, it, perm = images(boards, turn)
    m = answer(ib, it).astype(np.int64)
    back = np.argsort(perm, axis=1)  # back[j][s'] = the root's square that image j shows at s'
    home = np.where(m < 64, back[np.arange(len(m)), np.minimum(m, 63)], m).reshape(-1, 16)
    return (home != home[:, :1]).any(1)


@functools.lru_cache(maxsize=None)
def tie_roots(kind):
    """The first TIE_ROOTS tied roots of uniform(6)'s first 64 under the solver ("solve"), or of wide(32) under
    the depth-2 search on the "extreme" table ("search"), with their 16 images and the checker's answers on
    those: (boards, turn, value int64, best_move) of 16 * TIE_ROOTS rows."""
    if kind == "solve":
        b, t = _source("uniform:6", 64)
        answer = lambda bb, tt: solve_ref.solve(bb, tt)  # noqa: E731
    else:
        b, t = wide(32)
        answer = lambda bb, tt: search_ref.search(bb, tt, TIE_DEPTH, TABLES[TIE_TABLE])  # noqa: E731
    keep = np.nonzero(_tied(b, t, lambda bb, tt: answer(bb, tt)[1]))[0][:TIE_ROOTS]
    ib, it, _ = images(b[keep], t[keep])
    r = answer(ib, it)
    return _freeze(ib, it, r[0].astype(np.int64), r[1])


TIE_DEPTH, TIE_TABLE = 2, "extreme"


# ---------------------------------------------------------------- windows, per-move values and lines
# (ops.solve(window=, wld=), ops.solve_moves / search_moves, ops.solve_line / search_line: two batches with
# the answers of tests/window_ref.py, moves_ref.py and line_ref.py, each computed once per process)
X_ROOTS, S_ROOTS, X_MAX_EMPTIES = 32, 16, 12
S_SOURCES = ("uniform:20", "uniform:40", "uniform:52", "lopsided:8", "lopsided:12", "islands:6")
S_WIDE = 8
# (depth, table) of every search reference of batch S: the checkers take 6.1 s (line) and 2.9 s (rows) for one
# table at depth 4, under 1 s for all of depths 1 to 3
S_RUNS = tuple((d, table) for d in (1, 2, 3) for table in ALL_TABLES) + ((4, "default"),)
# depth 8 at 8 empties never meets the horizon: the first X_ROOTS roots of these, which batch X holds
FULL_DEPTH, FULL_DEPTH_CASES = 8, ("lopsided8", "islands8")


def _readonly(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def batch_x():
    """(boards, turn) of batch X: the first 32 roots of each of the twelve SOLVER cases, by name, then the rows
    of edges() with at most 12 empties; 398 positions."""
    eb, et, _ = edges()
    small = empties(eb) <= X_MAX_EMPTIES
    parts = [_source("%s:%d" % SOLVER[name][:2], X_ROOTS) for name in sorted(SOLVER)] + [(eb[small], et[small])]
    return _freeze(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def x_rows_of(name):
    """Where batch X holds a SOLVER case's 32 roots, or (name, turn) an edge: a slice, or an index."""
    if isinstance(name, tuple):
        eb, _, _ = edges()
        small = np.nonzero(empties(eb) <= X_MAX_EMPTIES)[0]
        return X_ROOTS * len(SOLVER) + int(np.nonzero(small == edge(*name))[0][0])
    k = sorted(SOLVER).index(name)
    return slice(X_ROOTS * k, X_ROOTS * (k + 1))


@functools.lru_cache(maxsize=None)
def x_line():
    """line_ref.exact of batch X."""
    return line_ref.exact(*batch_x())


@functools.lru_cache(maxsize=None)
def x_roots():
    """window_ref.roots of batch X: the exhaustive value of every root move."""
    return window_ref.roots(*batch_x())


@functools.lru_cache(maxsize=None)
def x_moves():
    """moves_ref.exact of batch X: (rows (n, 64), value, move)."""
    return _freeze(*moves_ref.exact(x_roots()))


@functools.lru_cache(maxsize=None)
def x_windows():
    """Batch X under the nine window families, built as window_ref.case_batch builds its batch: dict(boards,
    turn, alpha, beta, value, move, family (the index into window_ref.FAMILIES), root (the row of batch X))."""
    b, t = batch_x()
    r = x_roots()
    out = {k: [] for k in ("boards", "turn", "alpha", "beta", "value", "move", "family", "root")}
    for k, name in enumerate(window_ref.FAMILIES):
        lo, hi, keep = window_ref.family(name, r.value)
        lo, hi = np.where(keep, lo, window_ref.LO), np.where(keep, hi, window_ref.HI)
        v, m = window_ref.expect(r, lo, hi)
        for key, src in zip(out, (b, t, lo, hi, v, m, np.full(r.n, k), np.arange(r.n))):
            out[key].append(src[keep])
    return _readonly({k: np.concatenate(v) for k, v in out.items()})


def x_family(name):
    """The rows of x_windows() of one family."""
    return np.nonzero(x_windows()["family"] == window_ref.FAMILIES.index(name))[0]


@functools.lru_cache(maxsize=None)
def batch_s():
    """(boards, turn) of batch S: the first 16 roots of each of S_SOURCES, wide(8), every row of edges(); 124
    positions."""
    eb, et, _ = edges()
    parts = [_source(src, S_ROOTS) for src in S_SOURCES] + [wide(S_WIDE), (eb, et)]
    return _freeze(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def s_row_of(name, turn):
    """The row of batch S that holds an edge."""
    return S_ROOTS * len(S_SOURCES) + S_WIDE + edge(name, turn)


@functools.lru_cache(maxsize=None)
def s_line(depth, table):
    """line_ref.search of batch S."""
    return line_ref.search(*batch_s(), depth, TABLES[table])


@functools.lru_cache(maxsize=None)
def s_moves(depth, table):
    """moves_ref.search of batch S: (rows (n, 64), value, move)."""
    return _freeze(*moves_ref.search(*batch_s(), depth, TABLES[table]))


def exact_rows_times_t(rows, value, move):
    """What the search rows are where the horizon is never met: T times the exact rows."""
    return np.where(rows == moves_ref.NOT_A_MOVE, moves_ref.NOT_A_MOVE32, rows * T), value * T, move


@functools.lru_cache(maxsize=None)
def full_depth_case(name):
    """(boards, turn, exact line, exact (rows, value, move)) of a FULL_DEPTH_CASES entry, taken from batch X: at
    depth 8 the search line is that line with the value times T, the search rows exact_rows_times_t of those."""
    sel = x_rows_of(name)
    b, t = batch_x()
    assert (empties(b[sel]) <= FULL_DEPTH).all()
    return b[sel], t[sel], {k: v[sel] for k, v in x_line().items()}, tuple(v[sel] for v in x_moves())
