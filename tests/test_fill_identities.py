"""The reach and flips formulas of subproc_amd/csrc/bitboard.hpp that read the
Kogge-Stone fills G = A | P directly (no A = G & O), modelled in numpy uint64
operation by operation (same truth-table constants) and checked against a
naive 8x8 ray scan.  CPU only.

* reach (squares one step beyond an attached run, any content) and legal are
  equal to the scan's;
* the flips of every legal move, masked with the opponent's discs, are the
  scan's flips, and whatever else they hold are discs of the mover's own or
  the move square: place() ORs them into the mover and clears them from the
  opponent, so neither board changes.
"""
import numpy as np
import pytest

U = np.uint64
INNER = U(0x7E7E7E7E7E7E7E7E)
ALL = U(0xFFFFFFFFFFFFFFFF)
DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1)]  # +1 -1 +8 -8 +9 -9 +7 -7


# ---- the device primitives ------------------------------------------------
def bitop3(tt, a, b, c):
    """v_bitop3_b32's function: bit (4a + 2b + c) of tt, bitwise"""
    r = np.zeros_like(a)
    for i in range(8):
        if tt >> i & 1:
            r |= (a if i & 4 else ~a) & (b if i & 2 else ~b) & (c if i & 1 else ~c)
    return r


def sh(x, s, left):
    return x << U(s) if left else x >> U(s)


def and2(a, b):
    return bitop3(0xC0, a, b, b)


def or2(a, b):
    return bitop3(0xFC, a, b, b)


def or3(a, b, c):
    return bitop3(0xFE, a, b, c)


def bfi(m, a, b):
    return bitop3(0xCA, m, a, b)


def rev64(x):
    x = ((x >> U(1)) & U(0x5555555555555555)) | ((x & U(0x5555555555555555)) << U(1))
    x = ((x >> U(2)) & U(0x3333333333333333)) | ((x & U(0x3333333333333333)) << U(2))
    x = ((x >> U(4)) & U(0x0F0F0F0F0F0F0F0F)) | ((x & U(0x0F0F0F0F0F0F0F0F)) << U(4))
    return x.byteswap()


def east_run(src, oi):
    return bitop3(0x30, oi, (src << U(1)) + oi, (src << U(1)) + oi)


def pair_prop(s, pro):
    p2l = and2(pro, sh(pro, s, True))
    p4l = and2(p2l, sh(p2l, 2 * s, True))
    return dict(pro=pro, p2=(sh(p2l, s, False), p2l), p4=(sh(p4l, 3 * s, False), p4l))


def ks(s, left, src, q):
    """the fill and the source shifted one step (the first step's temporary)"""
    ps = sh(src, s, left)
    gen = bfi(q["pro"], ps, src)
    gen = bfi(q["p2"][left], sh(gen, 2 * s, left), gen)
    gen = bfi(q["p4"][left], sh(gen, 4 * s, left), gen)
    return gen, ps


def analyse(P, O):
    oi = and2(O, INNER)
    roi, rp = rev64(oi), rev64(P)
    props = {8: pair_prop(8, O), 9: pair_prop(9, oi), 7: pair_prop(7, oi)}
    a0 = east_run(P, oi)
    a1 = rev64(east_run(rp, roi))
    m = or2(sh(a0, 1, True), sh(a1, 1, False))
    G = {}
    for i, (s, left) in zip(range(2, 8), ((8, True), (8, False), (9, True), (9, False), (7, True), (7, False))):
        g, ps = ks(s, left, P, props[s])
        m = bitop3(0xF4, m, sh(g, s, left), ps)  # m | (sh(G) & ~sh(P))
        G[i] = g
    return dict(A0=a0, A1=a1, G=G, rP=rp, reach=m, legal=bitop3(0x04, P, m, O))


def ray_from(sq, dx, dy):
    r, x, y = 0, sq & 7, sq >> 3
    while True:
        x, y = x + dx, y + dy
        if not (0 <= x < 8 and 0 <= y < 8):
            return r
        r |= 1 << (x + 8 * y)


def rev_int(v):
    return int(f"{v:064b}"[::-1], 2)


# rows 0..2 = rays +8, +9, +7; rows 3..5 = rays -8, -9, -7 bit-reversed
RAYS = [[ray_from(sq, dx, dy) if row < 3 else rev_int(ray_from(sq, dx, dy)) for sq in range(64)]
        for row, (dx, dy) in enumerate([(0, 1), (1, 1), (-1, 1), (0, -1), (-1, -1), (1, -1)])]


def run_prefix(R, G, P):
    x = bitop3(0xB0, R, G, P)  # R & (~G | P)
    return bitop3(0x80, R, G, x - U(1))


def flips_col(sq, P, s):
    """flips of the move at sq for every position of the arrays, move bit included"""
    mv, rmv = np.full_like(P, U(1) << U(sq)), np.full_like(P, U(1) << U(63 - sq))
    R = [np.full_like(P, U(RAYS[row][sq])) for row in range(6)]
    G, rP = s["G"], s["rP"]
    ra0 = rev64(s["A0"])
    f = bitop3(0xBA, s["A1"], (mv << U(1)) + s["A1"], mv)
    fr = bitop3(0xBA, ra0, (rmv << U(1)) + ra0, rmv)
    f = or3(f, run_prefix(R[0], G[3], P), run_prefix(R[1], G[5], P))
    f = or2(f, run_prefix(R[2], G[7], P))
    fr = or3(fr, run_prefix(R[3], rev64(G[2]), rP), run_prefix(R[4], rev64(G[4]), rP))
    fr = or2(fr, run_prefix(R[5], rev64(G[6]), rP))
    return or2(f, rev64(fr))


# ---- the naive scan -------------------------------------------------------
def naive(P, O):
    """reach (N,) and flips (N, 64) by walking the 8x8 board square by square:
    from every square, along every direction, over opponent discs up to a disc
    of the mover's.  flips[:, sq] is what a move at sq would turn, whatever sq holds."""
    n = len(P)
    bits = (U(1) << np.arange(64, dtype=U))
    cell = np.where((P[:, None] & bits) != 0, 1, np.where((O[:, None] & bits) != 0, 2, 0)).astype(np.int8)
    flips = np.zeros((n, 64), U)
    for sq in range(64):
        x0, y0 = sq & 7, sq >> 3
        for dx, dy in DIRS:
            run = np.zeros(n, U)
            alive = np.ones(n, bool)
            found = np.zeros(n, bool)
            x, y = x0 + dx, y0 + dy
            while 0 <= x < 8 and 0 <= y < 8:
                c = cell[:, x + 8 * y]
                found |= alive & (c == 1) & (run != 0)
                alive &= c == 2
                run[alive] |= bits[x + 8 * y]
                x, y = x + dx, y + dy
            flips[:, sq] |= np.where(found, run, U(0))
    reach = ((flips != 0) * bits).sum(axis=1, dtype=U)
    return reach, flips


# ---- positions ------------------------------------------------------------
def random_positions(rng, n):
    """n positions with 4..64 discs, colours split at random"""
    ndisc = rng.integers(4, 65, n)
    order = np.argsort(rng.random((n, 64)), axis=1)
    occupied = order < ndisc[:, None]
    mine = rng.random((n, 64)) < rng.random(n)[:, None]
    bits = U(1) << np.arange(64, dtype=U)
    P = ((occupied & mine) * bits).sum(axis=1, dtype=U)
    O = ((occupied & ~mine) * bits).sum(axis=1, dtype=U)
    return P, O


EDGE = U(0xFF818181818181FF)


def edge_positions(rng, n):
    """random interiors with the a/h files and rows 1/8 full (alternating
    colours, one colour, or random colours): the wrap-prone cases of +-7 and +-9"""
    P, O = random_positions(rng, n)
    ring = [(x, 0) for x in range(8)] + [(7, y) for y in range(1, 8)] + [(x, 7) for x in range(6, -1, -1)] + \
           [(0, y) for y in range(6, 0, -1)]
    alt = [U(sum(1 << (x + 8 * y) for k, (x, y) in enumerate(ring) if k % 2 == ph)) for ph in (0, 1)]
    kind = rng.integers(0, 5, n)
    rnd = rng.integers(0, 2 ** 63, n).astype(U) * U(2) + rng.integers(0, 2, n).astype(U)
    pe = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [alt[0], alt[1], EDGE, U(0)], rnd & EDGE)
    P = (P & ~EDGE) | pe
    O = (O & ~EDGE) | (EDGE & ~pe)
    return P, O


def beyond_positions(rng, n):
    """a line from an empty square: k >= 1 opponent discs, a disc of the mover's
    (the stop square), then mostly more of the mover's discs with opponent
    discs and gaps among them, laid over a random position"""
    P, O = random_positions(rng, n)
    for i in range(n):
        while True:
            sq = int(rng.integers(0, 64))
            dx, dy = DIRS[int(rng.integers(0, 8))]
            line = []
            x, y = (sq & 7) + dx, (sq >> 3) + dy
            while 0 <= x < 8 and 0 <= y < 8:
                line.append(x + 8 * y)
                x, y = x + dx, y + dy
            if len(line) >= 3:
                break
        k = int(rng.integers(1, len(line) - 1))
        content = [2] * k + [1] + list(rng.choice([1, 2, 0], len(line) - k - 1, p=[0.7, 0.15, 0.15]))
        p, o = int(P[i]), int(O[i])
        for s, c in zip([sq] + line, [0] + content):
            p, o = p & ~(1 << s), o & ~(1 << s)
            if c == 1:
                p |= 1 << s
            elif c == 2:
                o |= 1 << s
        P[i], O[i] = U(p), U(o)
    return P, O


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(0xF111)
    parts = [random_positions(rng, 70000), edge_positions(rng, 24000), beyond_positions(rng, 8000)]
    # both colourings of the full board's edge ring with an empty interior, the opening
    extra_p = np.array([0xAA810081008100AA ^ 0, 0xFF818181818181FF, 0, 0x0000000810000000], U)
    extra_o = np.array([0xFF818181818181FF ^ 0xAA810081008100AA, 0, 0xFF818181818181FF, 0x0000001008000000], U)
    P = np.concatenate([p for p, _ in parts] + [extra_p])
    O = np.concatenate([o for _, o in parts] + [extra_o])
    assert len(P) >= 100000 and not (P & O).any()
    reach, flips = naive(P, O)
    return P, O, reach, flips


def test_positions_cover_the_cases(cases):
    P, O, _, _ = cases
    discs = np.bitwise_count(P | O)
    assert discs.min() <= 4 and discs.max() == 64
    assert ((P | O) & EDGE == EDGE).sum() >= 20000


def test_fills_are_runs_plus_own(cases):
    P, O, _, _ = cases
    s = analyse(P, O)
    for i in range(2, 8):
        assert not (s["G"][i] & ~(P | O)).any()
        assert ((s["G"][i] & P) == P).all()


def test_reach_and_legal_equal_the_scan(cases):
    P, O, reach, _ = cases
    s = analyse(P, O)
    assert (s["reach"] == reach).all()
    assert (s["legal"] == reach & ~(P | O)).all()
    # Board.puttables(Empty)'s operands: the empty squares move against one colour
    E = ~(P | O)
    r2, _ = naive(E[:5000], P[:5000])
    assert (analyse(E[:5000], P[:5000])["reach"] == r2).all()


def test_flips_masked_equal_the_scan(cases):
    P, O, reach, flips = cases
    legal = reach & ~(P | O)
    moves = own_extra = 0
    for sq in range(64):
        idx = np.nonzero(legal >> U(sq) & U(1))[0]
        if not len(idx):
            continue
        p, o = P[idx], O[idx]
        f = flips_col(sq, p, analyse(p, o))
        mv = U(1) << U(sq)
        assert ((f & o) == flips[idx, sq]).all(), sq
        assert not (f & ~(p | o | mv)).any(), sq  # nothing on an empty square but the move itself
        assert (f & mv == mv).all(), sq
        # place(): the boards after the move are the scan's
        assert ((p | f) == (p | flips[idx, sq] | mv)).all() and ((o & ~f) == (o & ~flips[idx, sq])).all()
        moves += len(idx)
        own_extra += int(((f & p) != 0).sum())
    assert moves > 300000
    assert own_extra > 10000  # the mover's own discs beyond the stop square do turn up in the flips
