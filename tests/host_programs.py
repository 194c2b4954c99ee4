"""What every test and check script of the host programs (tools/diag/*_host.cpp)
shares: the one compiler line, the files the programs read and write, and the
one way to run them.  A plain module, imported like golden_io.py.  DESIGN.md §30.

The programs are stand-alone: each run is a child process with its own `main`,
also under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "diag")

PLAIN = ("-O2", "-fopenmp")
SANITIZED = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
THREAD_SANITIZED = ("-O1", "-g", "-fsanitize=thread")
SUFFIX = {PLAIN: "", SANITIZED: "_asan", THREAD_SANITIZED: "_tsan"}
# what a program's build needs beyond the flag set: the MCTS scores are float32
# expressions the checker evaluates unfused; two programs start std::threads
EXTRA = {"mcts_host": ("-ffp-contract=off",), "mcts_tree_host": ("-ffp-contract=off",),
         "solve_window_host": ("-pthread",), "solve_hash_host": ("-pthread",)}
# the two programs without an OpenMP pragma, whose plain build is -O2 alone
NO_OPENMP = ("mcts_tree_host", "solve_hash_host")

_compiled = {}


def build(program, flags, exe):
    """Compile tools/diag/<program>.cpp into `exe`."""
    flags = [f for f in flags if f != "-fopenmp" or program not in NO_OPENMP]
    subprocess.check_call(["g++", "-std=c++17", *EXTRA.get(program, ()), *flags, "-o", exe,
                           os.path.join(DIAG, program + ".cpp")])
    return exe


def compiled(tmp_path_factory, program, flags=PLAIN):
    """The program's binary under `flags`, compiled once per process however many modules ask for it."""
    key = (program, tuple(flags))
    if key not in _compiled:
        if shutil.which("g++") is None:
            import pytest  # (here only: the check scripts use this module without it)

            pytest.skip("no g++")
        name = program + SUFFIX[key[1]]
        _compiled[key] = build(program, flags, str(tmp_path_factory.mktemp(name) / name))
    return _compiled[key]


class ProgramFailed(AssertionError):
    """A program ended with a non-zero status or a sanitizer's report; `.result` is its CompletedProcess."""

    def __init__(self, result):
        super().__init__("%s: exit status %d\n%s" % (os.path.basename(result.args[0]), result.returncode,
                                                     result.stderr[-2000:]))
        self.result = result


def run(argv):
    """Run a program to its end; a non-zero exit status or a sanitizer's report raises, with stderr's tail."""
    r = subprocess.run([str(a) for a in argv], capture_output=True, text=True)
    if r.returncode != 0 or "Sanitizer" in r.stderr or "runtime error" in r.stderr:
        raise ProgramFailed(r)
    return r


def position_lines(boards, turn, extra=None):
    """One line "<black hex> <white hex> <turn>" per position; `extra`: n values, or n rows of them, appended."""
    for i, ((b, w), t) in enumerate(zip(np.asarray(boards, np.uint64).tolist(), np.asarray(turn).tolist())):
        more = () if extra is None else np.atleast_1d(extra[i]).tolist()
        yield "%x %x %d" % (b, w, t) + "".join(" %d" % int(x) for x in more) + "\n"


def write_positions(path, boards, turn, extra=None):
    with open(path, "w") as f:
        f.writelines(position_lines(boards, turn, extra))


def weights_line(weights):
    return " ".join(str(int(x)) for x in np.asarray(weights).reshape(-1))


def write_weights(path, weights, end=""):
    with open(path, "w") as f:
        f.write(weights_line(weights) + end)


def read_rows(path, shape=None, orders=None, trailer=False):
    """An all-integer OUT file as an int64 array, one row per line, reshaped to `shape` if given.
    orders=k: the tree programs' lines of k task orders x (value, move, status, nodes), as four [k][n] arrays.
    trailer: the last line is words, not a row; (rows, its words) are returned."""
    lines = open(path).read().splitlines()
    last = lines.pop().split() if trailer else None
    rows = np.array([[int(x) for x in ln.split()] for ln in lines], np.int64)
    if orders is not None:
        rows = rows.reshape(-1, orders, 4)
        return tuple(rows[:, :, k].T for k in range(4))
    if shape is not None:
        rows = rows.reshape(shape)
    return (rows, last) if trailer else rows


def write_game_args(path, n, seed, depths, exact, n_rand, swap, limit, wa, wb, start=None, start_turn=None,
                    budgets=None, game_id0=0):
    """The ARGS file of the self-play programs: play_host.cpp's 11 fields without budgets, the 13 of
    budget_host.cpp's play and play_solve_host.cpp with them; the two tables; the starts if any."""
    head = [n, seed, game_id0, depths[0], depths[1]] + ([] if budgets is None else [budgets[0], budgets[1]])
    head += [exact, n_rand[0], n_rand[1], int(swap), limit, int(start is not None)]
    with open(path, "w") as f:
        f.write(" ".join("%d" % x for x in head) + "\n")
        for w in (wa, wb):
            f.write(weights_line(w) + "\n")
        if start is not None:
            f.writelines(position_lines(start, start_turn))


def read_games(path):
    """The self-play programs' OUT file: one game per line."""
    rows = [ln.split() for ln in open(path)]
    col = lambda k: np.array([int(r[k]) for r in rows], np.int64)  # noqa: E731
    return dict(a_black=col(0), final_boards=np.array([[int(r[1], 16), int(r[2], 16)] for r in rows],
                                                      np.uint64).reshape(-1, 2),
                diff=col(3), plies=col(4), status=col(5), nodes=col(6),
                moves=np.array([list(bytes.fromhex(r[7])) for r in rows], np.uint8).reshape(-1, 128))
