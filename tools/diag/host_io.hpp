// host_io.hpp — the front end every *_host.cpp shares: the files they read and
// the two defaults they all state.  What a program does with its positions, and
// every OUT format, stays in the program.
//
//   positions  "<black hex> <white hex> <turn>[ <extra>[ <extra>]]", one per line
//   weights    36 integers in -128..127, [phase][feature]
//
// HOST_IO_NO_CORES, defined before the include, leaves out the weights and with
// them the only core header this file reads: solve_deep_ref.cpp, the reference
// that must not depend on the cores, takes the positions reader that way.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// a node_limit of 0 on a command line or in a game-arguments file
constexpr uint32_t kNodeLimit = 1u << 28;
inline uint32_t node_limit(unsigned long long arg) { return arg ? (uint32_t)arg : kNodeLimit; }

// one line of a positions file.  The extra columns are what the program says
// they are (line_host and perft_host a depth, budget_host a budget,
// mcts_tree_host an id base, solve_window_host alpha and beta); they are read
// as unsigned, a minus sign wraps, and a signed column is cast back.
struct Pos {
    uint64_t black, white;
    int turn;
    unsigned long long extra[2];
    bool white_to_move() const { return turn == 2; }
    uint64_t mover() const { return turn == 2 ? white : black; }
    uint64_t other() const { return turn == 2 ? black : white; }
};

// the fields of one position in a line of text: 3 + its extra columns when whole
inline int parse_position(const char* line, Pos& p) {
    unsigned long long b, w;
    p.extra[0] = p.extra[1] = 0;
    const int got = sscanf(line, "%llx %llx %d %llu %llu", &b, &w, &p.turn, &p.extra[0], &p.extra[1]);
    if (got >= 2) p.black = b, p.white = w;
    return got < 0 ? 0 : got;
}

// The positions of an open file with `extras` extra columns each, up to `most`
// of them (< 0: all), up to the first that does not scan.  Returns that last
// record's fields: 0 at the end of the file, 3 where only its extras are short.
inline int read_positions(FILE* in, int extras, std::vector<Pos>& pos, long most = -1) {
    for (long i = 0; most < 0 || i < most; i++) {
        unsigned long long b, w;
        Pos p{};
        int got = fscanf(in, "%llx %llx %d", &b, &w, &p.turn);
        if (got != 3) return got < 0 ? 0 : got;
        for (int k = 0; k < extras; k++, got++)
            if (fscanf(in, "%llu", &p.extra[k]) != 1) return got;
        p.black = b, p.white = w;
        pos.push_back(p);
    }
    return 0;
}

// a file that does not open ends the program with status 1
inline FILE* open_or_exit(const char* path, const char* mode) {
    FILE* f = fopen(path, mode);
    if (!f) exit(1);
    return f;
}

inline int read_positions(const char* path, int extras, std::vector<Pos>& pos) {
    FILE* in = open_or_exit(path, "r");
    const int last = read_positions(in, extras, pos);
    fclose(in);
    return last;
}

// "usage: PROGRAM ARGUMENTS" on stderr, status 2
[[noreturn]] inline void usage(const char* program, const char* arguments) {
    fprintf(stderr, "usage: %s %s\n", program, arguments);
    exit(2);
}

#ifndef HOST_IO_NO_CORES
#include "../../subproc_amd/csrc/search_core.hpp"

// 36 weights from an open file, widened to the table the searches read
// (othm::kEvalTable ints).  False: one is missing or out of range.
inline bool read_weights(FILE* f, int* table) {
    int8_t w36[othm::kEvalPhases * othm::kEvalFeatures];
    for (int8_t& w : w36) {
        int v;
        if (fscanf(f, "%d", &v) != 1 || v < -128 || v > 127) return false;
        w = (int8_t)v;
    }
    for (int e = 0; e < othm::kEvalTable; e++) othm::widen_weight(w36, e, table);
    return true;
}

// the same from a path: status 1 where it does not open, 2 on a bad weight
inline void read_weights(const char* path, int* table) {
    FILE* f = open_or_exit(path, "r");
    if (!read_weights(f, table)) exit(2);
    fclose(f);
}
#endif  // HOST_IO_NO_CORES
