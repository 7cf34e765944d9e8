// Walks fg_grid_plan (fugue_amd/csrc/fg_grid_plan.h, the planner fg_grid.hip calls) over the pairs "n_a n_b" given on the command line, with
// the plan's own base_chunk, a caller's (3) and a byte cap that one base overruns, and checks what the launches rely on: the grid within the
// hardware's limits, every cell owned by exactly one (wave, lane) of k_grid_eval and every cell of a row by exactly one (thread, slot) of the
// row workgroup, the chunk table within FG_GRID_CHUNK_BYTES (or one base), and the cut of n bases into chunks covering [0, n) exactly, in
// order, for n below, at and one past a chunk boundary.  One line per pair:
//   plan n_a n_b | rc cells waves base_chunk row_threads row_per_thread col_blocks mix_blocks | ok|FAIL <what>
// then `refusals ok|FAIL`.  tests/test_grid_cpu.py reads the lines.  Built stand-alone with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_grid_plan.h"

static std::string check_chunks(const FgGridPlan &P) {
    const long long bc = P.base_chunk, Ns[] = {1, bc - 1, bc, bc + 1, 2 * bc, 2 * bc + 1};
    for (long long n : Ns) {
        if (n < 1) continue;
        long long at = 0;
        const long long L = fg_grid_n_chunks(P, n);
        for (long long k = 0; k < L; ++k) {
            long long first, count;
            fg_grid_chunk(P, n, k, &first, &count);
            if (first != at || count < 1 || count > bc || count > FG_GRID_MAX_GRID_Y) return "chunk " + std::to_string(k) + " of " + std::to_string(n) + " bases";
            at += count;
        }
        long long first, count;
        fg_grid_chunk(P, n, L, &first, &count);
        if (at != n || count != 0) return "the chunks do not cover " + std::to_string(n) + " bases";
    }
    return "ok";
}

static std::string check(long long n_a, long long n_b, long long base_chunk, FgGridPlan &P, int *rc_out) {
    const int rc = *rc_out = fg_grid_plan(n_a, n_b, base_chunk, &P);
    if (rc) return "plan rc " + std::to_string(rc);
    if (P.n_a != n_a || P.n_b != n_b || P.cells != n_a * n_b || P.cells > FG_GRID_MAX_CELLS) return "cells";
    if ((long long)P.waves * FG_GRID_WAVE < P.cells || ((long long)P.waves - 1) * FG_GRID_WAVE >= P.cells) return "waves";
    if (P.base_chunk < 1 || P.base_chunk > FG_GRID_MAX_GRID_Y) return "base_chunk";
    if (base_chunk > 0 && P.base_chunk != (base_chunk < FG_GRID_MAX_GRID_Y ? base_chunk : FG_GRID_MAX_GRID_Y)) return "the caller's base_chunk";
    if (base_chunk == 0 && P.base_chunk > 1 && P.base_chunk * P.cells * 8 > FG_GRID_CHUNK_BYTES) return "the chunk table is above the cap";
    if (base_chunk == 0 && P.base_chunk < FG_GRID_MAX_GRID_Y && (P.base_chunk + 1) * P.cells * 8 <= FG_GRID_CHUNK_BYTES) return "a larger chunk fits the cap";
    if (P.row_threads < 64 || P.row_threads > FG_GRID_ROW_MAX_THREADS || P.row_threads % 64 || (P.row_threads & (P.row_threads - 1))) return "row_threads";
    if (P.row_per_thread < 1 || (long long)P.row_per_thread * P.row_threads < n_a || (long long)(P.row_per_thread - 1) * P.row_threads >= n_a) return "row_per_thread";
    if ((long long)P.col_blocks * FG_GRID_COL_THREADS < n_a || ((long long)P.col_blocks - 1) * FG_GRID_COL_THREADS >= n_a) return "col_blocks";
    if ((long long)P.mix_blocks * FG_GRID_COL_THREADS < P.cells || ((long long)P.mix_blocks - 1) * FG_GRID_COL_THREADS >= P.cells) return "mix_blocks";
    if (P.cells <= (1LL << 22)) {                              // ownership, cell by cell
        std::vector<unsigned char> own((size_t)P.cells, 0);
        for (unsigned w = 0; w < P.waves; ++w)
            for (int l = 0; l < FG_GRID_WAVE; ++l) {
                const long long c = fg_grid_cell(P, w, l);
                if (c == -1) { if (w + 1 != P.waves) return "a dead lane before the tail wave"; continue; }
                if (c < 0 || c >= P.cells) return "a cell outside the surface";
                if (own[(size_t)c]++) return "cell " + std::to_string(c) + " scored twice";
            }
        for (long long c = 0; c < P.cells; ++c) if (own[(size_t)c] != 1) return "cell " + std::to_string(c) + " not scored";
    }
    if (n_a <= (1LL << 22)) {
        std::vector<int> rown((size_t)n_a, 0);
        for (int t = 0; t < P.row_threads; ++t)
            for (int k = 0; k < P.row_per_thread; ++k) {
                const long long i = fg_grid_row_owner(P, t, k);
                if (i == -1) continue;
                if (i < 0 || i >= n_a) return "a row slot outside [0, n_a)";
                rown[(size_t)i]++;
            }
        for (long long i = 0; i < n_a; ++i) if (rown[(size_t)i] != 1) return "row cell " + std::to_string(i) + " owned " + std::to_string(rown[(size_t)i]) + " times";
    }
    return check_chunks(P);
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a + 1 < argc; a += 2) {
        const long long n_a = std::atoll(argv[a]), n_b = std::atoll(argv[a + 1]);
        FgGridPlan P = {}, Q = {};
        int rc = 0, rc3 = 0;
        std::string r = check(n_a, n_b, 0, P, &rc);
        if (r == "ok") { r = check(n_a, n_b, 3, Q, &rc3); if (r == "ok" && Q.base_chunk != 3) r = "base_chunk 3 not taken"; }
        std::printf("plan %lld %lld | %d %lld %u %lld %d %d %u %u | %s\n", n_a, n_b, rc, P.cells, P.waves, P.base_chunk, P.row_threads, P.row_per_thread, P.col_blocks, P.mix_blocks,
                    r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    FgGridPlan P = {};
    int rc = 0;
    bool refuses = fg_grid_plan(0, 1, 0, &P) == FG_E_BAD_ARG && fg_grid_plan(1, 0, 0, &P) == FG_E_BAD_ARG && fg_grid_plan(-4, 3, 0, &P) == FG_E_BAD_ARG &&
                   fg_grid_plan(3, -4, 0, &P) == FG_E_BAD_ARG && fg_grid_plan(3, 3, -1, &P) == FG_E_BAD_ARG &&
                   fg_grid_plan(1LL << 16, 1LL << 15, 0, &P) == FG_E_LIMIT && fg_grid_plan(1LL << 31, 1, 0, &P) == FG_E_LIMIT && fg_grid_plan(1, 1LL << 31, 0, &P) == FG_E_LIMIT &&
                   fg_grid_plan(1LL << 40, 1LL << 40, 0, &P) == FG_E_LIMIT && fg_grid_plan(1LL << 62, 4, 0, &P) == FG_E_LIMIT;
    // the largest surface (one base overruns the byte cap: a chunk of one) and the largest caller's chunk (cut to grid y)
    refuses = refuses && check(FG_GRID_MAX_CELLS, 1, 0, P, &rc) == "ok" && P.base_chunk == 1 && check(46340, 46340, 0, P, &rc) == "ok" && P.base_chunk == 1 &&
              check(5, 5, 1LL << 40, P, &rc) == "ok" && P.base_chunk == FG_GRID_MAX_GRID_Y;
    // the bases of a call: chains [chain0, chain0 + n) of C
    refuses = refuses && fg_grid_check_bases(5, 0, 5) == FG_OK && fg_grid_check_bases(5, 2, 3) == FG_OK && fg_grid_check_bases(5, 4, 1) == FG_OK &&
              fg_grid_check_bases(5, 2, 4) == FG_E_BAD_ARG && fg_grid_check_bases(5, 5, 1) == FG_E_BAD_ARG && fg_grid_check_bases(5, 0, 0) == FG_E_BAD_ARG &&
              fg_grid_check_bases(5, -1, 2) == FG_E_BAD_ARG && fg_grid_check_bases(5, 0, -2) == FG_E_BAD_ARG && fg_grid_check_bases(5, 6, 1) == FG_E_BAD_ARG &&
              fg_grid_check_bases(5, 1, 0x7fffffffffffffffLL) == FG_E_BAD_ARG && fg_grid_check_bases(5, 0x7fffffffffffffffLL, 1) == FG_E_BAD_ARG;
    std::printf("refusals %s\n", refuses ? "ok" : "FAIL");
    return (bad || !refuses) ? 1 : 0;
}
