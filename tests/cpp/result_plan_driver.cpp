// Walks fg_result_plan (fugue_amd/csrc/fg_result_plan.h, the planner fg_result_eval calls) over a grid of shapes and checks, with
// the same fg_result_item / index helpers the kernel uses, what a launch relies on: every (tile, draw) pair is owned by exactly one
// wave, LDS <= 160 KB, <= 1 024 threads, a grid within HIP's limits, index products computed in 64 bits.  One line per point:
//   point C n n_slots n_cu force | W draws_per_wave tiles chunks items grid lds global scratch | ok|FAIL <what>
// tests/test_result_cpu.py reads the lines.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_result_plan.h"

static std::string check(long long C, long long n, int n_slots, int n_cu, bool force, FgResultPlan &P) {
    const int rc = fg_result_plan(C, n, n_slots, 7, n_cu, force, &P);
    if (rc) return "plan rc " + std::to_string(rc);
    if (P.W < 1 || P.W * FG_RES_WAVE > 1024) return "threads";
    if (P.lds > (size_t)FG_RES_LDS_MAX) return "lds";
    if (!P.global_tile && P.lds != (size_t)P.W * n_slots * 512) return "lds bytes";
    if (P.global_tile && (P.lds != 0 || P.scratch_bytes != (size_t)P.grid * P.W * n_slots * 512)) return "scratch bytes";
    if (!force && (size_t)n_slots * 512 <= (size_t)FG_RES_LDS_MAX && P.global_tile) return "global form without need";
    if ((size_t)n_slots * 512 > (size_t)FG_RES_LDS_MAX && !P.global_tile) return "slice beyond a CU's LDS kept in LDS";
    if (P.grid < 1 || P.grid > 0x7fffffffu) return "grid";
    if (P.tiles != (C + 63) / 64) return "tiles";
    if ((long long)P.grid * P.W < P.items || ((long long)P.grid - 1) * P.W >= P.items) return "grid does not match the items";
    // ownership: item g = chunk * tiles + tile; per tile the runs of draws must tile [0, n) in chunk order, without gap or overlap
    std::vector<long long> next((size_t)P.tiles, 0);
    for (long long g = 0; g < (long long)P.grid * P.W; ++g) {
        if (g >= P.items) continue;                       // the kernel's early return
        long long tile, t0, t1;
        fg_result_item(g, P.tiles, P.draws_per_wave, n, &tile, &t0, &t1);
        if (tile < 0 || tile >= P.tiles) return "tile out of range";
        if (t0 != next[(size_t)tile] || t1 <= t0 || t1 > n) return "draws of tile " + std::to_string(tile) + " not contiguous at item " + std::to_string(g);
        next[(size_t)tile] = t1;
    }
    for (long long q = 0; q < P.tiles; ++q) if (next[(size_t)q] != n) return "tile " + std::to_string(q) + " ends at draw " + std::to_string(next[(size_t)q]);
    // the last cell of the results [n][R][C] and of the draws [n][n_rows][C], against 128-bit arithmetic
    const long long R = 3, n_rows = 33;
    const __int128 want_out = (__int128)n * R * C - 1, want_in = (__int128)n * n_rows * C - 1;
    if ((__int128)fg_result_out_index(n - 1, R, R - 1, C, C - 1) != want_out) return "result index truncated";
    if ((__int128)fg_result_draw_index(n - 1, n_rows, n_rows - 1, C, C - 1) != want_in) return "draw index truncated";
    return "ok";
}

int main(int argc, char **argv) {
    const int n_cu = argc > 1 ? std::atoi(argv[1]) : 256;
    const long long Cs[] = {1, 63, 64, 65, 8192, 65536}, ns[] = {1, 2, 7, 64, 1000000};
    const int slots[] = {1, 2, 33, 64, 65, 128, 129, 320, 321, 1000};
    int bad = 0;
    for (long long C : Cs) for (long long n : ns) for (int s : slots) for (int force = 0; force < 2; ++force) {
        FgResultPlan P = {};
        const std::string r = check(C, n, s, n_cu, force != 0, P);
        std::printf("point %lld %lld %d %d %d | %d %lld %lld %lld %lld %u %zu %d %zu | %s\n", C, n, s, n_cu, force, P.W, P.draws_per_wave, P.tiles, P.chunks, P.items, P.grid,
                    P.lds, P.global_tile, P.scratch_bytes, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    // refused shapes are errors, not plans
    FgResultPlan P;
    const bool refuses = fg_result_plan(0, 1, 1, 1, n_cu, false, &P) == FG_E_BAD_ARG && fg_result_plan(1, 0, 1, 1, n_cu, false, &P) == FG_E_BAD_ARG &&
                         fg_result_plan(1, 1, 0, 1, n_cu, false, &P) == FG_E_BAD_ARG && fg_result_plan((1LL << 62), 1, 1, 1, n_cu, false, &P) == FG_E_LIMIT;
    std::printf("refusals %s\n", refuses ? "ok" : "FAIL");
    return (bad || !refuses) ? 1 : 0;
}
