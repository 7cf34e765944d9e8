// Walks fg_predict_plan (fugue_amd/csrc/fg_predict_plan.h, the planner fg_predict_eval calls) over a grid of shapes and checks, with
// the same fg_predict_item / index helpers the kernel uses, what a launch relies on: every (tile, draw) pair is owned by exactly one
// wave, LDS within the budget (160 KB for one slice, 64 KB when slices share a workgroup), <= 1 024 threads, a grid within HIP's
// limits, the global form chosen when and only when the slice exceeds a CU's LDS or it is forced, index products computed in 64
// bits.  One line per point:
//   point C n n_slots n_cu force | W draws_per_wave tiles chunks items grid lds global scratch | ok|FAIL <what>
// tests/test_predict_cpu.py reads the lines.  Built stand-alone with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_predict_plan.h"

static std::string check(long long C, long long n, int n_slots, int n_cu, bool force, FgPredictPlan &P) {
    const int rc = fg_predict_plan(C, n, n_slots, 7, n_cu, force, &P);
    if (rc) return "plan rc " + std::to_string(rc);
    const size_t slice = (size_t)n_slots * 512;
    if (P.W < 1 || P.W * FG_PRED_WAVE > 1024) return "threads";
    if (P.lds > (size_t)FG_PRED_LDS_MAX) return "lds";
    if (P.W > 1 && P.lds > (size_t)FG_PRED_LDS_PLAIN) return "shared workgroup beyond 64 KB";
    if (!P.global_tile && P.lds != (size_t)P.W * slice) return "lds bytes";
    if (!force && slice <= (size_t)FG_PRED_LDS_MAX && P.global_tile) return "global form without need";
    if ((force || slice > (size_t)FG_PRED_LDS_MAX) && !P.global_tile) return "global form not chosen";
    if (P.tiles != (C + 63) / 64) return "tiles";
    if (n == 0) {                                          // nothing to launch
        if (P.grid != 0 || P.items != 0 || P.chunks != 0 || P.scratch_bytes != 0) return "work planned for n = 0";
        return "ok";
    }
    if (P.global_tile && (P.lds != 0 || P.scratch_bytes != (size_t)P.grid * P.W * slice)) return "scratch bytes";
    if (P.grid < 1 || P.grid > 0x7fffffffu) return "grid";
    if (P.items != P.tiles * P.chunks) return "items";
    if ((long long)P.grid * P.W < P.items || ((long long)P.grid - 1) * P.W >= P.items) return "grid does not match the items";
    // ownership: every (tile, draw) exactly once.  Per tile the runs of draws must tile [0, n) in chunk order, and every cell is counted
    std::vector<long long> next((size_t)P.tiles, 0);
    std::vector<unsigned char> seen((size_t)(P.tiles * n), 0);
    for (long long g = 0; g < (long long)P.grid * P.W; ++g) {
        if (g >= P.items) continue;                       // the kernel's early return
        long long tile, t0, t1;
        fg_predict_item(g, P.tiles, P.draws_per_wave, n, &tile, &t0, &t1);
        if (tile < 0 || tile >= P.tiles) return "tile out of range";
        if (t0 != next[(size_t)tile] || t1 <= t0 || t1 > n) return "draws of tile " + std::to_string(tile) + " not contiguous at item " + std::to_string(g);
        next[(size_t)tile] = t1;
        for (long long t = t0; t < t1; ++t) if (seen[(size_t)(tile * n + t)]++) return "pair owned twice";
        // the scratch slice of this wave lies inside the scratch
        if (P.global_tile && ((size_t)g + 1) * slice > P.scratch_bytes) return "scratch slice out of range";
    }
    for (size_t q = 0; q < seen.size(); ++q) if (seen[q] != 1) return "pair " + std::to_string(q) + " owned " + std::to_string((int)seen[q]) + " times";
    // the last cell of the tables [n][n_sel][C] and of the draws [n][n_rows][C], against 128-bit arithmetic
    const long long n_sel = 1024, n_rows = 33, big_n = n * 100000;
    const __int128 want_out = (__int128)big_n * n_sel * C - 1, want_in = (__int128)big_n * n_rows * C - 1;
    if ((__int128)fg_predict_out_index(big_n - 1, n_sel, n_sel - 1, C, C - 1) != want_out) return "table index truncated";
    if ((__int128)fg_predict_draw_index(big_n - 1, n_rows, n_rows - 1, C, C - 1) != want_in) return "draw index truncated";
    return "ok";
}

int main(int argc, char **argv) {
    const int n_cu = argc > 1 ? std::atoi(argv[1]) : 256;
    const long long Cs[] = {1, 63, 64, 65, 130, 65536}, ns[] = {0, 1, 2, 7, 1000};
    const int slots[] = {2, 40, 320, 321, 2000};
    int bad = 0;
    for (long long C : Cs) for (long long n : ns) for (int s : slots) for (int force = 0; force < 2; ++force) {
        FgPredictPlan P = {};
        const std::string r = check(C, n, s, n_cu, force != 0, P);
        std::printf("point %lld %lld %d %d %d | %d %lld %lld %lld %lld %u %zu %d %zu | %s\n", C, n, s, n_cu, force, P.W, P.draws_per_wave, P.tiles, P.chunks, P.items, P.grid,
                    P.lds, P.global_tile, P.scratch_bytes, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    // refused shapes are errors, not plans
    FgPredictPlan P;
    const bool refuses = fg_predict_plan(0, 1, 1, 1, n_cu, false, &P) == FG_E_BAD_ARG && fg_predict_plan(1, -1, 1, 1, n_cu, false, &P) == FG_E_BAD_ARG &&
                         fg_predict_plan(1, 1, 0, 1, n_cu, false, &P) == FG_E_BAD_ARG && fg_predict_plan((1LL << 62), 1, 1, 1, n_cu, false, &P) == FG_E_LIMIT;
    std::printf("refusals %s\n", refuses ? "ok" : "FAIL");
    return (bad || !refuses) ? 1 : 0;
}
