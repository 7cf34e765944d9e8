// Walks fg_abc_mix_plan and fg_abc_compact_plan (fugue_amd/csrc/fg_abc_plan.h, the planners fg_abc.hip calls) over a grid of shapes
// and checks, with the same fg_abc_mix_item / index helpers the kernels use, what a launch relies on: every (particle tile, center)
// pair is owned by exactly one wave, the ranges of a tile walk [0, n) in split order, ranges without work are empty and inside
// [0, n], every partial cell a wave writes lies inside the partial buffers, the table and coordinate indices are computed in 64
// bits, the grids are within HIP's limits; for the compaction that the waves cover the B attempts once and the scan walks every
// wave count.  One line per point:
//   mix m n d n_cu force | tiles splits cps items grid finish_grid d_reg partial table | ok|FAIL <what>
//   compact B | waves grid scan_chunks | ok|FAIL <what>
// tests/test_abc_cpu.py reads the lines.  Built stand-alone with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_abc_plan.h"

static std::string check_mix(long long m, long long n, long long d, int n_cu, long long force, FgAbcMixPlan &P) {
    const int rc = fg_abc_mix_plan(m, n, d, n_cu, force, &P);
    if (rc) return "plan rc " + std::to_string(rc);
    if (P.tiles != (m + 63) / 64) return "tiles";
    if (P.d_reg != ((d >= 1 && d <= FG_ABC_DREG) ? (int)d : 0)) return "register form";
    if (P.table_elems != (size_t)n * (size_t)(d + 1)) return "table size";
    if (m == 0) return (P.grid == 0 && P.items == 0 && P.partial_elems == 0 && P.finish_grid == 0) ? "ok" : "work planned for m = 0";
    if (P.splits < 1 || P.splits > FG_ABC_MAX_SPLITS) return "splits";
    if (force > 0 && P.splits != (force < FG_ABC_MAX_SPLITS ? force : FG_ABC_MAX_SPLITS)) return "forced splits not taken";
    if (P.centers_per_split < 1 || P.centers_per_split * P.splits < n) return "the ranges do not cover the centers";
    if (force == 0 && (P.splits - 1) * P.centers_per_split >= n) return "a planned range without work";
    if (P.items != P.tiles * P.splits) return "items";
    if ((long long)P.grid * FG_ABC_MIX_W < P.items || ((long long)P.grid - 1) * FG_ABC_MIX_W >= P.items) return "grid does not match the items";
    if (P.grid < 1 || P.grid > 0x7fffffffu) return "grid";
    if ((long long)P.finish_grid * 256 < m || ((long long)P.finish_grid - 1) * 256 >= m) return "finish grid";
    if (P.partial_elems != (size_t)P.splits * (size_t)m) return "partial size";
    // ownership: per tile the ranges walk [0, n) in split order; every partial cell written once and inside the buffer
    std::vector<long long> next((size_t)P.tiles, 0);
    std::vector<long long> seen_split((size_t)P.tiles, 0);
    std::vector<unsigned char> cell(P.partial_elems, 0);
    for (long long g = 0; g < (long long)P.grid * FG_ABC_MIX_W; ++g) {
        if (g >= P.items) continue;                       // the kernel's early return
        long long tile, split, j0, j1;
        fg_abc_mix_item(g, P.tiles, P.centers_per_split, n, &tile, &split, &j0, &j1);
        if (tile < 0 || tile >= P.tiles || split < 0 || split >= P.splits) return "item out of range";
        if (split != seen_split[(size_t)tile]++) return "splits of a tile out of order";
        if (j0 < 0 || j1 < j0 || j1 > n) return "range outside [0, n]";
        if (j0 != next[(size_t)tile]) return "ranges of tile " + std::to_string(tile) + " not contiguous at item " + std::to_string(g);
        next[(size_t)tile] = j1;
        for (int lane = 0; lane < 64; ++lane) {
            const long long i = tile * 64 + lane;
            if (i >= m) continue;                         // the kernel's `live`
            const long long o = fg_abc_partial_index(split, m, i);
            if (o < 0 || (size_t)o >= P.partial_elems) return "partial cell out of range";
            if (cell[(size_t)o]++) return "partial cell written twice";
        }
        if (j1 > j0 && (size_t)fg_abc_table_index(j1 - 1, d, d) >= P.table_elems) return "table row out of range";
    }
    for (long long t = 0; t < P.tiles; ++t) if (next[(size_t)t] != n || seen_split[(size_t)t] != P.splits) return "tile " + std::to_string(t) + " does not reach n";
    for (size_t q = 0; q < cell.size(); ++q) if (cell[q] != 1) return "partial cell " + std::to_string(q) + " written " + std::to_string((int)cell[q]) + " times";
    // 64-bit indices against 128-bit arithmetic
    const long long bm = 3000000000LL, bn = 5000000000LL, bd = 40;
    if ((__int128)fg_abc_partial_index(65534, bm, bm - 1) != (__int128)65534 * bm + bm - 1) return "partial index truncated";
    if ((__int128)fg_abc_table_index(bn - 1, bd, bd) != (__int128)(bn - 1) * (bd + 1) + bd) return "table index truncated";
    if ((__int128)fg_abc_coord_index(bd - 1, bn, bn - 1) != (__int128)(bd - 1) * bn + bn - 1) return "coordinate index truncated";
    return "ok";
}

static std::string check_compact(long long B, FgAbcCompactPlan &P) {
    const int rc = fg_abc_compact_plan(B, &P);
    if (rc) return "plan rc " + std::to_string(rc);
    if (P.waves * 64 < B || (P.waves - 1) * 64 >= B) return "waves";
    if ((long long)P.grid * 4 < P.waves || ((long long)P.grid - 1) * 4 >= P.waves) return "grid";
    if (P.scan_chunks * FG_ABC_SCAN_THREADS < P.waves || (P.scan_chunks - 1) * FG_ABC_SCAN_THREADS >= P.waves) return "scan chunks";
    return "ok";
}

int main(int argc, char **argv) {
    const int n_cu = argc > 1 ? std::atoi(argv[1]) : 256;
    const long long ms[] = {0, 1, 63, 64, 65, 130, 4096}, ns[] = {1, 10, 64, 65, 257, 1000, 65536}, ds[] = {0, 1, 5, 8, 9, 33}, forces[] = {0, 1, 7, 300};
    int bad = 0;
    for (long long m : ms) for (long long n : ns) for (long long d : ds) for (long long f : forces) {
        FgAbcMixPlan P = {};
        const std::string r = check_mix(m, n, d, n_cu, f, P);
        std::printf("mix %lld %lld %lld %d %lld | %lld %lld %lld %lld %u %u %d %zu %zu | %s\n", m, n, d, n_cu, f, P.tiles, P.splits, P.centers_per_split, P.items, P.grid,
                    P.finish_grid, P.d_reg, P.partial_elems, P.table_elems, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    const long long Bs[] = {1, 63, 64, 65, 200, 1024, 65536, 65537, 1LL << 31};
    for (long long B : Bs) {
        FgAbcCompactPlan P = {};
        const std::string r = check_compact(B, P);
        std::printf("compact %lld | %lld %u %lld | %s\n", B, P.waves, P.grid, P.scan_chunks, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    const bool rounds = fg_abc_max_rounds(1, 64) == 1 && fg_abc_max_rounds(64, 64) == 1 && fg_abc_max_rounds(65, 64) == 2 && fg_abc_max_rounds(0, 64) == 0 &&
                        fg_abc_max_rounds((1LL << 32), 1) == (1LL << 32);
    std::printf("rounds %s\n", rounds ? "ok" : "FAIL");
    // refused shapes are errors, not plans
    FgAbcMixPlan P;
    FgAbcCompactPlan Q;
    const bool refuses = fg_abc_mix_plan(-1, 1, 1, n_cu, 0, &P) == FG_E_BAD_ARG && fg_abc_mix_plan(1, 0, 1, n_cu, 0, &P) == FG_E_BAD_ARG &&
                         fg_abc_mix_plan(1, 1, -1, n_cu, 0, &P) == FG_E_BAD_ARG && fg_abc_mix_plan(1, 1, 1, n_cu, -1, &P) == FG_E_BAD_ARG &&
                         fg_abc_mix_plan((1LL << 60), 1, 1, n_cu, 65535, &P) == FG_E_LIMIT && fg_abc_mix_plan(1, (1LL << 61), 7, n_cu, 0, &P) == FG_E_LIMIT &&
                         fg_abc_compact_plan(0, &Q) == FG_E_BAD_ARG && fg_abc_compact_plan((1LL << 62), &Q) == FG_E_LIMIT;
    std::printf("refusals %s\n", refuses ? "ok" : "FAIL");
    return (bad || !rounds || !refuses) ? 1 : 0;
}
