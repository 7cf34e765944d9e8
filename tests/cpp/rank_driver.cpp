// Runs the rule of the rank-normalised diagnostics (fugue_amd/csrc/fg_diag_rank_plan.h, what fg_diag_rank.hip's kernels share) on the host.
//   rank_driver coord <file of S doubles> <p_lo> <p_hi> <out file>
//       one coordinate's pooled cells through the plan's own sort -- the stable LSD radix sort by host loops over the plan's blocks,
//       (digit, block) scan order and skipped passes, checked against std::stable_sort on the keys -- the run pass by a forward max
//       scan and a backward min scan, checked against lower / upper bounds, the normal scores, the median, the folded sort and the
//       tail indicators.  Writes doubles: r2 [S], z [S], z_folded [S], I_lo [S], I_hi [S], median, x_lo, x_hi, the FG_RANK_COUNTS counts.
//       Prints:  coord S | runs longest passes | ok|FAIL <what>
//   rank_driver z <S> <file of int64 r2> <out file>        fg_rank_z of every r2; also checks z(r2) = -z(2 S + 2 - r2) bit for bit
//   rank_driver plan <n> <C> <d> <j0> <n_j> <p_lo> <p_hi> ...    one line per seven:  plan | rc S k_lo k_hi nb nb_run nb_key block | ok
//   rank_driver refusals
// tests/test_diag_rank_cpu.py reads the lines.  Built stand-alone, a second time with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_diag_rank_plan.h"

static std::vector<double> read_doubles(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    double b[1024];
    size_t g;
    while ((g = std::fread(b, 8, 1024, f)) > 0) v.insert(v.end(), b, b + g);
    std::fclose(f);
    return v;
}

struct Sorted { std::vector<uint64_t> key; std::vector<uint32_t> idx; int passes = 0; std::string err; };

// the plan's sort of (key, cell index)
static Sorted plan_sort(const std::vector<uint64_t> &keys) {
    const long long S = (long long)keys.size();
    Sorted R;
    std::vector<uint64_t> ka = keys, kb(keys.size());
    std::vector<uint32_t> ia(keys.size()), ib(keys.size());
    for (long long i = 0; i < S; ++i) ia[i] = (uint32_t)i;
    std::vector<unsigned int> hist((size_t)FG_RANK_PASSES * FG_RANK_BINS, 0u);
    for (long long i = 0; i < S; ++i)
        for (int p = 0; p < FG_RANK_PASSES; ++p) hist[(size_t)p * FG_RANK_BINS + ((keys[i] >> (8 * p)) & 255u)] += 1u;
    const long long nb = (S + FG_RANK_TILE - 1) / FG_RANK_TILE;
    std::vector<unsigned int> table((size_t)FG_RANK_BINS * nb);
    for (int p = 0; p < FG_RANK_PASSES; ++p) {
        if (fg_rank_pass_skipped(&hist[(size_t)p * FG_RANK_BINS], S)) continue;
        std::fill(table.begin(), table.end(), 0u);
        for (long long i = 0; i < S; ++i) table[(size_t)((ka[i] >> (8 * p)) & 255u) * nb + i / FG_RANK_TILE] += 1u;
        unsigned int run = 0u;
        for (size_t t = 0; t < table.size(); ++t) { const unsigned int v = table[t]; table[t] = run; run += v; }
        if ((long long)run != S) { R.err = "the table does not count S"; return R; }
        for (long long b = 0; b < nb; ++b)                                      // block, then wave, round and lane: position order
            for (long long i = b * FG_RANK_TILE; i < std::min<long long>(S, (b + 1) * FG_RANK_TILE); ++i) {
                const unsigned int pos = table[(size_t)((ka[i] >> (8 * p)) & 255u) * nb + b]++;
                if ((long long)pos >= S) { R.err = "a position past S"; return R; }
                kb[pos] = ka[i]; ib[pos] = ia[i];
            }
        ka.swap(kb); ia.swap(ib);
        R.passes += 1;
    }
    R.key.swap(ka); R.idx.swap(ia);
    return R;
}

struct Ranks { std::vector<uint32_t> lo, hi; long long runs = 0, longest = 0; };       // per CELL

static std::string rank_cells(const std::vector<uint64_t> &keys, Sorted &st, Ranks &R) {
    const long long S = (long long)keys.size();
    st = plan_sort(keys);
    if (!st.err.empty()) return st.err;
    std::vector<uint32_t> ord(S);
    for (long long i = 0; i < S; ++i) ord[i] = (uint32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    for (long long i = 0; i < S; ++i)
        if (st.idx[i] != ord[i] || st.key[i] != keys[ord[i]]) return "the plan's sort is not the stable sort";
    std::vector<long long> lo(S), hi(S);
    long long run = -1;
    for (long long i = 0; i < S; ++i) { if (i == 0 || st.key[i - 1] != st.key[i]) run = i; lo[i] = run; }
    run = S;
    for (long long i = S - 1; i >= 0; --i) { if (i == S - 1 || st.key[i + 1] != st.key[i]) run = i + 1; hi[i] = run; }
    R.lo.assign(S, 0u); R.hi.assign(S, 0u); R.runs = 0; R.longest = 0;
    for (long long i = 0; i < S; ++i) {
        const long long l = std::lower_bound(st.key.begin(), st.key.end(), st.key[i]) - st.key.begin();
        const long long h = std::upper_bound(st.key.begin(), st.key.end(), st.key[i]) - st.key.begin();
        if (l != lo[i] || h != hi[i]) return "the scans disagree with the bounds";
        R.lo[st.idx[i]] = (uint32_t)lo[i]; R.hi[st.idx[i]] = (uint32_t)hi[i];
        if (lo[i] == i) { R.runs += 1; R.longest = std::max(R.longest, hi[i] - lo[i]); }
    }
    return "";
}

static int cmd_coord(const char *in, double p_lo, double p_hi, const char *out) {
    const std::vector<double> x = read_doubles(in);
    const long long S = (long long)x.size();
    FgRankPlan P;
    const int rc = fg_rank_plan(S, 1, 1, 0, 1, p_lo, p_hi, &P);
    if (rc || S < 1) { std::printf("coord %lld | | FAIL plan rc %d\n", S, rc); return 1; }
    std::vector<uint64_t> keys(S);
    long long n_nan = 0, n_ninf = 0, n_pinf = 0, n_nanf = 0;
    for (long long i = 0; i < S; ++i) {
        keys[i] = fg_rank_key(x[i]);
        n_nan += x[i] != x[i]; n_ninf += x[i] == -INFINITY; n_pinf += x[i] == INFINITY;
        const double back = fg_rank_unkey(keys[i]);
        if (!((back != back && x[i] != x[i]) || back == x[i])) { std::printf("coord %lld | | FAIL unkey\n", S); return 1; }
    }
    Sorted st, stf;
    Ranks R, Rf;
    std::string err = rank_cells(keys, st, R);
    if (!err.empty()) { std::printf("coord %lld | | FAIL %s\n", S, err.c_str()); return 1; }
    const double med = fg_rank_median(fg_rank_unkey(st.key[(S - 1) / 2]), fg_rank_unkey(st.key[S / 2]));
    std::vector<uint64_t> fkeys(S);
    for (long long i = 0; i < S; ++i) { const double f = fg_rank_fold(x[i], med); fkeys[i] = fg_rank_key(f); n_nanf += f != f; }
    err = rank_cells(fkeys, stf, Rf);
    if (!err.empty()) { std::printf("coord %lld | | FAIL folded: %s\n", S, err.c_str()); return 1; }
    std::vector<double> o((size_t)5 * S + 3 + FG_RANK_COUNTS);
    for (long long i = 0; i < S; ++i) {
        const long long r2 = (long long)R.lo[i] + R.hi[i] + 1, rf = (long long)Rf.lo[i] + Rf.hi[i] + 1;
        if (r2 < 2 || r2 > 2 * S) { std::printf("coord %lld | | FAIL r2 outside [2, 2 S]\n", S); return 1; }
        o[i] = (double)r2;
        o[S + i] = fg_rank_z(r2, S);
        o[2 * S + i] = fg_rank_z(rf, S);
        o[3 * S + i] = (long long)R.lo[i] <= P.k_lo ? 1.0 : 0.0;
        o[4 * S + i] = (long long)R.lo[i] <= P.k_hi ? 1.0 : 0.0;
        if ((o[3 * S + i] == 1.0) != (keys[i] <= st.key[P.k_lo])) { std::printf("coord %lld | | FAIL I_lo is not x <= sorted[k_lo]\n", S); return 1; }
    }
    double *t = &o[(size_t)5 * S];
    t[0] = med; t[1] = fg_rank_unkey(st.key[P.k_lo]); t[2] = fg_rank_unkey(st.key[P.k_hi]);
    const long long c[FG_RANK_COUNTS] = { S, R.runs, R.longest, n_nan, n_ninf, n_pinf, n_nanf, st.passes + stf.passes };
    for (int i = 0; i < FG_RANK_COUNTS; ++i) t[3 + i] = (double)c[i];
    FILE *f = std::fopen(out, "wb");
    if (!f || std::fwrite(o.data(), 8, o.size(), f) != o.size()) { std::printf("coord %lld | | FAIL write\n", S); return 1; }
    std::fclose(f);
    std::printf("coord %lld | %lld %lld %d | ok\n", S, R.runs, R.longest, st.passes + stf.passes);
    return 0;
}

static int cmd_z(long long S, const char *in, const char *out) {
    const std::vector<double> raw = read_doubles(in);                          // int64 read as 8-byte words
    std::vector<double> z(raw.size());
    for (size_t i = 0; i < raw.size(); ++i) {
        int64_t r2;
        std::memcpy(&r2, &raw[i], 8);
        if (r2 < 2 || r2 > 2 * S) { std::printf("z | FAIL r2 outside [2, 2 S]\n"); return 1; }
        z[i] = fg_rank_z(r2, S);
        const double m = fg_rank_z(2 * S + 2 - r2, S);
        if (fg_rank_bits(m) != fg_rank_bits(-z[i]) && !(z[i] == 0.0 && m == 0.0)) { std::printf("z | FAIL z(%lld) is not -z(%lld)\n", (long long)r2, (long long)(2 * S + 2 - r2)); return 1; }
        if (!(z[i] == z[i]) || std::isinf(z[i])) { std::printf("z | FAIL not finite\n"); return 1; }
    }
    FILE *f = std::fopen(out, "wb");
    if (!f || std::fwrite(z.data(), 8, z.size(), f) != z.size()) { std::printf("z | FAIL write\n"); return 1; }
    std::fclose(f);
    std::printf("z %lld %zu | ok\n", S, z.size());
    return 0;
}

static int cmd_plan(int argc, char **argv) {
    int bad = 0;
    for (int a = 2; a + 6 < argc; a += 7) {
        const long long n = std::atoll(argv[a]), C = std::atoll(argv[a + 1]), d = std::atoll(argv[a + 2]), j0 = std::atoll(argv[a + 3]), nj = std::atoll(argv[a + 4]);
        const double p_lo = std::atof(argv[a + 5]), p_hi = std::atof(argv[a + 6]);
        FgRankPlan P;
        std::memset(&P, 0, sizeof P);
        const int rc = fg_rank_plan(n, C, d, j0, nj, p_lo, p_hi, &P);
        std::string ok = "ok";
        if (!rc) {
            if (P.S != n * C || (long long)P.nb * FG_RANK_TILE < P.S || ((long long)P.nb - 1) * FG_RANK_TILE >= P.S) ok = "FAIL blocks";
            if ((long long)P.nb_run * FG_RANK_RUN_TILE < P.S || ((long long)P.nb_run - 1) * FG_RANK_RUN_TILE >= P.S) ok = "FAIL run blocks";
            if (P.k_lo < 0 || P.k_hi >= P.S || P.k_lo > P.k_hi) ok = "FAIL k_p";
            if (P.b_keys != (size_t)P.S * 8 || P.b_idx != (size_t)P.S * 4) ok = "FAIL bytes";
            const long long blk = fg_rank_block(P, d, 0), one = fg_rank_block(P, d, 1);
            if (blk < 1 || blk > d || one != 1) ok = "FAIL block of coordinates";
        }
        if (ok != "ok") bad = 1;
        std::printf("plan | %d %lld %lld %lld %u %u %u %lld | %s\n", rc, rc ? 0ll : P.S, rc ? 0ll : P.k_lo, rc ? 0ll : P.k_hi, rc ? 0u : P.nb, rc ? 0u : P.nb_run, rc ? 0u : P.nb_key,
                    rc ? 0ll : fg_rank_block(P, d, 0), ok.c_str());
    }
    return bad;
}

static int cmd_refusals() {
    FgRankPlan P;
    struct { long long n, C, d, j0, nj; double lo, hi; int want; } t[] = {
        { 0, 4, 1, 0, 1, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 0, 1, 0, 1, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 4, 0, 0, 1, 0.05, 0.95, FG_E_BAD_ARG },
        { 4, 4, 65536, 0, 1, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 4, 3, 3, 1, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 4, 3, -1, 1, 0.05, 0.95, FG_E_BAD_ARG },
        { 4, 4, 3, 1, 3, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 4, 3, 0, 0, 0.05, 0.95, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, -0.1, 0.95, FG_E_BAD_ARG },
        { 4, 4, 3, 0, 3, 0.05, 1.5, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, 0.6, 0.5, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, NAN, 0.5, FG_E_BAD_ARG },
        { 65536, 32768, 1, 0, 1, 0.05, 0.95, FG_E_LIMIT }, { 1ll << 40, 1ll << 40, 1, 0, 1, 0.05, 0.95, FG_E_LIMIT }, { 32767, 65536, 1, 0, 1, 0.05, 0.95, FG_OK },
        { 4, 4, 65535, 65534, 1, 0.0, 1.0, FG_OK }, { 1, 1, 1, 0, 1, 0.5, 0.5, FG_OK },
    };
    int bad = 0;
    for (auto &c : t) {
        const int rc = fg_rank_plan(c.n, c.C, c.d, c.j0, c.nj, c.lo, c.hi, &P);
        std::printf("refusal n %lld C %lld d %lld j0 %lld n_j %lld p %g %g | rc %d want %d\n", c.n, c.C, c.d, c.j0, c.nj, c.lo, c.hi, rc, c.want);
        bad |= rc != c.want;
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc >= 6 && !std::strcmp(argv[1], "coord")) return cmd_coord(argv[2], std::atof(argv[3]), std::atof(argv[4]), argv[5]);
    if (argc >= 5 && !std::strcmp(argv[1], "z")) return cmd_z(std::atoll(argv[2]), argv[3], argv[4]);
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return cmd_plan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return cmd_refusals();
    std::fprintf(stderr, "usage: rank_driver coord|z|plan|refusals ...\n");
    return 2;
}
