// Walks fg_gibbs_plan (fugue_amd/csrc/fg_gibbs_plan.h, the planner fg_gibbs.hip calls) over a model made of one discrete site per
// "K" given on the command line (site j: support [-3, -3 + K - 1]) followed by an f64 site `x`, a Poisson-like site `po` without a
// support and a site `big` of FG_GIBBS_K_CAP + 1 values, for C = 1, 64, 65 and 130 chains, and checks what the launch relies on: cell0
// the running sum of K, K_max, the work table and the cell tables in bytes, the grid covering every chain with exactly one (wave, lane),
// the pooling tree ending in one element, the automatic list (n_sites == 0) keeping exactly the sites a sweep can move.  One line per C:
//   plan C | rc n_sites n_cells K_max grid work_bytes cell_bytes | cell0 ... | ok|FAIL <what>
// then one line per refusal, `refusal <name> | rc | message`, and `sweeps ok|FAIL`.  tests/test_gibbs_cpu.py reads the lines.
// Built stand-alone with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_gibbs_plan.h"

static std::string check(const std::vector<FgGibbsSiteInfo> &info, const std::vector<int32_t> &list, const std::vector<int32_t> &expect, const std::vector<long long> &Ks, long long C, FgGibbsPlan &P, int *rc_out) {
    std::string err;
    const int rc = *rc_out = fg_gibbs_plan(info, list.data(), (int)list.size(), C, &P, &err);
    if (rc) return "plan rc " + std::to_string(rc) + " " + err;
    if (P.sites.size() != Ks.size()) return "n_sites";
    long long at = 0; int kmax = 0;
    for (size_t i = 0; i < Ks.size(); ++i) {
        const FgGibbsSite &s = P.sites[i];
        if (s.site != expect[i] || s.K != Ks[i] || s.lo != -3 || s.cell0 != at) return "site " + std::to_string(i);
        at += s.K;
        if (s.K > kmax) kmax = s.K;
    }
    if (P.n_cells != at || P.K_max != kmax || P.C != C) return "n_cells / K_max";
    if (P.work_bytes != (size_t)kmax * (size_t)C * 8 || P.cell_bytes != (size_t)at * (size_t)C * 8) return "bytes";
    if ((long long)P.grid * FG_GIBBS_WAVE < C || ((long long)P.grid - 1) * FG_GIBBS_WAVE >= C) return "grid";
    std::vector<unsigned char> own((size_t)C, 0);
    for (unsigned w = 0; w < P.grid; ++w)
        for (int l = 0; l < FG_GIBBS_WAVE; ++l) {
            const long long c = fg_gibbs_chain(P, w, l);
            if (c == -1) { if (w + 1 != P.grid) return "a dead lane before the tail wave"; continue; }
            if (c < 0 || c >= C) return "a chain outside the engine";
            if (own[(size_t)c]++) return "chain " + std::to_string(c) + " swept twice";
        }
    for (long long c = 0; c < C; ++c) if (own[(size_t)c] != 1) return "chain " + std::to_string(c) + " not swept";
    if (P.levels.empty() || P.levels[0].m_in != C || P.levels.back().m_out != 1) return "the pooling tree";
    if (P.slices.empty() || P.slices.back().k0 + P.slices.back().nk != P.n_cells) return "the pooling slices";
    // the pooled sum of a table of ones on the fixed tree is C, exactly
    std::vector<double> ones((size_t)P.n_cells * (size_t)C, 1.0);
    const std::vector<double> pooled = fg_pool_host<FgGibbsPool>(P.levels, P.slices, ones.data(), 0);
    for (double v : pooled) if (v != (double)C) return "the pooled sum of ones";
    return "ok";
}

int main(int argc, char **argv) {
    std::vector<FgGibbsSiteInfo> info;
    std::vector<long long> Ks;
    std::vector<int32_t> list;
    for (int a = 1; a < argc; ++a) {
        const long long K = std::atoll(argv[a]);
        FgGibbsSiteInfo I;
        I.name = "s#" + std::to_string(a - 1); I.vtype = FG_I64; I.has_support = 1; I.lo = -3; I.hi = -3 + K - 1;
        list.push_back((int32_t)info.size());
        info.push_back(I); Ks.push_back(K);
    }
    FgGibbsSiteInfo X; X.name = "x"; X.vtype = FG_F64;
    FgGibbsSiteInfo Po; Po.name = "po"; Po.vtype = FG_U64;
    FgGibbsSiteInfo Big; Big.name = "big"; Big.vtype = FG_USIZE; Big.has_support = 1; Big.lo = 0; Big.hi = FG_GIBBS_K_CAP;
    FgGibbsSiteInfo Empty; Empty.name = "empty"; Empty.vtype = FG_I64; Empty.has_support = 1; Empty.lo = 2; Empty.hi = 1;
    const int x = (int)info.size(), po = x + 1, big = x + 2, empty = x + 3;
    info.push_back(X); info.push_back(Po); info.push_back(Big); info.push_back(Empty);
    int bad = 0;
    for (long long C : {1LL, 64LL, 65LL, 130LL}) {
        FgGibbsPlan P, Q;
        int rc = 0, rc0 = 0;
        std::string r = check(info, list, list, Ks, C, P, &rc);
        if (r == "ok") { r = check(info, {}, list, Ks, C, Q, &rc0); if (r != "ok") r = "automatic list: " + r; }     // n_sites == 0 keeps the same sites: x, po, big and empty are left out
        std::printf("plan %lld | %d %zu %lld %d %u %zu %zu |", C, rc, P.sites.size(), P.n_cells, P.K_max, P.grid, P.work_bytes, P.cell_bytes);
        for (const FgGibbsSite &s : P.sites) std::printf(" %lld", s.cell0);
        std::printf(" | %s\n", r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    struct Case { const char *name; std::vector<int32_t> sites; int n; bool null_list; long long C; bool null_out; };
    const std::vector<Case> cases = {
        { "k_cap", { big }, 1, false, 4, false }, { "f64", { 0, x }, 2, false, 4, false }, { "no_support", { po }, 1, false, 4, false }, { "empty_support", { empty }, 1, false, 4, false },
        { "twice", { 0, 1, 0 }, 3, false, 4, false }, { "negative_n", { 0 }, -1, false, 4, false }, { "null_list", {}, 2, true, 4, false }, { "outside", { (int32_t)info.size() }, 1, false, 4, false },
        { "below", { -1 }, 1, false, 4, false }, { "no_chains", { 0 }, 1, false, 0, false }, { "null_out", { 0 }, 1, false, 4, true },
    };
    for (const Case &c : cases) {
        FgGibbsPlan P;
        std::string err;
        const int rc = fg_gibbs_plan(info, c.null_list ? nullptr : c.sites.data(), c.n, c.C, c.null_out ? nullptr : &P, &err);
        std::printf("refusal %s | %d | %s\n", c.name, rc, err.c_str());
    }
    {   // a model without a site to move: the automatic list is empty
        std::vector<FgGibbsSiteInfo> none = { X, Po, Big, Empty };
        FgGibbsPlan P;
        std::string err;
        const int rc = fg_gibbs_plan(none, nullptr, 0, 4, &P, &err);
        std::printf("refusal empty_list | %d | %s\n", rc, err.c_str());
    }
    std::string e;
    const int32_t rec_ok[] = { 0, 0, 3 }, rec_bad[] = { 0, 4 };
    const bool sweeps = fg_gibbs_check_sweeps(0, 0, &e) == FG_OK && fg_gibbs_check_sweeps(0xffffffffLL, 1, &e) == FG_OK && fg_gibbs_check_sweeps(0xffffffffLL, 2, &e) == FG_E_LIMIT &&
                        fg_gibbs_check_sweeps(5, -1, &e) == FG_E_BAD_ARG && fg_gibbs_check_sweeps(0, 0x7fffffff, &e) == FG_OK && fg_gibbs_check_sweeps(0x100000000LL, 0, &e) == FG_E_LIMIT &&
                        fg_gibbs_check_rec(4, rec_ok, 3, &e) == FG_OK && fg_gibbs_check_rec(4, nullptr, 0, &e) == FG_OK && fg_gibbs_check_rec(4, rec_bad, 2, &e) == FG_E_BAD_ARG &&
                        fg_gibbs_check_rec(4, nullptr, 1, &e) == FG_E_BAD_ARG && fg_gibbs_check_rec(4, rec_ok, -1, &e) == FG_E_BAD_ARG &&
                        fg_gibbs_support_size(0, 0) == 1 && fg_gibbs_support_size(1, 0) == 0 && fg_gibbs_support_size(-2, 5) == 8 &&
                        fg_gibbs_support_size(-9223372036854775807LL - 1, 9223372036854775807LL) == 0 && fg_gibbs_support_size(0, 9223372036854775807LL) == 0 && fg_gibbs_support_size(0, FG_GIBBS_K_CAP - 1) == FG_GIBBS_K_CAP;
    std::printf("sweeps %s\n", sweeps ? "ok" : "FAIL");
    return (bad || !sweeps) ? 1 : 0;
}
