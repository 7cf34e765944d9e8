// Walks fg_pf_plan (fugue_amd/csrc/fg_pf_plan.h, the planner fg_pf.hip calls) over the particle counts given on the command line
// (the word `cap` stands for FG_PF_N_CAP, `cap+1` for one above it) and checks what a launch relies on: a workgroup of whole waves within
// the hardware's 1024 threads, the LDS within 160 KiB and large enough for the three arrays and the wave totals, every particle owned
// by exactly one (thread, slot) under both ownerships (the elementwise phases and sums: fg_pf_owner; the scan: fg_pf_scan_owner), and
// the cut of T steps into launches covering [0, T) exactly, in order, for T around the steps of a launch.  One line per point:
//   plan n | rc threads per_thread n_pad lds grid steps_per_launch | ok|FAIL <what>
// tests/test_pf_cpu.py reads the lines.  Built stand-alone with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_pf_plan.h"

static std::string check(long long n, long long B, FgPfPlan &P, int *rc_out) {
    const int rc = *rc_out = fg_pf_plan(n, B, &P);
    if (n > FG_PF_N_CAP) return rc == FG_E_LIMIT ? "ok" : "a filter above the cap was planned";
    if (n < 2) return rc == FG_E_BAD_ARG ? "ok" : "a filter below two particles was planned";
    if (rc) return "plan rc " + std::to_string(rc);
    if (P.n != n || P.grid != (unsigned)B) return "n or grid";
    if (P.threads < 64 || P.threads > 1024 || P.threads % 64 || (P.threads & (P.threads - 1))) return "threads";
    if (P.per_thread < 1 || (long long)P.per_thread * P.threads < n || (long long)(P.per_thread - 1) * P.threads >= n) return "per_thread";
    if (P.n_pad < n || P.n_pad % 2) return "n_pad";
    if (P.lds > 163840 || P.lds != (size_t)3 * P.n_pad * 8 + FG_PF_LDS_RESERVE || P.lds % 16) return "lds";
    if ((size_t)(6 * 16 + 16) * 8 > FG_PF_LDS_RESERVE) return "the reserve does not hold the wave totals";
    for (int form = 0; form < 2; ++form) {
        std::vector<int> owners((size_t)n, 0);
        for (int t = 0; t < P.threads; ++t)
            for (int k = 0; k < P.per_thread; ++k) {
                const int i = form ? fg_pf_scan_owner(P, t, k) : fg_pf_owner(P, t, k);
                if (i == -1) continue;
                if (i < 0 || i >= n) return "a slot outside [0, n)";
                owners[(size_t)i]++;
            }
        for (long long i = 0; i < n; ++i) if (owners[(size_t)i] != 1) return "particle " + std::to_string(i) + " owned " + std::to_string(owners[(size_t)i]) + " times";
    }
    if (P.steps_per_launch < 1 || P.steps_per_launch > FG_PF_MAX_STEPS_PER_LAUNCH) return "steps_per_launch";
    const long long spl = P.steps_per_launch, Ts[] = {0, 1, spl - 1, spl, spl + 1, 2 * spl, 2 * spl + 1, 1000};
    for (long long T : Ts) {
        if (T < 0) continue;
        long long at = 0;
        const long long L = fg_pf_n_launches(P, T);
        for (long long k = 0; k < L; ++k) {
            long long first, count;
            fg_pf_launch_steps(P, T, k, &first, &count);
            if (first != at || count < 1 || count > spl) return "launch " + std::to_string(k) + " of T = " + std::to_string(T);
            at += count;
        }
        long long first, count;
        fg_pf_launch_steps(P, T, L, &first, &count);
        if (at != T || count != 0) return "the launches do not cover T = " + std::to_string(T);
    }
    return "ok";
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        const long long n = !std::strcmp(argv[a], "cap") ? FG_PF_N_CAP : (!std::strcmp(argv[a], "cap+1") ? FG_PF_N_CAP + 1 : std::atoll(argv[a]));
        FgPfPlan P = {};
        int rc = 0;
        const std::string r = check(n, 7, P, &rc);
        std::printf("plan %lld | %d %d %d %d %zu %u %d | %s\n", n, rc, P.threads, P.per_thread, P.n_pad, P.lds, P.grid, P.steps_per_launch, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    FgPfPlan P;
    const bool refuses = fg_pf_plan(1, 1, &P) == FG_E_BAD_ARG && fg_pf_plan(-5, 1, &P) == FG_E_BAD_ARG && fg_pf_plan(64, 0, &P) == FG_E_BAD_ARG &&
                         fg_pf_plan(64, 1LL << 31, &P) == FG_E_BAD_ARG && fg_pf_plan(FG_PF_N_CAP + 1, 1, &P) == FG_E_LIMIT && fg_pf_plan(1LL << 40, 1, &P) == FG_E_LIMIT;
    std::printf("refusals %s\n", refuses ? "ok" : "FAIL");
    return (bad || !refuses) ? 1 : 0;
}
