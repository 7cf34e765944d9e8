// ppc_stream_driver.cpp -- the posterior predictive check stream on the host: fg_ppc_stream_plan.h and fg_chain_pool.h (the statistics,
// update, merge and finish functions the device code runs, the pieces, the launch cuts and the tree schedule) with the two kernels of
// fg_ppc_stream.hip and k_chain_pool replaced by plain loops.  tests/test_ppc_cpu.py builds it with g++ (once more with
// -fsanitize=address,undefined) and compares its output bit for bit with the Python restatement.
//
//   ppc_stream_driver N_TOTAL N_ROWS C SPEC TABLE C1,C2,... [MAX_GRID_X MAX_GRID_Y]
//
// SPEC: five text lines -- the value types [N_ROWS], the offsets [n_checks + 1], the member rows, the masks [n_checks], the observed
// values as 16 hex digits each (aligned with the members).  TABLE: N_TOTAL x N_ROWS x C raw 8-byte cells ([n][n_rows][C]), fed in
// chunks of C1, C2, ... draws.  Prints "tobs K HEX" per slot, "state K W" + C words as hex per slot and state word, "pooled K LT EQ GT
// NAN FIN MEAN SSD" per slot, then "launches L levels V slices S stat_launches P update_launches U".  An error of the plan is
// printed as "error RC MESSAGE" with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_ppc_stream_plan.h"

static int fail(int rc, const std::string &msg) { std::printf("error %d %s\n", rc, msg.c_str()); return 2; }

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

static std::vector<std::string> words(const std::string &line) {
    std::istringstream in(line);
    std::vector<std::string> out;
    for (std::string w; in >> w;) out.push_back(w);
    return out;
}

int main(int argc, char **argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: ppc_stream_driver N_TOTAL N_ROWS C SPEC TABLE C1,C2,... [MAX_GRID_X MAX_GRID_Y]\n"); return 1; }
    const int n_total = std::atoi(argv[1]), n_rows = std::atoi(argv[2]);
    const long long C = std::atoll(argv[3]);
    const long long gx = argc > 7 ? std::atoll(argv[7]) : FG_POOL_MAX_GRID_X;
    const long long gy = argc > 8 ? std::atoll(argv[8]) : FG_POOL_MAX_GRID_Y;
    std::ifstream spec(argv[4]);
    std::vector<int32_t> lists[4];                                                  // vtypes, offsets, members, masks
    std::vector<double> observed;
    std::string line;
    for (int i = 0; i < 5; ++i) {
        if (!std::getline(spec, line)) { std::fprintf(stderr, "cannot read line %d of %s\n", i, argv[4]); return 1; }
        for (const std::string &w : words(line)) {
            if (i < 4) lists[i].push_back((int32_t)std::atoi(w.c_str()));
            else { const unsigned long long u = std::strtoull(w.c_str(), nullptr, 16); double v; std::memcpy(&v, &u, 8); observed.push_back(v); }
        }
    }
    const int n_checks = (int)lists[3].size();
    if ((int)lists[0].size() != n_rows || (int)lists[1].size() != n_checks + 1 || lists[2].size() != observed.size()) {
        std::fprintf(stderr, "the lines of %s do not fit together\n", argv[4]);
        return 1;
    }
    // a list the plan must refuse may name more members than the lines hold: pad, so the driver itself reads nothing out of bounds
    const int32_t most = lists[1].empty() ? 0 : *std::max_element(lists[1].begin(), lists[1].end());
    if (most > 0 && (size_t)most > lists[2].size()) { lists[2].resize((size_t)most, 0); observed.resize((size_t)most, 0.0); }
    lists[2].push_back(0); observed.push_back(0.0);                                 // never empty
    FgPpcPlan P;
    std::string err;
    int rc = fg_ppc_init(P, n_total, C, n_rows, lists[0].data(), n_checks, lists[1].data(), lists[2].data(), lists[3].data(), observed.data(), &err, gx, gy);
    if (rc) return fail(rc, err);
    const long long stride = (long long)P.n_slots * C;
    std::vector<uint64_t> x((size_t)n_total * (size_t)n_rows * (size_t)C);
    FILE *f = std::fopen(argv[5], "rb");
    if (!f || std::fread(x.data(), 8, x.size(), f) != x.size()) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 1; }
    std::fclose(f);
    std::vector<double> state(fg_ppc_state_words(P), 0.0), scratch(fg_ppc_scratch_words(P), 0.0);      // zeroed, as the device state
    size_t stat_launches = 0, update_launches = 0;
    long long done = 0;
    const std::string chunks = argv[6];
    for (size_t at = 0; at < chunks.size();) {
        size_t end = chunks.find(',', at);
        if (end == std::string::npos) end = chunks.size();
        const int n_c = std::atoi(chunks.substr(at, end - at).c_str());
        at = end + 1;
        rc = P.draws.take(n_c, "fg_ppc_stream_update", &err);
        if (rc) return fail(rc, err);
        for (int t0 = 0; t0 < n_c; t0 += P.scratch_draws) {                         // fg_ppc_stream_update
            const int n_piece = std::min(P.scratch_draws, n_c - t0);
            const uint64_t *cells = x.data() + (size_t)(done + t0) * (size_t)n_rows * (size_t)C;
            for (const FgPoolLaunch &L : P.launches)                               // k_ppc_stream_stats
                for (const FgPoolSlice &S : fg_ppc_pair_slices(P, n_piece)) {
                    ++stat_launches;
                    for (long long y = 0; y < S.nk; ++y)
                        for (long long j = 0; j < L.cols; ++j) {
                            const long long c = L.col0 + j, p = S.k0 + y, t = p / P.n_checks;
                            const int q = (int)(p - t * P.n_checks);
                            const int o0 = P.offsets[q], K = P.offsets[q + 1] - o0, mask = P.mask[q];
                            const int32_t *members = P.members.data() + o0;
                            const uint64_t *base = cells + t * n_rows * C + c;
                            double T[FG_PPC_N_STATS];
                            fg_ppc_stats(K, [&](int i) { const int m = members[i]; return fg_ppc_cell(base[(long long)(m >> 2) * C], m & 3); }, (mask >> FG_PPC_VAR) & 1, T);
                            double *out = scratch.data() + (t * P.n_slots + P.slot0[q]) * C + c;
                            for (int st = 0; st < FG_PPC_N_STATS; ++st)
                                if ((mask >> st) & 1) { *out = T[st]; out += C; }
                        }
                }
            for (const FgPoolLaunch &L : P.launches)                               // k_ppc_stream_update
                for (const FgPoolSlice &S : P.slices) {
                    ++update_launches;
                    for (long long y = 0; y < S.nk; ++y)
                        for (long long j = 0; j < L.cols; ++j) {
                            const long long k = S.k0 + y, col = k * C + L.col0 + j;
                            FgPpcState s;
                            fg_ppc_state_load(s, state.data() + col, stride);
                            for (int t = 0; t < n_piece; ++t) fg_ppc_update(s, scratch[(size_t)((long long)t * stride + col)], P.t_obs[(size_t)k]);
                            fg_ppc_state_store(s, state.data() + col, stride);
                        }
                }
        }
        done += n_c;
    }
    rc = P.draws.complete("fg_ppc_stream_pooled", &err);
    if (rc) return fail(rc, err);
    const std::vector<FgPpcElem> cur = fg_pool_host<FgPpcPool>(P.levels, P.slices, state.data(), stride);     // k_chain_pool, level by level
    for (int k = 0; k < P.n_slots; ++k) std::printf("tobs %d %016llx\n", k, bits(P.t_obs[(size_t)k]));
    for (int k = 0; k < P.n_slots; ++k)
        for (int w = 0; w < FG_PPC_WORDS; ++w) {
            std::printf("state %d %d", k, w);
            for (long long c = 0; c < C; ++c) std::printf(" %016llx", bits(state[(size_t)(((long long)w * P.n_slots + k) * C + c)]));
            std::printf("\n");
        }
    for (int k = 0; k < P.n_slots; ++k) {
        double w[FG_PPC_ELEM], mom[2];
        int64_t cnt[5];
        FgPpcPool::elem_store(cur[(size_t)k], w);
        fg_ppc_finish(FgPpcPool::elem_load(w), cnt, mom);
        std::printf("pooled %d %lld %lld %lld %lld %lld %016llx %016llx\n", k, (long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3], (long long)cnt[4],
                    bits(mom[0]), bits(mom[1]));
    }
    std::printf("launches %zu levels %zu slices %zu stat_launches %zu update_launches %zu\n", P.launches.size(), P.levels.size(), P.slices.size(), stat_launches, update_launches);
    return 0;
}
