// cstream_driver.cpp -- the streamed frequency tables on the host: fg_diag_cstream_plan.h (the planner the device code calls) with
// the kernel of fg_diag_cstream.hip replaced by a plain loop over the plan's launches.  tests/test_diag_cstream_cpu.py builds it
// with g++ (once more with -fsanitize=address,undefined) and compares its output with the numpy restatement.
//
//   cstream_driver run N_TOTAL N_REC C FORM ROWS VTYPES LO BINS FILE@C1,C2,... [SHORT]
//   cstream_driver split N_WATCH C N_CHUNK
//
// run: FORM = default | narrow | wide (FG_DIAG_CSTREAM_FORM); ROWS, VTYPES, LO, BINS comma-separated, one entry per watched row;
// FILE holds N_TOTAL x N_REC x C 8-byte cells ([n][n_rec][C], raw) and is fed in the listed chunk lengths.  SHORT (the test hook)
// leaves that many draws of the last chunk uncounted although the plan took them.  Prints "row K form F below B above A min M max X
// counts c0,c1,..." per watched row; an error of the planner is printed as "error RC MESSAGE" with exit status 2.
// split: the launch split of one chunk, from arithmetic only: "blocks B launches L draws D block_elements E".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_diag_cstream_plan.h"

static std::vector<long long> split_ints(const std::string &s) {
    std::vector<long long> out;
    size_t at = 0;
    while (at < s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        out.push_back(std::strtoll(s.substr(at, end - at).c_str(), nullptr, 10));
        at = end + 1;
    }
    return out;
}

static int fail(int rc, const std::string &msg) { std::printf("error %d %s\n", rc, msg.c_str()); return 2; }

static int usage() {
    std::fprintf(stderr, "usage: cstream_driver run N_TOTAL N_REC C FORM ROWS VTYPES LO BINS FILE@C1,C2,... [SHORT]\n"
                         "       cstream_driver split N_WATCH C N_CHUNK\n");
    return 1;
}

static int run_split(int n_watch, long long C, int n_chunk) {
    std::vector<int32_t> rows((size_t)n_watch), vt((size_t)n_watch, FG_BOOL), bins((size_t)n_watch, 2);
    std::vector<int64_t> lo((size_t)n_watch, 0);
    for (int k = 0; k < n_watch; ++k) rows[(size_t)k] = k;
    FgCsPlan P;
    std::string err;
    int rc = fg_cs_init(P, n_chunk, C, n_watch, rows.data(), vt.data(), lo.data(), bins.data(), n_watch, FG_CS_FORCE_NONE, &err);
    if (rc) return fail(rc, err);
    unsigned blocks = 0;
    std::vector<FgCsLaunch> launches;
    fg_cs_split(P, n_chunk, &blocks, launches);
    long long draws = 0, expect_t0 = 0;
    uint64_t most = 0;
    for (const FgCsLaunch &L : launches) {
        if (L.t0 != expect_t0 || L.n < 1) return fail(-100, "launches do not tile the chunk");
        expect_t0 += L.n; draws += L.n;
        most = std::max(most, fg_cs_block_elements(P, blocks, L));
    }
    std::printf("blocks %u launches %zu draws %lld block_elements %" PRIu64 "\n", blocks, launches.size(), draws, most);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    if (mode == "split") {
        if (argc != 5) return usage();
        return run_split(std::atoi(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]));
    }
    if (mode != "run" || argc < 11) return usage();
    const int n_total = std::atoi(argv[2]), n_rec = std::atoi(argv[3]);
    const long long C = std::atoll(argv[4]);
    const std::string form = argv[5];
    const int force = form == "narrow" ? FG_CS_FORCE_NARROW : form == "wide" ? FG_CS_FORCE_WIDE : FG_CS_FORCE_NONE;
    std::vector<int32_t> rows, vt, bins;
    std::vector<int64_t> lo;
    for (long long v : split_ints(argv[6])) rows.push_back((int32_t)v);
    for (long long v : split_ints(argv[7])) vt.push_back((int32_t)v);
    for (long long v : split_ints(argv[8])) lo.push_back((int64_t)v);
    for (long long v : split_ints(argv[9])) bins.push_back((int32_t)v);
    const int n_watch = (int)rows.size();
    if (vt.size() != rows.size() || lo.size() != rows.size() || bins.size() != rows.size()) return usage();
    const std::string spec = argv[10];
    const long long short_last = argc > 11 ? std::atoll(argv[11]) : 0;
    FgCsPlan P;
    std::string err;
    int rc = fg_cs_init(P, n_total, C, n_rec, rows.data(), vt.data(), lo.data(), bins.data(), n_watch, force, &err);
    if (rc) return fail(rc, err);
    const size_t at = spec.rfind('@');
    if (at == std::string::npos) return usage();
    std::vector<uint64_t> x((size_t)n_total * n_rec * C);
    FILE *f = std::fopen(spec.substr(0, at).c_str(), "rb");
    if (!f || std::fread(x.data(), 8, x.size(), f) != x.size()) { std::fprintf(stderr, "cannot read %s\n", spec.c_str()); return 1; }
    std::fclose(f);
    // the device state: the row table and the counter table
    std::vector<uint64_t> tab, ctr(fg_cs_words(P), 0);
    fg_cs_table(P, tab);
    uint64_t *below = ctr.data() + P.n_bins, *above = below + n_watch, *mn = above + n_watch, *mx = mn + n_watch;
    const std::vector<long long> chunks = split_ints(spec.substr(at + 1));
    long long t_done = 0;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const int n_c = (int)chunks[ci];
        rc = fg_cs_take(P, n_c, &err);
        if (rc) return fail(rc, err);
        const uint64_t *chunk = x.data() + (size_t)t_done * n_rec * C;
        const long long skip = ci + 1 == chunks.size() ? short_last : 0;
        unsigned blocks = 0;
        std::vector<FgCsLaunch> launches;
        fg_cs_split(P, n_c, &blocks, launches);
        for (const FgCsLaunch &L : launches) {
            if (fg_cs_block_elements(P, blocks, L) >= (1ull << 32)) return fail(-100, "a block would see 2^32 elements");
            for (int k = 0; k < n_watch; ++k) {                                 // k_diag_cstream_count, one grid row
                const uint64_t *t5 = &tab[(size_t)k * FG_CS_TAB_WORDS];
                const long long row = (long long)t5[0];
                const uint64_t klo = t5[1], flip = t5[4];
                const int nb = (int)(t5[2] & 0xffffffffull);
                const size_t off = (size_t)t5[3];
                for (long long t = L.t0; t < L.t0 + L.n && t < n_c - skip; ++t)
                    for (long long c = 0; c < C; ++c) {
                        const uint64_t key = chunk[((size_t)t * n_rec + row) * C + c] ^ flip;
                        const int b = fg_cs_bin(key, klo, nb);
                        if (b < 0) ++below[k]; else if (b == nb) ++above[k]; else ++ctr[off + (size_t)b];
                        mn[k] = std::max(mn[k], ~key); mx[k] = std::max(mx[k], key);
                    }
            }
        }
        t_done += n_c;
    }
    std::vector<uint64_t> counts(P.n_bins), h_below((size_t)n_watch), h_above((size_t)n_watch);
    std::vector<int64_t> h_min((size_t)n_watch), h_max((size_t)n_watch);
    rc = fg_cs_result(P, ctr.data(), counts.data(), h_below.data(), h_above.data(), h_min.data(), h_max.data(), &err);
    if (rc) return fail(rc, err);
    for (int k = 0; k < n_watch; ++k) {
        const FgCsRow &r = P.rows[(size_t)k];
        std::printf("row %d form %s below %" PRIu64 " above %" PRIu64, k, r.form == FG_CS_NARROW ? "narrow" : "wide", h_below[(size_t)k], h_above[(size_t)k]);
        if (r.vtype == FG_U64) std::printf(" min %" PRIu64 " max %" PRIu64 " counts ", (uint64_t)h_min[(size_t)k], (uint64_t)h_max[(size_t)k]);
        else std::printf(" min %" PRId64 " max %" PRId64 " counts ", h_min[(size_t)k], h_max[(size_t)k]);
        for (int j = 0; j < r.bins; ++j) std::printf("%s%" PRIu64, j ? "," : "", counts[r.off + (size_t)j]);
        std::printf("\n");
    }
    return 0;
}
