// fg_diag_cstream_plan.h -- the host side of the streamed frequency tables (fg_diag_cstream.hip): what the reference's callers do
// with extract_bool_values / extract_u64_values / extract_usize_values / extract_i64_values (diagnostics.rs:76-98) -- tabulate the
// values of a discrete site -- for a run that is handed over one chunk at a time and never stored.  Plain C++ (no HIP, no engine):
// the device code and tests/cpp/cstream_driver.cpp both call it, the latter with host loops in place of the kernel.
//
// A chunk is what fg_mh_step records: [n_chunk][n_rec][C] 8-byte cells, f64 rows and integer rows mixed.  The stream watches
// n_watch integer rows.  Watched row k keeps counts[bins_k] (bin j: cells equal to lo_k + j), `below` and `above` (the cells outside
// [lo_k, lo_k + bins_k)) and the smallest and largest cell seen, all 64-bit integers: sums of integers, so the tables do not depend
// on chunk boundaries or arrival order.  FG_U64 cells compare as unsigned, FG_BOOL / FG_USIZE / FG_I64 cells as signed; both become
// one unsigned comparison of KEYS, key = cell ^ flip with flip = 2^63 for the signed tags and 0 for FG_U64.
//
// Device counter table, 64-bit words, zeroed at creation (B = the sum of the rows' bins):
//   counts [B] (row k at rows[k].off) | below [n_watch] | above [n_watch] | mn [n_watch] (as ~key under atomicMax, so 0 is "none
//   yet") | mx [n_watch] (key under atomicMax)
// Device row table, 4 words per watched row: chunk row | key of lo | bins + (form << 32) | off, then flip in a fifth word.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fugue_amd.h"

#if defined(__HIPCC__)
#define FG_CS_HD __host__ __device__ __forceinline__
#else
#define FG_CS_HD inline
#endif

#define FG_CS_MAX_BINS 4096
#define FG_CS_NARROW_BINS 8          // the NARROW form: one ballot per bin, no LDS atomics
#define FG_CS_NARROW 0
#define FG_CS_WIDE 1
#define FG_CS_FORCE_NONE 0           // FG_DIAG_CSTREAM_FORM: unset | narrow | wide
#define FG_CS_FORCE_NARROW 1
#define FG_CS_FORCE_WIDE 2
#define FG_CS_THREADS 256
#define FG_CS_BLOCKS 2048            // blocks of a launch, over all watched rows
#define FG_CS_TAB_WORDS 5
// a thread takes at most this many elements of a launch: a block sees fewer than 2^32 (its u32 counters cannot wrap)
#define FG_CS_MAX_ITERS ((1ll << 24) - 1)

// where a cell falls: -1 below, `bins` above, else its bin.  klo = lo ^ flip.
FG_CS_HD int fg_cs_bin(uint64_t key, uint64_t klo, int bins) {
    if (key < klo) return -1;
    const uint64_t off = key - klo;
    return off < (uint64_t)bins ? (int)off : bins;
}

struct FgCsRow {
    int row = 0, vtype = 0, bins = 0, form = FG_CS_NARROW;
    int64_t lo = 0;
    uint64_t flip = 0, klo = 0;
    size_t off = 0;                  // of its counts in the counter table
};

struct FgCsPlan {
    int n_total = 0, n_rec = 0, n_watch = 0, count = 0;
    long long C = 0;
    size_t n_bins = 0;               // B
    std::vector<FgCsRow> rows;
};

struct FgCsLaunch { int t0 = 0, n = 0; };     // draws [t0, t0 + n) of the chunk

inline size_t fg_cs_words(const FgCsPlan &P) { return P.n_bins + 4 * (size_t)P.n_watch; }

// FG_E_BAD_ARG with *err set, or FG_OK.  C: the chains of one draw.  force: FG_CS_FORCE_* (narrow is ignored above 8 bins).
inline int fg_cs_init(FgCsPlan &P, int n_total, long long C, int n_rec, const int32_t *h_rows, const int32_t *h_vtypes, const int64_t *h_lo,
                      const int32_t *h_bins, int n_watch, int force, std::string *err) {
    std::string bad;
    if (n_total < 1) bad = "n_total < 1";
    else if (C < 1) bad = "no chains";
    else if (n_rec < 1) bad = "n_rec < 1";
    else if (n_watch < 1 || n_watch > 65535) bad = "n_watch must lie in [1, 65535]";
    else if (!h_rows || !h_vtypes || !h_lo || !h_bins) bad = "null table";
    if (bad.empty()) {
        std::vector<int32_t> seen(h_rows, h_rows + n_watch);
        std::sort(seen.begin(), seen.end());
        for (int k = 0; k < n_watch && bad.empty(); ++k) {
            const std::string at = "watched row " + std::to_string(k) + ": ";
            const int vt = h_vtypes[k];
            if (h_rows[k] < 0 || h_rows[k] >= n_rec) bad = at + "chunk row " + std::to_string(h_rows[k]) + " outside [0, n_rec)";
            else if (k > 0 && seen[k] == seen[k - 1]) bad = "chunk row " + std::to_string(seen[k]) + " is given twice";
            else if (vt == FG_F64) bad = at + "an f64 row has no frequency table";
            else if (vt != FG_BOOL && vt != FG_U64 && vt != FG_USIZE && vt != FG_I64) bad = at + "unknown value type " + std::to_string(vt);
            else if (h_bins[k] < 1 || h_bins[k] > FG_CS_MAX_BINS) bad = at + "bins must lie in [1, 4096]";
            else if (vt == FG_U64 && h_lo[k] < 0) bad = at + "lo of an unsigned row must not be negative";
            else if (vt != FG_U64 && h_lo[k] > INT64_MAX - (h_bins[k] - 1)) bad = at + "lo + bins overflows the row's integer type";
        }
    }
    if (!bad.empty()) { if (err) *err = "fg_diag_cstream_new: " + bad; return FG_E_BAD_ARG; }
    P = FgCsPlan();
    P.n_total = n_total; P.C = C; P.n_rec = n_rec; P.n_watch = n_watch;
    P.rows.resize((size_t)n_watch);
    for (int k = 0; k < n_watch; ++k) {
        FgCsRow &r = P.rows[(size_t)k];
        r.row = h_rows[k]; r.vtype = h_vtypes[k]; r.lo = h_lo[k]; r.bins = h_bins[k];
        r.flip = r.vtype == FG_U64 ? 0ull : 0x8000000000000000ull;
        r.klo = (uint64_t)r.lo ^ r.flip;
        r.form = r.bins <= FG_CS_NARROW_BINS && force != FG_CS_FORCE_WIDE ? FG_CS_NARROW : FG_CS_WIDE;
        r.off = P.n_bins;
        P.n_bins += (size_t)r.bins;
    }
    return FG_OK;
}

// the device row table
inline void fg_cs_table(const FgCsPlan &P, std::vector<uint64_t> &tab) {
    tab.assign((size_t)P.n_watch * FG_CS_TAB_WORDS, 0);
    for (int k = 0; k < P.n_watch; ++k) {
        const FgCsRow &r = P.rows[(size_t)k];
        uint64_t *t = &tab[(size_t)k * FG_CS_TAB_WORDS];
        t[0] = (uint64_t)r.row; t[1] = r.klo; t[2] = (uint64_t)r.bins | ((uint64_t)r.form << 32); t[3] = (uint64_t)r.off; t[4] = r.flip;
    }
}

// n_chunk more draws: FG_E_STATE past n_total
inline int fg_cs_take(FgCsPlan &P, int n_chunk, std::string *err) {
    if (n_chunk < 1) { if (err) *err = "fg_diag_cstream_update: n_chunk < 1"; return FG_E_BAD_ARG; }
    if (n_chunk > P.n_total - P.count) {
        if (err) *err = "fg_diag_cstream_update: " + std::to_string(P.count) + " + " + std::to_string(n_chunk) + " draws pass n_total = " + std::to_string(P.n_total);
        return FG_E_STATE;
    }
    P.count += n_chunk;
    return FG_OK;
}

// a launch that never ran gives its draws back
inline void fg_cs_untake(FgCsPlan &P, int n_chunk) { P.count -= n_chunk; }

// the u32 words of LDS histogram a block needs: the bins of the stream's widest WIDE row (a stream of NARROW rows: none)
inline int fg_cs_lds_bins(const FgCsPlan &P) {
    int most = 0;
    for (const FgCsRow &r : P.rows) if (r.form == FG_CS_WIDE) most = std::max(most, r.bins);
    return most;
}

// How a chunk of n_chunk draws is launched: `blocks` blocks of FG_CS_THREADS threads per watched row (grid x; grid y = n_watch), and
// the chunk cut into launches of whole draws so that a thread takes at most FG_CS_MAX_ITERS elements of a launch -- a block then
// sees fewer than 2^32, and neither its u32 LDS bins nor a wave's u32 counters can wrap.  Arithmetic only.
inline void fg_cs_split(const FgCsPlan &P, int n_chunk, unsigned *blocks, std::vector<FgCsLaunch> &launches) {
    const long long per_pass = FG_CS_THREADS * FG_CS_MAX_ITERS;                 // elements one block may see
    const long long total = (long long)n_chunk * P.C;
    long long nb = std::max<long long>(1, (FG_CS_BLOCKS + P.n_watch - 1) / P.n_watch);
    nb = std::min(nb, (total + FG_CS_THREADS - 1) / FG_CS_THREADS);
    nb = std::max(nb, (P.C + per_pass - 1) / per_pass);                         // one draw must fit a launch
    nb = std::max<long long>(nb, 1);
    const long long draws = std::max<long long>(1, std::min<long long>(n_chunk, nb * per_pass / P.C));
    *blocks = (unsigned)nb;
    launches.clear();
    for (long long t0 = 0; t0 < n_chunk; t0 += draws) {
        FgCsLaunch L;
        L.t0 = (int)t0; L.n = (int)std::min<long long>(draws, n_chunk - t0);
        launches.push_back(L);
    }
}
// the most elements one block of such a launch sees
inline uint64_t fg_cs_block_elements(const FgCsPlan &P, unsigned blocks, const FgCsLaunch &L) {
    const uint64_t total = (uint64_t)L.n * (uint64_t)P.C, threads = (uint64_t)blocks * FG_CS_THREADS;
    return (total + threads - 1) / threads * FG_CS_THREADS;
}

// The read-out from the counter table `ctr` (fg_cs_words words): FG_E_STATE before n_total draws, or when a row's counts + below +
// above is not n_total x C (the stream's integrity check).  h_counts: the rows' bins back to back; min / max as the cells' 64 bits.
inline int fg_cs_result(const FgCsPlan &P, const uint64_t *ctr, uint64_t *h_counts, uint64_t *h_below, uint64_t *h_above, int64_t *h_min, int64_t *h_max,
                        std::string *err) {
    if (P.count != P.n_total) {
        if (err) *err = "fg_diag_cstream_result: " + std::to_string(P.count) + " of " + std::to_string(P.n_total) + " draws have arrived";
        return FG_E_STATE;
    }
    if (!ctr || !h_counts || !h_below || !h_above || !h_min || !h_max) { if (err) *err = "fg_diag_cstream_result: null output"; return FG_E_BAD_ARG; }
    const size_t nw = (size_t)P.n_watch;
    const uint64_t *below = ctr + P.n_bins, *above = below + nw, *mn = above + nw, *mx = mn + nw;
    const uint64_t want = (uint64_t)P.n_total * (uint64_t)P.C;
    for (size_t k = 0; k < nw; ++k) {
        const FgCsRow &r = P.rows[k];
        uint64_t tot = below[k] + above[k];
        for (int j = 0; j < r.bins; ++j) tot += ctr[r.off + (size_t)j];
        if (tot != want) {
            if (err) *err = "fg_diag_cstream_result: watched row " + std::to_string(k) + " counted " + std::to_string(tot) + " cells where " +
                            std::to_string(want) + " arrived";
            return FG_E_STATE;
        }
    }
    std::memcpy(h_counts, ctr, P.n_bins * 8);
    for (size_t k = 0; k < nw; ++k) {
        h_below[k] = below[k]; h_above[k] = above[k];
        h_min[k] = (int64_t)(~mn[k] ^ P.rows[k].flip);
        h_max[k] = (int64_t)(mx[k] ^ P.rows[k].flip);
    }
    return FG_OK;
}
